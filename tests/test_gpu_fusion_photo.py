"""GPU: fusion.FusionVideoStream(color=True, track=True, photo=True) against a hand-written loop — VideoDepthStream.push ->
ops.depth_regress -> TSDFVolume.track(image = the reference frame's ring slot, image_affine = (std, mean)) from the composed guess ->
TSDFVolume.integrate with the same picture — on the smallest configuration of tests/test_gpu_fusion_stream.py, built as
tests/test_gpu_fusion_track.py builds its stream.  Volume, colour and tracked poses are compared bit for bit.  With seeded weights
the depth maps are poor and losing track is an expected branch: the gate is equality with the loop, not success."""
import numpy as np
import pytest
import torch

import test_gpu_fusion_color as fc
import test_gpu_fusion_stream as fsn
import test_gpu_video as tv
from neuralrgbd_amd import fusion
from test_gpu_fusion_track import _same_poses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 1


def _hand_track(vol, photo):
    """The loop written out -> (tracked poses [(ref_index, extM, ok)], frames lost, the last pose integrated)."""
    frames, extMs, maps, pictures, (mean, std, H, W) = fc._hand(R)
    cam, d_candi = tv.gt.setup()
    prev, poses, lost, last = None, [], 0, None
    for ci in sorted(maps):
        depth = fsn._regress(maps[ci][0][0], d_candi)[0]
        pushed = np.asarray(extMs[ci], dtype=np.float64)
        pose = pushed
        if prev is not None:
            guess = pushed @ np.linalg.solve(prev[0], prev[1])
            kw = dict(image=pictures[ci], image_affine=(std, mean)) if photo else {}
            res = vol.track(depth, guess, cam, depth_range=fsn.DEPTH_RANGE, **kw)
            poses.append((ci, res.extM, res.ok))
            lost += 0 if res.ok else 1
            pose = res.extM
        assert vol.integrate(depth, pose, cam, depth_range=fsn.DEPTH_RANGE, color=pictures[ci],
                             color_intrinsics=fusion.intrinsics_at(cam, H, W), color_affine=(std, mean))
        prev, last = (pushed, pose), pose
    return poses, lost, last


def _same_colour_volume(a, b):
    fsn._same_volume(a, b)
    assert torch.equal(a.color.view(torch.int32), b.color.view(torch.int32)), "colour differs"


@pytest.mark.parametrize("mode", ["eager", "pipeline"])
def test_photo_stream_equals_the_hand_written_loop(mode):
    frames, extMs, maps, pictures, _ = fc._hand(R)
    want = fc._volume()
    poses, lost, last = _hand_track(want, photo=True)
    kw = dict(use_graph=False) if mode == "eager" else dict(use_graph=True, pipeline=True)
    vol = fc._volume()
    fs, outs = fsn._stream(R, frames, extMs, vol, color=True, track=True, photo=True, **kw)
    fsn._same_maps(outs, maps)
    print("[fusion-photo] %s: %d frames tracked, %d lost; flags %s" % (mode, len(poses), lost, [ok for _, _, ok in poses]))
    assert len(poses) == len(maps) - 1 and fs.n_integrated == len(maps)
    _same_poses(fs.tracked_poses, poses)
    assert fs.n_track_lost == lost and np.array_equal(fs.last_ext, last)
    _same_colour_volume(vol, want)
    assert int((want.weight > 0).sum()) > 1000
    assert [k[3] for k in vol._trackers] == [True]                  # the photometric tracker, and no other


def test_without_photo_the_stream_keeps_its_bits_and_builds_nothing_new():
    frames, extMs, maps, pictures, _ = fc._hand(R)
    want = fc._volume()
    poses, lost, last = _hand_track(want, photo=False)
    vol = fc._volume()
    fs, outs = fsn._stream(R, frames, extMs, vol, color=True, track=True, use_graph=False)
    assert fs.photo is False
    _same_poses(fs.tracked_poses, poses)
    assert fs.n_track_lost == lost
    _same_colour_volume(vol, want)
    assert [k[3] for k in vol._trackers] == [False]
    assert all(len(level[4]) == 2 and t._resid_photo is None for t in vol._trackers.values() for level in t._levels)


def test_refusals():
    model, cam, d_candi = tv._model(R)
    colour, plain = fc._volume(), fc._volume(False)
    for kw, vol in ((dict(color=False, track=True), plain), (dict(color=True, track=False), colour),
                    (dict(color=True, track=True, source="dpv"), colour)):
        with pytest.raises(ValueError, match="photo=True needs"):
            fusion.FusionVideoStream(model, cam, d_candi, vol, t_win_r=R, photo=True, **kw)
