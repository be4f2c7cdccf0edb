"""GPU: fusion.FusionVideoStream against a hand-built loop — VideoDepthStream.push -> ops.depth_regress -> TSDFVolume.integrate with
the extrinsic of the reference frame's push — on the model, sizes and synthetic sequence of tests/test_gpu_video.py.  The volume and
the returned maps are compared bit for bit: eager, hipGraph, pipelined with flush(), r = 2 and 1, both sources, confidence weights
behind a confidence gate, across a NaN pose and after reset().  The trace of a push holds no kernel outside nrgbd:: beyond those of
the bare VideoDepthStream."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_video as tv
from neuralrgbd_amd import fusion, ops, video
from neuralrgbd_amd import homography as warp_homo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS, VOXEL, ORIGIN = (64, 64, 48), 0.1, (-3.2, -3.2, 0.4)          # the candidates span 0.1 .. 5 m in front of a camera near the origin
DEPTH_RANGE = (0.2, 4.9)


def _volume():
    return fusion.TSDFVolume(DIMS, VOXEL, ORIGIN, device=DEV)


def _maps(r, frames, extMs):
    """{ref_index: (refined, dpv)} of an eager VideoDepthStream."""
    model, cam, d_candi = tv._model(r)
    vs = video.VideoDepthStream(model, cam, d_candi, t_win_r=r, copy_outputs=True, use_graph=False)
    maps = {}
    for f, e in zip(frames, extMs):
        out = vs.push(f, e)
        if out is not None:
            maps[out[0]] = (out[1].clone(), out[2].clone())
    assert vs.flush() is None
    torch.cuda.synchronize()
    vs.check()
    return maps


def _regress(vol, d_candi):
    d_dev = warp_homo._d_candi_dev(d_candi, vol.device)
    cl = ops.is_channels_last_view(vol)
    depth, logconf = ops.depth_regress(vol, d_dev, channels_last=cl)
    return depth, logconf, d_dev, cl


def _median_confidence(maps, source, d_candi):
    """A confidence that some but not all pixels of the sequence reach: the median of exp(max_k logp) over its maps."""
    conf = [np.exp(_regress(m[0 if source == "refined" else 1][0], d_candi)[1].cpu().numpy().astype(np.float64)) for m in maps.values()]
    return float(np.median(np.concatenate([c.reshape(-1) for c in conf])))


def _hand_integrate(vol, maps, extMs, source, weight, c):
    """The loop written out; returns the number of pixels (passing the gate, in all)."""
    cam, d_candi = tv.gt.setup()
    thr = None if c == 0 else float(np.log(np.float64(c)).astype(np.float32))
    passing = total = 0
    for ci in sorted(maps):
        v = maps[ci][0 if source == "refined" else 1][0]
        depth, logconf, d_dev, cl = _regress(v, d_candi)
        wmap = ops.export_depth_u16(v, d_dev, channels_last=cl)[1] if weight == "conf" else None
        assert vol.integrate(depth, extMs[ci], cam, gate=None if thr is None else logconf, gate_thr=thr, weight=wmap, depth_range=DEPTH_RANGE)
        if thr is not None:
            passing += int((logconf.cpu().numpy() >= np.float32(thr)).sum())
            total += logconf.numel()
    return passing, total


@functools.lru_cache(maxsize=None)
def _hand(r):
    """The sequence of window radius r and the maps of the bare stream on it, computed once."""
    frames, _, extMs = tv._sequence(r)
    return r, frames, extMs, _maps(r, frames, extMs)


def _stream(r, frames, extMs, vol, **kw):
    model, cam, d_candi = tv._model(r)
    fs = fusion.FusionVideoStream(model, cam, d_candi, vol, t_win_r=r, depth_range=DEPTH_RANGE, copy_outputs=True, **kw)
    assert isinstance(fs, video.VideoDepthStream) and fs.n_slots == 2 * r + 2
    outs = {}
    for f, e in zip(frames, extMs):
        o = fs.push(f, e)
        if o is not None:
            assert o[0] not in outs
            outs[o[0]] = (o[1].clone(), o[2].clone())
    o = fs.flush()
    if o is not None:
        outs[o[0]] = (o[1].clone(), o[2].clone())
    torch.cuda.synchronize()
    fs.check()
    return fs, outs


def _same_maps(outs, maps):
    assert sorted(outs) == sorted(maps)
    for c in maps:
        assert torch.equal(outs[c][0], maps[c][0]) and torch.equal(outs[c][1], maps[c][1]), "maps of frame %d differ" % c      # fusion perturbs nothing


def _same_volume(a, b):
    assert torch.equal(a.tsdf.view(torch.int32), b.tsdf.view(torch.int32)), "tsdf differs"
    assert torch.equal(a.weight.view(torch.int32), b.weight.view(torch.int32)), "weight differs"


SETTINGS = {"eager": (dict(use_graph=False), "refined", "uniform", False),
            "graph": (dict(use_graph=True), "dpv", "conf", True),
            "pipeline": (dict(use_graph=True, pipeline=True), "refined", "conf", True),
            "eager_dpv": (dict(use_graph=False), "dpv", "uniform", False)}


# both sources run eagerly at r = 1; r = 2 runs each of them in the other modes
@pytest.mark.parametrize("r,mode", [(2, "eager"), (2, "graph"), (2, "pipeline"), (1, "eager"), (1, "graph"), (1, "pipeline"), (1, "eager_dpv")])
def test_stream_equals_the_hand_built_loop(r, mode):
    r, frames, extMs, maps = _hand(r)
    kw, source, weight, gated = SETTINGS[mode]
    d_candi = tv.gt.setup()[1]
    c = _median_confidence(maps, source, d_candi) if gated else 0.0
    want = _volume()
    passing, total = _hand_integrate(want, maps, extMs, source, weight, c)
    if gated:
        print("[fusion] r=%d %s: confidence threshold %.4f passes %d of %d pixels" % (r, source, c, passing, total))
        assert 0 < passing < total                                  # the gate excludes some but not all pixels (downloaded maps)
    vol = _volume()
    fs, outs = _stream(r, frames, extMs, vol, source=source, weight=weight, conf_threshold=c, **kw)
    if kw["use_graph"]:
        assert fs.stream._graph is not None, fs.stream.graph_error
    assert sorted(outs) == list(range(r, len(frames) - r)) and fs.n_integrated == len(outs)
    _same_maps(outs, maps)
    _same_volume(vol, want)
    assert int((want.weight > 0).sum()) > 1000                      # the sequence lies inside the volume
    pts, found = vol.points(w_min=1.0)
    assert found == len(pts)


@pytest.mark.parametrize("device", [None, "cuda"])
def test_a_volume_on_the_default_device_joins_the_stream(device):
    """TSDFVolume's default device and "cuda" name the current device; the stream's device carries its index (cuda:0)."""
    r, frames, extMs, maps = _hand(1)
    vol = fusion.TSDFVolume(DIMS, VOXEL, ORIGIN, device=device)
    assert vol.device == vol.tsdf.device == torch.device("cuda", torch.cuda.current_device())
    fs, outs = _stream(r, frames, extMs, vol, use_graph=False)
    assert fs.device == vol.device
    want = _volume()
    _hand_integrate(want, maps, extMs, "refined", "uniform", 0.0)
    _same_maps(outs, maps)
    _same_volume(vol, want)
    pts, found = vol.points(w_min=1.0)
    assert pts.device == vol.device and found == len(pts)
    other = fusion.TSDFVolume((4, 3, 2), VOXEL, ORIGIN, device="cpu")
    with pytest.raises(ValueError, match="the volume is on cpu"):
        fusion.FusionVideoStream(tv._model(r)[0], *tv.gt.setup(), other, t_win_r=r)


def test_a_nan_pose_integrates_none_of_its_windows_and_reset_keeps_the_volume():
    r, frames, extMs, maps = _hand(1)                               # the NaN-pose sequence of tests/test_gpu_video.py
    bad = list(extMs)
    bad[3] = np.full((4, 4), np.nan)
    bad_maps = _maps(r, frames, bad)
    assert sorted(bad_maps) == [1, 5]
    want = _volume()
    _hand_integrate(want, bad_maps, bad, "refined", "uniform", 0.0)
    vol = _volume()
    fs, outs = _stream(r, frames, bad, vol, use_graph=False)
    _same_maps(outs, bad_maps)
    _same_volume(vol, want)
    assert fs.n_integrated == 2
    # reset() starts a trajectory and keeps the volume: the clean sequence on top of what is there
    fs.reset()
    assert fs.n_pushed == 0 and fs.ext_ring.held == [None] * fs.n_slots
    _same_volume(vol, want)
    assert fusion.fuse_sequence(fs, frames, extMs) == len(maps)
    _hand_integrate(want, maps, extMs, "refined", "uniform", 0.0)
    torch.cuda.synchronize()
    _same_volume(vol, want)


def test_a_push_launches_no_kernel_of_another_library():
    """Every kernel of a steady-state push of the fusion stream is a kernel of the library (nrgbd::) or one the bare VideoDepthStream
    launches as well.  The model has 64 candidates here (config B's count): the R-Net runs 64 or 128 candidate channels wide and hands
    its volume out as a view of those channels-last pixels, which is read where it lies; with the 8 candidates of the tests above the
    view is a slice of the padded pixels, which ops.depth_regress copies first."""
    from torch.profiler import ProfilerActivity, profile
    import neuralrgbd_amd
    from neuralrgbd_amd import synth
    r, frames, extMs, _ = _hand(1)
    cam = tv.gt.setup()[0]
    d_candi = np.linspace(tv.gt.TWIN["d_min"], tv.gt.TWIN["d_max"], 64)
    model = neuralrgbd_amd.KVNET(64, cam, d_candi, tv.gt.TWIN["sigma"], 64, None, if_refined=True, refineNet_name="DPV", t_win_r=r)
    model.load_state_dict(synth.seeded_state_dict(model, tv.gt.TWIN["weight_seed"]))
    model = model.to(DEV)
    streams = {"plain": video.VideoDepthStream(model, cam, d_candi, t_win_r=r, use_graph=False),
               "fusion": fusion.FusionVideoStream(model, cam, d_candi, _volume(), t_win_r=r, weight="conf", conf_threshold=0.05,
                                                  depth_range=DEPTH_RANGE, use_graph=False)}
    names = {}
    for key, s in streams.items():
        for f, e in zip(frames[:-1], extMs[:-1]):                   # caches warm, the filter in its update branch
            s.push(f, e)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            out = s.push(frames[-1], extMs[-1])
            torch.cuda.synchronize()
        assert out is not None and ops.is_channels_last_view(out[1][0])
        names[key] = {e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                      and "memset" not in e.name.lower()}
    assert streams["fusion"].n_integrated == len(frames) - 2 * r and bool((streams["fusion"].volume.weight > 0).any())
    new = names["fusion"] - names["plain"]
    assert any("tsdf_integrate_kernel" in n for n in new) and any("depth_rows_kernel" in n for n in new) and len(names["plain"]) > 5
    extra = sorted(n for n in new if "nrgbd::" not in n)
    assert not extra, extra
