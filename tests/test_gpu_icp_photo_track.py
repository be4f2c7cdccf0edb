"""GPU: TSDFVolume.track(..., image=...) (tracking.FrameTracker(photo=True)) on the textured fixtures of tests/icp_photo_ref.py — the
single plane of tests/test_gpu_icp_track.py's degenerate case and its room corner, with a texture uploaded into a colour volume; the
frame's depth map and picture are ray cast on the device from the true pose.

Gate, as in tests/test_gpu_icp_track.py and with its floors (derived there): poses are compared after float32(extM[:3,:4]) rounding;
the tracker's error to the truth against the error e_ref the all-float64 comparator (icp_photo_ref.schedule_photo) ends with on the
same inputs, computed here: e_gpu <= 2 e_ref + floor.  Measured on an MI355X: see DESIGN.md row f16."""
import functools

import numpy as np
import pytest
import torch

import icp_photo_ref as pr
import icp_ref as ir
from neuralrgbd_amd import _lib, fusion
from test_gpu_icp_track import FLOOR_R, FLOOR_T, _error, _rounded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = ir.CORNER


def _volume(field, color=None):
    vol = fusion.TSDFVolume(C["dims"], C["vs"], C["origin"], trunc=C["trunc"], device=DEV, color=color is not None)
    vol.tsdf.copy_(torch.from_numpy(field[0]))
    vol.weight.copy_(torch.from_numpy(field[1]))
    if color is not None:
        vol.color.copy_(torch.from_numpy(color))
    return vol


@functools.lru_cache(maxsize=None)
def _fixture(name):
    """A textured fixture on the host and on the device, the frame (depth and picture ray cast on the device from the truth) and the
    float64 comparator's result from the guess on the same inputs: computed once, shared, never modified."""
    field, color, truth, guess = pr.plane_fixture() if name == "plane" else pr.corner_fixture()
    vol = _volume(field, color)
    depth, picture = vol.raycast(truth, C["K"], C["size"], color=True)
    assert float((depth > 0).float().mean()) > 0.9
    s = pr.schedule_photo(np.float64, field, color, C["origin"], C["vs"], depth.cpu().numpy(), picture.cpu().numpy(), None, guess, C["K"],
                          dist_thr=C["dist_thr"], huber=C["huber"])
    assert s["flag"] == 0
    return field, vol, truth, guess, depth, picture, (_error(s["extM"], truth), s)


def test_the_textured_plane_without_an_image_is_degenerate_and_returns_the_guess():
    """Today's behaviour, on a colour volume as well: the geometric track cannot see the in-plane motions."""
    field, vol, truth, guess, depth, picture, ref = _fixture("plane")
    res = vol.track(depth, guess, C["K"])
    assert not res.ok and res.flag == _lib.ICP_DEGENERATE and res.log[0, 3] == _lib.ICP_DEGENERATE
    assert np.array_equal(res.extM, _rounded(guess)) and np.array_equal(res.delta, np.eye(4))


@pytest.mark.parametrize("name", ["plane", "corner"])
def test_track_with_an_image_meets_the_comparator(name):
    field, vol, truth, guess, depth, picture, ((t_ref, r_ref), s) = _fixture(name)
    res = vol.track(depth, guess, C["K"], image=picture)           # the defaults: photo_weight = photo_huber = 0.1
    t0, r0 = _error(guess, truth)
    t_gpu, r_gpu = _error(res.extM, truth)
    print("[icp photo] %s from %.3g m / %.3g rad: GPU %.4g m / %.4g rad, float64 comparator %.4g m / %.4g rad; gates %.4g m / %.4g rad"
          % (name, t0, r0, t_gpu, r_gpu, t_ref, r_ref, 2 * t_ref + FLOOR_T, 2 * r_ref + FLOOR_R))
    print("[icp photo] %s pairs per level %s (comparator %s, photometric %s)"
          % (name, res.log[[0, 10, 15], 0], s["log"][[0, 10, 15], 0], s["photo_pairs"][[0, 10, 15]]))
    assert res.ok and res.flag == 0 and res.log.shape == (19, 4) and not res.log[:, 3].any()
    assert np.array_equal(res.extM, np.linalg.solve(res.delta, _rounded(guess)))
    assert t_gpu <= 2 * t_ref + FLOOR_T and r_gpu <= 2 * r_ref + FLOOR_R


def test_the_second_photometric_track_allocates_nothing_and_repeats_its_bits():
    field, vol, truth, guess, depth, picture, ref = _fixture("plane")
    first = vol.track(depth, guess, C["K"], image=picture)
    torch.cuda.synchronize()
    before, trackers = torch.cuda.memory_allocated(), len(vol._trackers)
    second = vol.track(depth, guess, C["K"], image=picture)
    assert torch.cuda.memory_allocated() == before and len(vol._trackers) == trackers
    assert np.array_equal(first.extM, second.extM) and np.array_equal(first.log, second.log)
    # the tracker cache is keyed on photo as well: the geometric track of the same size has a tracker of its own
    vol.track(depth, guess, C["K"])
    assert sorted(k[3] for k in vol._trackers) == [False, True]


def test_refusals():
    from neuralrgbd_amd import tracking
    field, vol, truth, guess, depth, picture, ref = _fixture("plane")
    plain = _volume(field)
    with pytest.raises(ValueError, match="colour volume"):
        plain.track(depth, guess, C["K"], image=picture)
    with pytest.raises(ValueError, match="colour volume"):
        tracking.FrameTracker(plain, C["size"], C["K"], photo=True)
    with pytest.raises(ValueError, match="photo=True"):
        tracking.FrameTracker(vol, C["size"], C["K"]).track(depth, guess, image=picture)
    photo = tracking.FrameTracker(vol, C["size"], C["K"], photo=True)
    with pytest.raises(ValueError, match="takes an image"):
        photo.track(depth, guess)
    with pytest.raises(ValueError, match="takes an image"):
        photo.residual_map(depth, guess)
    with pytest.raises(ValueError, match="image is"):
        photo.track(depth, guess, image=picture[:, :-1])


def test_photometric_residual_map_falls_at_the_tracked_pose():
    field, vol, truth, guess, depth, picture, ref = _fixture("plane")
    res = vol.track(depth, guess, C["K"], image=picture)
    tracker = next(t for k, t in vol._trackers.items() if k[3])
    geo, photo = tracker.residual_map(depth, guess, image=picture)
    assert tuple(geo.shape) == tuple(photo.shape) == C["size"]
    at_guess = photo.abs().nanmean().item()
    geo, photo = tracker.residual_map(depth, res.extM, image=picture)
    assert float(torch.isnan(photo).float().mean()) < 0.1
    at_tracked = photo.abs().nanmean().item()
    print("[icp photo] mean |intensity residual|: %.3g at the guess, %.3g at the tracked pose" % (at_guess, at_tracked))
    assert 5 * at_tracked < at_guess
