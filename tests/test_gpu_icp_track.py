"""GPU: TSDFVolume.track (tracking.FrameTracker) on the corner fixture of tests/icp_ref.py — an analytic room corner uploaded into
the volume, the frame's depth map ray cast on the device from the true pose, the track started about 2 cm / 0.04 rad off.

Gate.  Poses are compared after float32(extM[:3,:4]) rounding, as the ray cast and the integration use them.  The tracker's error
to the truth is gated against the error e_ref the all-float64 comparator (icp_ref.schedule on tsdf_raycast_ref.raycast) ends with on
the same inputs, computed here: e_gpu <= 2 e_ref + floor.  The factor 2 covers association flips between the fp32 and the float64
model maps, which no bound captures.  The floor is the fp32 rounding of the two compared poses at the scene's scale S = 4 m (the power
of two above the volume's 2.4 m extent): every entry moves by at most 2^-24 of its size, a rotation by at most 3 x 2^-24 (Frobenius),
a translation by (sqrt(3) + 3) 2^-24 S (its own entries, and the rotation's error times the camera's distance) — twice that for two
poses: 3.6e-7 rad and 2.3e-6 m.  Measured on an MI355X: see DESIGN.md row f15."""
import functools
import math

import numpy as np
import pytest
import torch

import icp_ref as ir
import tsdf_raycast_ref as rc
from neuralrgbd_amd import _lib, fusion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = ir.CORNER
SCALE = 4.0
FLOOR_R = 2 * 3 * 2.0 ** -24
FLOOR_T = 2 * (math.sqrt(3.0) + 3.0) * 2.0 ** -24 * SCALE


def _volume(field):
    vol = fusion.TSDFVolume(C["dims"], C["vs"], C["origin"], trunc=C["trunc"], device=DEV)
    vol.tsdf.copy_(torch.from_numpy(field[0]))
    vol.weight.copy_(torch.from_numpy(field[1]))
    return vol


@functools.lru_cache(maxsize=None)
def _corner():
    """The corner volume on the host and on the device, the frame's depth map (device ray cast from the truth) and the comparator's
    final errors from the perturbed guess and from the truth: computed once, shared, never modified."""
    field = ir.corner_field(C["dims"], C["origin"], C["vs"], C["trunc"], C["planes"])
    vol = _volume(field)
    truth, guess = ir.corner_poses()
    depth = vol.raycast(truth, C["K"], C["size"])
    assert float((depth > 0).float().mean()) > 0.9
    host = depth.cpu().numpy()
    ref = {}
    for name, start in (("guess", guess), ("truth", truth)):
        s = ir.schedule(np.float64, field, C["origin"], C["vs"], host, start, C["K"], dist_thr=C["dist_thr"], huber=C["huber"])
        assert s["flag"] == 0
        ref[name] = (_error(s["extM"], truth), s)
    return field, vol, truth, guess, depth, ref


def _rounded(m):
    out = np.eye(4)
    out[:3, :4] = np.asarray(m)[:3, :4].astype(np.float32).astype(np.float64)
    return out


def _error(extM, truth):
    return ir.pose_error(_rounded(extM), _rounded(truth))


def test_track_from_a_perturbed_guess_meets_the_comparator():
    field, vol, truth, guess, depth, ref = _corner()
    (t_ref, r_ref), s = ref["guess"]
    res = vol.track(depth, guess, C["K"])                           # the defaults: dist_thr = 2 trunc = 0.3, huber = voxel_size = 0.05
    t0, r0 = _error(guess, truth)
    t_gpu, r_gpu = _error(res.extM, truth)
    print("[icp] corner from %.3g m / %.3g rad: GPU %.4g m / %.4g rad, float64 comparator %.4g m / %.4g rad; gates %.4g m / %.4g rad"
          % (t0, r0, t_gpu, r_gpu, t_ref, r_ref, 2 * t_ref + FLOOR_T, 2 * r_ref + FLOOR_R))
    print("[icp] pairs per level %s (comparator %s)" % (res.log[[0, 10, 15], 0], s["log"][[0, 10, 15], 0]))
    assert res.ok and res.flag == 0 and res.log.shape == (19, 4) and not res.log[:, 3].any()
    assert np.array_equal(res.delta[3], [0, 0, 0, 1]) and np.array_equal(res.extM, np.linalg.solve(res.delta, _rounded(guess)))
    assert t_gpu <= 2 * t_ref + FLOOR_T and r_gpu <= 2 * r_ref + FLOOR_R


def test_track_from_the_true_pose_stays():
    """The same gate, e_ref being the comparator's final error on these inputs: started from the truth.  The coarse levels pull the
    pose off (their pixel centres are not the full map's), the last level pulls it back: |xi|^2 falls."""
    field, vol, truth, guess, depth, ref = _corner()
    t_ref, r_ref = ref["truth"][0]
    res = vol.track(depth, truth, C["K"])
    t_gpu, r_gpu = _error(res.extM, truth)
    print("[icp] corner from the truth: GPU %.4g m / %.4g rad, float64 comparator %.4g m / %.4g rad; gates %.4g m / %.4g rad; |xi|^2 "
          "first %.3g last %.3g" % (t_gpu, r_gpu, t_ref, r_ref, 2 * t_ref + FLOOR_T, 2 * r_ref + FLOOR_R, res.log[0, 2], res.log[-1, 2]))
    assert res.ok and t_gpu <= 2 * t_ref + FLOOR_T and r_gpu <= 2 * r_ref + FLOOR_R
    assert res.log[-1, 2] < res.log[0, 2]


def test_a_single_plane_is_degenerate_and_returns_the_guess():
    field, vol, truth, guess, depth, ref = _corner()
    plane = rc.linear_field(C["dims"], C["origin"], C["vs"], C["trunc"], (0.0, 0.0, -1.0), -2.0, np.float32)
    pvol = _volume(plane)
    start = np.eye(4)
    start[:3, 3] = [0.01, -0.02, 0.015]
    pdepth = pvol.raycast(np.eye(4), C["K"], C["size"])
    assert bool((pdepth > 0).all())
    res = pvol.track(pdepth, start, C["K"])
    host = ir.schedule(np.float32, plane, C["origin"], C["vs"], pdepth.cpu().numpy(), start, C["K"], dist_thr=C["dist_thr"], huber=C["huber"])
    print("[icp] smallest relative pivot: plane %.3g, corner %.3g; min_pivot 1e-6 lies between"
          % (host["rel_pivot"], ref["guess"][1]["rel_pivot"]))
    assert abs(host["rel_pivot"]) < 1e-6 < ref["guess"][1]["rel_pivot"]
    assert not res.ok and res.flag == _lib.ICP_DEGENERATE and res.log[0, 3] == _lib.ICP_DEGENERATE and res.log[-1, 3] == _lib.ICP_DEGENERATE
    assert np.array_equal(res.extM, _rounded(start)) and np.array_equal(res.delta, np.eye(4))


def test_an_empty_volume_has_too_few_pairs():
    field, vol, truth, guess, depth, ref = _corner()
    empty = fusion.TSDFVolume(C["dims"], C["vs"], C["origin"], trunc=C["trunc"], device=DEV)
    res = empty.track(depth, guess, C["K"])
    assert not res.ok and res.flag == _lib.ICP_FEW and not res.log[:, 0].any() and np.array_equal(res.extM, _rounded(guess))


def test_the_second_track_allocates_nothing():
    field, vol, truth, guess, depth, ref = _corner()
    first = vol.track(depth, guess, C["K"])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    second = vol.track(depth, guess, C["K"])
    assert torch.cuda.memory_allocated() == before and len(vol._trackers) == 1
    assert np.array_equal(first.extM, second.extM) and np.array_equal(first.log, second.log)      # and gives the same bits


def test_residual_map_at_the_tracked_pose():
    field, vol, truth, guess, depth, ref = _corner()
    res = vol.track(depth, guess, C["K"])
    tracker = next(iter(vol._trackers.values()))
    at_guess = tracker.residual_map(depth, guess).abs().nan_to_num(0.0).mean().item()       # the frame placed at the guess: off
    r = tracker.residual_map(depth, res.extM)
    assert tuple(r.shape) == C["size"] and float(torch.isnan(r).float().mean()) < 0.1
    at_tracked = r.abs().nan_to_num(0.0).mean().item()
    print("[icp] mean |residual|: %.3g m at the guess, %.3g m at the tracked pose" % (at_guess, at_tracked))
    assert 5 * at_tracked < at_guess
