"""PREDICT (csrc/resample.hpp / resample.hip: dpv_resample, dpv_resample_to) at its edge inputs against cpu_oracle.dpv_resample, within
the gate 24 * 2^-24 * max(max |dpv|, |pad|) derived in tests/resample_edges.py: points behind the camera, q_z = 0 on a whole plane,
coordinates clipped at both ends of all three axes (the dropped x1 / y1 / z1 taps), footprints on each of the six pad faces, D = 1
and 2 (every plane a face), both ends of the clamp and no clamp, new candidates, a non-finite pose.  tests/test_resample_edges_host.py
asserts without a GPU that the poses hold these voxels.  A kernel that took a tap in another cell than the oracle would miss the gate by
orders of magnitude (neighbouring values differ by ~10): that is a finding to explain, never to absorb."""
import numpy as np
import pytest
import torch

import resample_edges as rx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PADS = (-2.0, -5000.0)
_worst = {"fraction": 0.0}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _run(case, T, pad, clamp=(-1000.0, 0.0), d_out=None):
    from neuralrgbd_amd import ops
    zh, zr = rx.z_range(case["d_candi"], d_out is not None)
    d = case["d_candi"] if d_out is None else d_out
    out = ops.dpv_resample(_dev(case["dpv"]), _dev(T), _dev(case["rays"]), _dev(d), case["tan_hh"], case["tan_hv"], zh, zr, pad,
                           clamp=clamp, new_candi=d_out is not None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(name, case, T, pad, clamp=(-1000.0, 0.0), d_out=None):
    want = rx.oracle(case, T, pad, clamp, d_out)
    got = _run(case, T, pad, clamp, d_out)
    assert got.shape == want.shape
    gate = rx.gate(case, pad)
    diff = np.abs(got.astype(np.float64) - want)
    worst = float(diff.max()) if np.isfinite(diff).all() else float("inf")
    print("[parity] dpv_resample %-44s pad %7.1f: worst |diff| %.3e = %.3f of the gate %.3e, %d elements differ"
          % (name, pad, worst, worst / gate, gate, int((diff != 0).sum())))
    _worst["fraction"] = max(_worst["fraction"], worst / gate)
    assert worst <= gate, name
    return got, want


@pytest.mark.parametrize("pose", rx.POSES)
@pytest.mark.parametrize("D", rx.DEPTHS)
@pytest.mark.parametrize("h,w", rx.GRIDS)
def test_edge_poses_vs_oracle(h, w, D, pose):
    case = rx.make_case(h, w, D)
    T = rx.pose(pose, case["d_candi"])
    for pad in PADS:
        _check("%s %dx%dx%d" % (pose, h, w, D), case, T, pad)


@pytest.mark.parametrize("clamp", [(-1000.0, 0.0), None])
@pytest.mark.parametrize("pose", ["rot", "backward", "right_up"])
@pytest.mark.parametrize("h,w", rx.GRIDS)
def test_both_ends_of_the_clamp_and_no_clamp(h, w, pose, clamp):
    """Values in [-2000, 5]: with the clamp (-1000, 0) both ends act (asserted on the oracle's output in the host test); the same
    inputs with clamp=None keep what lies beyond them."""
    case = rx.make_case(h, w, 8, "wide")
    got, _ = _check("%s %dx%dx8 wide clamp=%s" % (pose, h, w, clamp is not None), case, rx.pose(pose, case["d_candi"]), -5000.0, clamp)
    if clamp is None:
        assert (got < -1000.0).sum() >= h and (got > 0.0).sum() >= 1
    else:
        assert got.min() == -1000.0 and got.max() == 0.0


@pytest.mark.parametrize("form", ["fewer", "more", "inverse"])
@pytest.mark.parametrize("pose", ["backward", "on_plane", "right_up", "left_down", "rot"])
@pytest.mark.parametrize("h,w,D", [(7, 9, 2), (20, 36, 8)])
def test_new_candidates_on_the_edge_poses(h, w, D, pose, form):
    """dpv_resample_to: fewer, more and differently spaced output planes than the source volume has."""
    case = rx.make_case(h, w, D)
    d_out = rx.new_candidates(case, form)
    got, _ = _check("%s %dx%dx%d -> %d planes (%s)" % (pose, h, w, D, len(d_out), form), case, rx.pose(pose, case["d_candi"]), -13.8,
                    d_out=d_out)
    assert got.shape[0] == len(d_out) and (form == "inverse" or len(d_out) != D)


@pytest.mark.parametrize("h,w", rx.GRIDS)
def test_identity_pose_reproduces_the_volume(h, w):
    """Output planes placed on the source planes (resample_edges.plane_aligned_candidates: the reference normalises z so that the
    source candidates themselves fall between the planes).  Against the oracle the gate holds as everywhere.  Against the volume
    itself the rounding of the POSITION comes on top: on each axis the coordinate chain has at most 8 roundings (ray, d * ray, the
    two divisions, g + 1, the product with the size, - 1; for z the two of (q_z - z_half) / z_radius and the candidate), each relative
    to a value of at most 2 * size before the halving: |f - integer| <= 8 * 2^-24 * size, doubled.  The output then moves by at most
    that times the difference between the two neighbours on that axis in the bordered volume.  Face voxels read pad."""
    D, pad = 8, -13.8
    case = rx.make_case(h, w, D)
    d_out = rx.plane_aligned_candidates(case)
    got, _ = _check("identity %dx%dx%d plane-aligned" % (h, w, D), case, rx.pose("identity", case["d_candi"]), pad, d_out=d_out)
    vol = rx.bordered(case, pad)
    tol = np.full(vol.shape, rx.gate(case, pad))
    for ax, size in enumerate((D, h, w)):
        step = np.abs(np.diff(vol, axis=ax))
        lo, hi = [(0, 0)] * 3, [(0, 0)] * 3
        lo[ax], hi[ax] = (1, 0), (0, 1)
        tol += 16 * rx.U * size * np.maximum(np.pad(step, lo), np.pad(step, hi))
    err = np.abs(got.astype(np.float64) - vol)
    print("[parity] dpv_resample identity %dx%dx%d vs the volume itself: worst error / tolerance %.3f" % (h, w, D, (err / tol).max()))
    assert (err <= tol).all()
    face = np.ones(vol.shape, bool)
    face[1:-1, 1:-1, 1:-1] = False
    assert np.abs(got[face] - np.float32(pad)).max() <= tol[face].max() and (~face).sum() == (D - 2) * (h - 2) * (w - 2)


@pytest.mark.parametrize("D", rx.DEPTHS)
@pytest.mark.parametrize("h,w", rx.GRIDS)
def test_non_finite_pose_entry(h, w, D):
    """T[0][3] = NaN and T[1][3] = inf.  The oracle: q_x is NaN and q_y infinite for every voxel, both coordinates clip to size - 1
    (ATen's clip_coordinates sends NaN there), x1 / y1 are dropped, and all remaining taps lie on the x = w - 1 face: every output
    is the pad value (times ez + wz = 1 up to rounding).  The kernel must give the same, so every index stayed inside the volume
    (the host test asserts the indices themselves from the same arithmetic)."""
    case = rx.make_case(h, w, D)
    T = rx.pose("nonfinite", case["d_candi"])
    got, want = _check("non-finite pose %dx%dx%d" % (h, w, D), case, T, -13.8)
    assert np.isfinite(got).all() and np.abs(want - np.float32(-13.8)).max() <= rx.gate(case, -13.8)
    got, _ = _check("non-finite pose %dx%dx%d no clamp" % (h, w, D), case, T, -5000.0, clamp=None)
    assert np.isfinite(got).all()


def test_report_worst_fraction_of_the_gate():
    """Last in the file: the worst observed fraction of the gate over the tests above (0 = the oracle's bits)."""
    print("[parity] dpv_resample worst |diff| / gate over this file: %.3f" % _worst["fraction"])
    assert _worst["fraction"] <= 1.0
