"""The edge inputs of PREDICT (tests/resample_edges.py) checked on the CPU: each pose holds the voxels it is there for, counted from the
oracle's own arithmetic, and that arithmetic's restatement is held against the oracle itself."""
import numpy as np
import pytest

import resample_edges as rx


def _pops(h, w, D):
    case = rx.make_case(h, w, D)
    return case, {name: rx.population(case, rx.pose(name, case["d_candi"])) for name in rx.POSES}


@pytest.mark.parametrize("D", rx.DEPTHS)
@pytest.mark.parametrize("h,w", rx.GRIDS)
def test_edge_poses_hold_what_they_claim(h, w, D):
    case, pop = _pops(h, w, D)
    hw = h * w
    for name in rx.POSES:
        print("[inputs] resample %dx%dx%d %-9s %s" % (h, w, D, name, pop[name]))
        assert pop[name]["voxels"] == D * hw and pop[name]["indices_inside"]
    # coordinates clipped at 0 and at size - 1 on each axis; the latter are the dropped x1 / y1 / z1 taps
    assert pop["left_down"]["x_clip_lo"] >= h and pop["right_up"]["x_clip_hi"] >= h and pop["right_up"]["x_dropped_tap"] >= h
    assert pop["right_up"]["y_clip_lo"] >= w and pop["left_down"]["y_clip_hi"] >= w and pop["left_down"]["y_dropped_tap"] >= w
    assert pop["backward"]["z_clip_lo"] >= hw and pop["forward"]["z_clip_hi"] >= hw and pop["forward"]["z_dropped_tap"] >= hw
    # a footprint on each of the six pad faces
    assert pop["left_down"]["x_face_lo"] >= h and pop["right_up"]["x_face_hi"] >= h
    assert pop["right_up"]["y_face_lo"] >= w and pop["left_down"]["y_face_hi"] >= w
    assert pop["backward"]["z_face_lo"] >= hw and pop["forward"]["z_face_hi"] >= hw
    # q_z = 0 exactly on one whole plane; points behind the camera
    assert pop["on_plane"]["qz_zero_planes"] == 1 and pop["on_plane"]["qz_zero"] >= hw
    if D >= 2:
        assert pop["backward"]["behind"] >= hw and pop["on_plane"]["behind"] >= hw
        assert pop["rot"]["nonfinite"] == 0
    # with D of 1 or 2 every plane is a pad face
    for name in rx.POSES:
        assert (pop[name]["interior"] == 0) == (D <= 2 or name not in ("identity", "right_up", "left_down", "forward", "backward",
                                                                      "rot", "on_plane"))
    if D == 8:
        assert pop["identity"]["interior"] >= (h - 3) * (w - 3)


@pytest.mark.parametrize("values,clamp", [("logp", (-1000.0, 0.0)), ("wide", (-1000.0, 0.0)), ("wide", None)])
@pytest.mark.parametrize("h,w,D", [(7, 9, 2), (20, 36, 8), (7, 9, 1)])
def test_coordinate_restatement_vs_oracle(h, w, D, values, clamp):
    case = rx.make_case(h, w, D, values)
    for pad in (-2.0, -5000.0):
        for name in rx.POSES + ("nonfinite",):
            T = rx.pose(name, case["d_candi"])
            want = rx.oracle(case, T, pad, clamp)
            got = rx.float64_from_coordinates(case, T, pad, clamp)
            assert np.abs(got - want).max() <= 0.5 * rx.gate(case, pad), (name, pad)
        for form in ("fewer", "more", "inverse"):
            d_out = rx.new_candidates(case, form)
            T = rx.pose("rot", case["d_candi"])
            want = rx.oracle(case, T, pad, clamp, d_out)
            assert want.shape == (len(d_out), h, w)
            assert np.abs(rx.float64_from_coordinates(case, T, pad, clamp, d_out) - want).max() <= 0.5 * rx.gate(case, pad), form


def test_wide_values_reach_both_ends_of_the_clamp():
    for h, w in rx.GRIDS:
        case = rx.make_case(h, w, 8, "wide")
        for name in ("rot", "backward", "right_up"):
            T = rx.pose(name, case["d_candi"])
            clamped, free = rx.oracle(case, T, -5000.0), rx.oracle(case, T, -5000.0, clamp=None)
            assert (clamped == -1000.0).sum() >= h and (clamped == 0.0).sum() >= 1 and clamped.min() == -1000.0 and clamped.max() == 0.0
            assert (free < -1000.0).sum() >= h and (free > 0.0).sum() >= 1


def test_non_finite_pose_keeps_every_index_inside():
    """T[0][3] = NaN, T[1][3] = inf: x is NaN and y infinite for every voxel; both clip to size - 1 (a face), so every output is the
    pad value (weights (1, 0) on x and y; ez + wz = 1 up to rounding), clamped."""
    for h, w in rx.GRIDS:
        for D in rx.DEPTHS:
            case = rx.make_case(h, w, D)
            T = rx.pose("nonfinite", case["d_candi"])
            pop = rx.population(case, T)
            assert pop["nonfinite"] == D * h * w and pop["indices_inside"]
            assert pop["x_clip_hi"] == D * h * w and pop["y_clip_hi"] == D * h * w
            want = rx.oracle(case, T, -13.8)
            assert np.abs(want - np.float32(-13.8)).max() <= rx.gate(case, -13.8)
