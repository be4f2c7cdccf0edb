"""Host-side checks of the frame-to-model tracking (csrc/icp.hip): the restatement of tests/icp_ref.py against finite differences,
Rodrigues' formula and np.linalg.solve; the mutants each gate of the GPU tests has to catch, with the fp32 restatement standing in for
the device; the conditions on the fixtures (the seeded inputs reach every branch, the corner fixture converges, a single plane is
singular); the C entries (declared, bound, exported, every refusal without a GPU and in the documented order).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import icp_ref as ir
import tsdf_raycast_ref as rc
from conftest import ROOT
from neuralrgbd_amd import _lib, synth

E_NULL, E_SHAPE, E_ALIGN, E_ARG = -1, -2, -3, -4
NAN, INF = float("nan"), float("inf")
ENTRIES = {"nrgbd_icp_workgroups": "int", "nrgbd_icp_workspace": "long", "nrgbd_icp_terms_f32": "int", "nrgbd_icp_update": "int"}


# ---- 1. the restatement against independent mathematics
def test_jacobian_against_central_differences():
    """J = (n, q x n) is d r / d(v, omega) of r(xi) = n . (Rw(omega) q + v - m) at xi = 0, float64."""
    rng = np.random.RandomState(3)
    for _ in range(20):
        q, m = rng.uniform(-1, 1, 3) + [0, 0, 2], rng.uniform(-1, 1, 3) + [0, 0, 2]
        n = rng.normal(0, 1, 3)
        n /= np.linalg.norm(n)
        J = np.concatenate([n, np.cross(q, n)])
        r = lambda xi: n @ (ir.rotation(xi[3:]) @ q + xi[:3] - m)
        h = 1e-6
        fd = np.array([(r(h * np.eye(6)[k]) - r(-h * np.eye(6)[k])) / (2 * h) for k in range(6)])
        assert np.abs(fd - J).max() < 1e-9, (fd, J)


@pytest.mark.parametrize("theta", [0.0, 1e-8, 0.1, 0.5])
def test_taylor_rotation_against_rodrigues(theta):
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    w = theta * axis
    R = ir.rotation(w)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    want = np.eye(3) + np.sin(theta) * Kx + (1 - np.cos(theta)) * (Kx @ Kx)
    print("[icp] theta %g: |R - Rodrigues| %.3g, |R R^T - I| %.3g" % (theta, np.abs(R - want).max(), np.abs(R @ R.T - np.eye(3)).max()))
    assert np.abs(R - want).max() <= 1e-15
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(R) - 1) <= 1e-15


def test_update_against_linalg_solve():
    recs, counts = ir.make_records(7)
    S = ir.add_records(recs)
    T0 = ir.init_motion()[:3]
    T, Tf, flag, its, row, rel = ir.update(S, int(counts.sum()), T0, 0, 0, 6, 1e-6)
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(ir.IDX):
        A[i, j] = A[j, i] = S[k]
    xi = np.linalg.solve(A, -S[21:27])
    got, _ = ir.solve(S, 1e-6)
    assert flag == 0 and its == 1 and np.abs(got - xi).max() <= 1e-12 * np.abs(xi).max() * np.linalg.cond(A)
    assert abs(row[2] - xi @ xi) <= 1e-12 and row[0] == counts.sum() and row[1] == S[27] and row[3] == 0
    th = np.linalg.norm(xi[3:])
    want = np.eye(4)
    want[:3, :3] = synth.rotvec_to_R(xi[3:]) if th > 0 else np.eye(3)
    want[:3, 3] = xi[:3]
    want = want @ ir.init_motion()
    assert np.abs(T - want[:3]).max() <= 1e-12
    assert np.array_equal(Tf, T.astype(np.float32)) and rel > 1e-4
    # the crafted systems recover the motion they were built from
    assert np.abs(xi - [0.02, -0.01, 0.015, 0.03, -0.02, 0.01]).max() < 2e-3


@pytest.mark.parametrize("kind,want", [("few", ir.FEW), ("nan", ir.NONFINITE), ("plane", ir.DEGENERATE), ("large", ir.LARGE)])
def test_update_flags_keep_the_motion_and_are_sticky(kind, want):
    recs, counts = ir.make_records(7, kind)
    T0 = ir.init_motion()[:3]
    T, Tf, flag, its, row, _ = ir.update(ir.add_records(recs), int(counts.sum()), T0, 0, 0, 6, 1e-6)
    assert flag == want and its == 0 and np.array_equal(T, T0) and row[3] == want
    good, gc = ir.make_records(7)
    T2, _, flag2, its2, row2, _ = ir.update(ir.add_records(good), int(gc.sum()), T, flag, its, 6, 1e-6)
    assert flag2 == want and its2 == 0 and np.array_equal(T2, T0) and row2[0] == gc.sum() and row2[3] == want


def test_the_order_of_the_flag_tests():
    recs, counts = ir.make_records(7, "nan")
    assert ir.update(ir.add_records(recs), 5, np.eye(4)[:3], 0, 0, 6, 1e-6)[2] == ir.FEW          # few before non-finite


# ---- 2. the fixtures
@pytest.mark.parametrize("H,W,sub", ir.TERMS_SIZES[1:])
def test_seeded_inputs_reach_every_branch(H, W, sub):
    case = ir.make_terms_case(H, W, sub)
    t = ir.terms_of(np.float32, case)
    visited = (H // sub) * (W // sub)
    print("[icp] %dx%d sub %d: %d of %d visited pixels accepted" % (H, W, sub, t["count"], visited))
    assert 0 < t["count"] < visited
    if visited >= 256:
        ar = np.abs(t["r"])
        assert (ar <= np.float32(case["huber"])).sum() > 5 and (ar > np.float32(case["huber"])).sum() > 5
        far = ir.terms(np.float32, case["depth"], case["K"], sub, case["mdepth"], case["mnormal"], case["Km"], case["T"].astype(np.float32),
                       100.0, case["huber"], case["depth_range"], case["gate"], case["gate_thr"])
        assert far["count"] > t["count"] + 5                        # pairs beyond dist_thr
        nogate = ir.terms(np.float32, case["depth"], case["K"], sub, case["mdepth"], case["mnormal"], case["Km"],
                          case["T"].astype(np.float32), case["dist_thr"], case["huber"], case["depth_range"])
        assert nogate["count"] > t["count"] + 5                     # pixels the gate excludes
        ident = ir.terms_of(np.float32, case, T=np.eye(4, dtype=np.float32)[:3])
        assert ident["count"] != t["count"]                         # the motion matters: pixels leave the map or fall behind


def test_fp32_terms_are_close_to_float64():
    case = ir.make_terms_case(48, 64, 1)
    a, b = ir.terms_of(np.float32, case), ir.terms_of(np.float64, case)
    both = ~np.isnan(a["resid"]) & ~np.isnan(b["resid"])
    assert both.sum() > 0.95 * max(a["count"], b["count"])
    assert np.abs(a["resid"][both] - b["resid"][both]).max() < 1e-5


def test_corner_fixture_converges_and_fp32_follows():
    """The all-float64 schedule on the corner fixture ends at least 10 x closer to the truth than it started, in translation and in
    rotation; otherwise the GPU test on it shows nothing.  Measured: 1.91 cm / 0.0406 rad -> 0.253 mm / 2.86e-4 rad, float64 and the
    fp32 restatement alike (75 x and 142 x closer); smallest relative pivot 0.055."""
    C = ir.CORNER
    vol = ir.corner_field(C["dims"], C["origin"], C["vs"], C["trunc"], C["planes"])
    truth, guess = ir.corner_poses()
    frame = rc.raycast(np.float32, vol[0], vol[1], C["origin"], C["vs"], truth, C["K"], C["size"], 0.0, INF, 1.0, None)
    assert frame["hit"].mean() > 0.9
    t0, r0 = ir.pose_error(guess, truth)
    assert 0.015 < t0 < 0.025 and 0.03 < r0 < 0.05
    for dtype in (np.float64, np.float32):
        s = ir.schedule(dtype, vol, C["origin"], C["vs"], frame["depth"], guess, C["K"], dist_thr=C["dist_thr"], huber=C["huber"])
        t1, r1 = ir.pose_error(s["extM"], truth)
        print("[icp] corner %s: %.3g m / %.3g rad -> %.3g m / %.3g rad, relative pivot %.3g" % (dtype.__name__, t0, r0, t1, r1, s["rel_pivot"]))
        assert s["flag"] == 0 and 10 * t1 <= t0 and 10 * r1 <= r0 and s["rel_pivot"] > 1e-3


def test_a_single_frontal_plane_is_singular():
    C = ir.CORNER
    vol = rc.linear_field(C["dims"], C["origin"], C["vs"], C["trunc"], (0.0, 0.0, -1.0), -2.0, np.float32)
    frame = rc.raycast(np.float32, vol[0], vol[1], C["origin"], C["vs"], np.eye(4), C["K"], C["size"], 0.0, INF, 1.0, None)
    assert frame["hit"].all()
    s = ir.schedule(np.float32, vol, C["origin"], C["vs"], frame["depth"], np.eye(4), C["K"], dist_thr=C["dist_thr"], huber=C["huber"])
    print("[icp] plane: flag %d, relative pivot %.3g" % (s["flag"], s["rel_pivot"]))
    assert s["flag"] == ir.DEGENERATE and abs(s["rel_pivot"]) < 1e-9 and np.array_equal(s["extM"], np.eye(4))


# ---- 3. the mutants: each leaves a gate of the GPU tests (the fp32 restatement stands in for the device)
def test_mutant_without_the_half_pixel_changes_the_residual_bits():
    case = ir.make_terms_case(48, 64, 2)
    a, b = ir.terms_of(np.float32, case), ir.terms_of(np.float32, case, mutant="half")
    assert not np.array_equal(a["resid"].view(np.int32), b["resid"].view(np.int32))


@pytest.mark.parametrize("mutant", ["cross_sign", "huber"])
def test_mutants_of_the_jacobian_and_the_weight_leave_the_sum_bound(mutant):
    """The residual map is the same; the sums are not: outside gamma_{N-1} S|t| on at least one of the 28."""
    case = ir.make_terms_case(48, 64, 1)
    a, b = ir.terms_of(np.float32, case), ir.terms_of(np.float32, case, mutant=mutant)
    assert np.array_equal(a["resid"].view(np.int32), b["resid"].view(np.int32)) and a["count"] == b["count"]
    assert (np.abs(b["sums"] - a["sums"]) > ir.sum_bound(a["abs_sums"], a["count"])).any()


@pytest.mark.parametrize("mutant", ["transpose", "swap"])
def test_mutants_of_the_update_change_the_state_bits(mutant):
    recs, counts = ir.make_records(7)
    S, T0 = ir.add_records(recs), ir.init_motion()[:3]
    a = ir.update(S, int(counts.sum()), T0, 0, 0, 6, 1e-6)
    b = ir.update(S, int(counts.sum()), T0, 0, 0, 6, 1e-6, mutant)
    assert not np.array_equal(ir.state_words(*a[:4]).view(np.int64), ir.state_words(*b[:4]).view(np.int64))


def test_the_order_of_additions_stays_inside_the_bound():
    """Any order of the additions — here the records' index order over a seeded split — meets the gate the GPU test applies."""
    case = ir.make_terms_case(48, 64, 1)
    a = ir.terms_of(np.float32, case)
    parts = np.array_split(a["terms"], 12)
    S = ir.add_records([p.sum(0) for p in parts])
    assert (np.abs(S - a["sums"]) <= ir.sum_bound(a["abs_sums"], a["count"])).all()


# ---- 4. the C entries
def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, res in ENTRIES.items():
        decl = re.search(r"\b%s %s\((.*?)\);" % (res, name), code, flags=re.S).group(1)
        assert decl.count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
        assert re.search(r"%s — no counterpart in the reference" % name, header)
        assert name in header[:header.index("#define NRGBD_INTERFACE_VERSION")]       # named in the list at the top
    assert header.count('#define NRGBD_INTERFACE_VERSION "0.10"') == 1                 # no entry changed or disappeared
    for name in ("MAX_WG", "RECORD_BYTES", "STATE_BYTES", "FEW", "NONFINITE", "DEGENERATE", "LARGE"):
        assert getattr(_lib, "ICP_" + name) == int(re.search(r"#define NRGBD_ICP_%s (\d+)" % name, header).group(1))
    assert _lib.ICP_MAX_THETA2 == float(re.search(r"#define NRGBD_ICP_MAX_THETA2 ([\d.]+)", header).group(1)) == ir.MAX_THETA2
    assert (_lib.ICP_FEW, _lib.ICP_NONFINITE, _lib.ICP_DEGENERATE, _lib.ICP_LARGE) == (ir.FEW, ir.NONFINITE, ir.DEGENERATE, ir.LARGE)
    assert _lib.ICP_RECORD_BYTES == 8 * ir.RECORD_WORDS and _lib.ICP_RECORD_BYTES % 16 == 0 and _lib.ICP_STATE_BYTES == 8 * ir.STATE_WORDS


def test_workgroups_and_workspace_need_no_gpu():
    from neuralrgbd_amd import ops
    for Hs, Ws in ((1, 1), (5, 7), (16, 16), (33, 65), (48, 64), (256, 256), (260, 256), (768, 1024)):
        assert ops.icp_workgroups(Hs, Ws) == ir.workgroups(Hs, Ws) == min(-(-Hs * Ws // 256), 256)
        assert ops.icp_workspace(Hs, Ws) == ir.workgroups(Hs, Ws) * 240
    assert ops.icp_workgroups(260, 256) == 256 and 260 * 256 > 256 * 256      # past the cap: the grid-stride loop runs
    lib = _lib.load()
    for Hs, Ws in ((0, 4), (4, -1), (32769, 1)):
        assert lib.nrgbd_icp_workgroups(Hs, Ws) == E_SHAPE and lib.nrgbd_icp_workspace(Hs, Ws) == E_SHAPE


P = ctypes.c_void_p(4096)                   # a non-NULL, aligned address: every refusal comes before anything touches the device
ODD = ctypes.c_void_p(4100)


def test_terms_refuses_bad_arguments_without_a_gpu():
    fn = _lib.load().nrgbd_icp_terms_f32

    def call(null=None, H=48, W=64, sub=2, Hm=24, Wm=32, fx=60., fy=60., cx=32., cy=24., fxm=30., fym=30., cxm=16., cym=12., d_near=0.,
             d_far=INF, dist_thr=.3, huber=.05, gate=P, gate_thr=0., state=P, partial=P, nbytes=240 * 3, resid=P):
        ptr = [None if i == null else p for i, p in enumerate((P, P, P, state, partial))]     # depth, mdepth, mnormal, state, partial
        return fn(ptr[0], gate, gate_thr, H, W, d_near, d_far, fx, fy, cx, cy, sub, ptr[1], ptr[2], Hm, Wm, fxm, fym, cxm, cym, ptr[3],
                  dist_thr, huber, ptr[4], nbytes, resid, None)
    for i in range(5):
        assert call(null=i) == E_NULL
    for kw in (dict(H=0), dict(W=-1), dict(Hm=0), dict(Wm=0), dict(sub=0), dict(sub=-2), dict(sub=49), dict(sub=65), dict(H=32769),
               dict(nbytes=240 * 3 - 1), dict(nbytes=0)):
        assert call(**kw) == E_SHAPE, kw
    for kw in (dict(fx=0.), dict(fx=NAN), dict(fy=-1.), dict(fy=INF), dict(fxm=0.), dict(fym=NAN), dict(cx=NAN), dict(cy=INF),
               dict(cxm=-INF), dict(cym=NAN), dict(dist_thr=0.), dict(dist_thr=NAN), dict(dist_thr=INF), dict(huber=0.), dict(huber=-1.),
               dict(huber=NAN), dict(d_near=1., d_far=1.), dict(d_near=2., d_far=1.), dict(d_near=NAN), dict(d_far=NAN),
               dict(gate_thr=NAN)):
        assert call(**kw) == E_ARG, kw
    assert call(state=ODD) == E_ALIGN and call(partial=ODD) == E_ALIGN
    # the order: NULL, shape, argument, alignment
    assert call(null=0, H=0, fx=0., state=ODD) == E_NULL and call(H=0, fx=0., state=ODD) == E_SHAPE
    assert call(nbytes=1, huber=0., partial=ODD) == E_SHAPE and call(fx=0., state=ODD) == E_ARG
    assert call(gate=None, gate_thr=NAN, state=ODD) == E_ALIGN       # gate and resid may be NULL; a NaN threshold without a gate is unused


def test_update_refuses_bad_arguments_without_a_gpu():
    fn = _lib.load().nrgbd_icp_update
    eye = (ctypes.c_double * 12)(*np.eye(4)[:3].reshape(-1))

    def call(state=P, init=eye, step=1, partial=P, nwg=3, min_pairs=6, min_pivot=1e-6, log=P):
        return fn(state, init, step, partial, nwg, min_pairs, min_pivot, log, None)
    assert call(state=None) == E_NULL and call(partial=None) == E_NULL and call(log=None) == E_NULL and call(state=None, step=0) == E_NULL
    for kw in (dict(step=-1), dict(nwg=0), dict(nwg=257), dict(nwg=-3)):
        assert call(**kw) == E_SHAPE, kw
    for kw in (dict(min_pivot=0.), dict(min_pivot=-1e-6), dict(min_pivot=NAN), dict(min_pivot=INF), dict(min_pairs=5), dict(min_pairs=0)):
        assert call(**kw) == E_ARG, kw
    for i, v in ((0, NAN), (7, INF), (11, -INF)):
        bad = (ctypes.c_double * 12)(*[v if j == i else x for j, x in enumerate(np.eye(4)[:3].reshape(-1))])
        assert call(step=0, init=bad) == E_ARG
        assert call(step=0, init=bad, state=ODD) == E_ARG
    assert call(state=ODD) == E_ALIGN and call(partial=ODD) == E_ALIGN and call(log=ODD) == E_ALIGN and call(state=ODD, step=0) == E_ALIGN
    # the order: NULL, shape, argument, alignment
    assert call(partial=None, nwg=0, min_pairs=0, state=ODD) == E_NULL and call(nwg=0, min_pairs=0, state=ODD) == E_SHAPE
    assert call(min_pairs=0, state=ODD) == E_ARG
