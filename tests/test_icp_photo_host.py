"""Host-side checks of the photometric term of the frame-to-model tracking (csrc/icp.hip: nrgbd_icp_terms_photo_f32): the restatement
of tests/icp_photo_ref.py against finite differences and against its own float64 form; the mutants each gate has to catch, with the
fp32 restatement standing in for the device; the pixels that lose the photometric term and keep the geometric one; the C entry
(declared, bound, exported, every refusal without a GPU and in the documented order); the conditions on the textured plane (the
geometric track is degenerate, the combined one converges).  No GPU."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import icp_photo_ref as pr
import icp_ref as ir
from conftest import ROOT
from neuralrgbd_amd import _lib

E_NULL, E_SHAPE, E_ALIGN, E_ARG = -1, -2, -3, -4
NAN, INF = float("nan"), float("inf")
U32 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _case(H, W, sub):
    """One seeded case with its fp32 and float64 restatements: computed once, shared, never modified."""
    case = pr.make_photo_case(H, W, sub)
    return case, pr.terms_photo_of(np.float32, case), pr.terms_photo_of(np.float64, case)


# ---- 1. the restatement against independent mathematics
def _bilinear(L, u, v):
    """The interpolant of the header at model coordinates (u, v), float64: pixel n's centre is at n + 0.5."""
    ub, vb = u - 0.5, v - 0.5
    x0, y0 = int(np.floor(ub)), int(np.floor(vb))
    fu, fv = ub - x0, vb - y0
    return (1 - fv) * (L[y0, x0] + fu * (L[y0, x0 + 1] - L[y0, x0])) + fv * (L[y0 + 1, x0] + fu * (L[y0 + 1, x0 + 1] - L[y0 + 1, x0]))


def test_photometric_jacobian_against_central_differences():
    """Ji is d ri / d(v, omega) of ri(xi) = Im(pi(Rw(omega) q + v)) - Lf at xi = 0, float64, along the six axes.

    Tolerance, derived.  Inside a cell Im is a polynomial of degree 2 in (u, v) (bilinear: one u v term) with coefficients bounded by
    the largest neighbour difference G; along an axis (u, v)(t) = pi(q(t)) is smooth with k-th derivatives of the order S^k,
    S = f (1 + |q|)^2 / q_z^2 model pixels per unit of xi (the quotient rule on q(t) = Rw(t e) q + t e).  A central difference of
    step h errs by h^2 / 6 max|f'''| <= h^2 G S^3 (the chain rule's terms of a degree-2 polynomial, each below G S^3; their count is
    covered by the 1 / 6), and by the rounding of two evaluations, 2 (8 u Lmax) / (2 h) with 8 roundings in an evaluation.  The
    points keep 0.2 of a model pixel from the cell's border and h S << 0.2, so no evaluation leaves the cell (the interpolant has a
    kink there).  With h = 1e-6, f = 60, |q| <= 2.5: about 5e-7 against |Ji| of the order G S = 100."""
    rng = np.random.RandomState(5)
    Hm, Wm, f, cxm, cym = 24, 32, 60.0, 16.0, 12.0
    L = rng.rand(Hm, Wm)
    h, checked = 1e-6, 0
    for _ in range(40):
        u, v = rng.uniform(2, Wm - 2), rng.uniform(2, Hm - 2)
        fr = np.array([u - 0.5, v - 0.5]) % 1.0
        if fr.min() < 0.2 or fr.max() > 0.8:
            continue
        z = rng.uniform(1.0, 2.0)
        q = np.array([(u - cxm) / f * z, (v - cym) / f * z, z])
        Lf = rng.rand()

        def ri(xi):
            p = ir.rotation(xi[3:]) @ q + xi[:3]
            return _bilinear(L, f * (p[0] / p[2]) + cxm, f * (p[1] / p[2]) + cym) - Lf
        ub, vb = u - 0.5, v - 0.5
        x0, y0 = int(np.floor(ub)), int(np.floor(vb))
        fu, fv = ub - x0, vb - y0
        gu0, gu1 = L[y0, x0 + 1] - L[y0, x0], L[y0 + 1, x0 + 1] - L[y0 + 1, x0]
        gu = (1 - fv) * gu0 + fv * gu1
        gv = (1 - fu) * (L[y0 + 1, x0] - L[y0, x0]) + fu * (L[y0 + 1, x0 + 1] - L[y0, x0 + 1])
        ax, ay = gu * f / q[2], gv * f / q[2]
        a = np.array([ax, ay, -(ax * (q[0] / q[2]) + ay * (q[1] / q[2]))])
        Ji = np.concatenate([a, np.cross(q, a)])
        fd = np.array([(ri(h * np.eye(6)[k]) - ri(-h * np.eye(6)[k])) / (2 * h) for k in range(6)])
        G = np.abs(np.diff(L[y0:y0 + 2, x0:x0 + 2], axis=0)).max() + np.abs(np.diff(L[y0:y0 + 2, x0:x0 + 2], axis=1)).max()
        S = f * (1 + np.linalg.norm(q)) ** 2 / q[2] ** 2
        assert h * S < 0.02
        tol = h * h * G * S ** 3 + 8 * 2.0 ** -53 * 1.0 / h
        assert np.abs(fd - Ji).max() <= tol, (fd, Ji, tol)
        checked += 1
    assert checked >= 10


def test_the_restatement_computes_that_jacobian():
    """terms_photo's own float64 Ji, at its own q and cell, against central differences of the residual (the tolerance of the test
    above, with the case's intrinsics), and Ji, ri and wi against the formulas of that test evaluated pixel by pixel in plain
    Python: the restatement the GPU tests compare the kernel with is tied to the mathematics, the translational half included."""
    case, _, t = _case(48, 64, 2)
    fxm, fym, cxm, cym = (float(np.float32(k)) for k in case["Km"])
    md, mc = case["mdepth"].astype(np.float64), case["mrgb"].astype(np.float64)
    L = (np.float64(np.float32(0.299)) * mc[0] + np.float64(np.float32(0.587)) * mc[1]) + np.float64(np.float32(0.114)) * mc[2]
    assert t["photo_count"] > 50
    differenced = 0
    for k in range(t["photo_count"]):
        q = t["q"][k]
        u, v = fxm * (q[0] / q[2]) + cxm, fym * (q[1] / q[2]) + cym
        x0, y0 = int(np.floor(u - 0.5)), int(np.floor(v - 0.5))
        assert (x0, y0) == tuple(t["cell"][k])
        Im = _bilinear(L, u, v)
        y, x = t["pixel"][k]
        a, b = (np.float32(w).astype(np.float64) for w in case["affine"])
        cimg = case["image"][:, y, x].astype(np.float64) * a + b
        Lf = (np.float64(np.float32(0.299)) * cimg[0] + np.float64(np.float32(0.587)) * cimg[1]) + np.float64(np.float32(0.114)) * cimg[2]
        assert abs((Im - Lf) - t["ri"][k]) <= 1e-14
        assert t["wi"][k] == (np.float64(np.float32(0.1)) if abs(t["ri"][k]) <= np.float32(0.1) else
                              np.float64(np.float32(0.1)) * (np.float64(np.float32(0.1)) / abs(t["ri"][k])))
        fu, fv = (u - 0.5) - x0, (v - 0.5) - y0
        gu = (1 - fv) * (L[y0, x0 + 1] - L[y0, x0]) + fv * (L[y0 + 1, x0 + 1] - L[y0 + 1, x0])
        gv = (1 - fu) * (L[y0 + 1, x0] - L[y0, x0]) + fu * (L[y0 + 1, x0 + 1] - L[y0, x0 + 1])
        ax, ay = gu * fxm / q[2], gv * fym / q[2]
        a3 = np.array([ax, ay, -(ax * (q[0] / q[2]) + ay * (q[1] / q[2]))])
        want = np.concatenate([a3, np.cross(q, a3)])
        assert np.abs(t["Ji"][k] - want).max() <= 1e-12 * (1 + np.abs(want).max()), (t["Ji"][k], want)
        if min(fu, fv) < 0.1 or max(fu, fv) > 0.9:                  # a difference would cross the cell's border: a kink
            continue

        def ri(xi):
            p = ir.rotation(xi[3:]) @ q + xi[:3]
            return _bilinear(L, fxm * (p[0] / p[2]) + cxm, fym * (p[1] / p[2]) + cym) - Lf
        h = 1e-6
        fd = np.array([(ri(h * np.eye(6)[i]) - ri(-h * np.eye(6)[i])) / (2 * h) for i in range(6)])
        blk = L[y0:y0 + 2, x0:x0 + 2]
        G = np.abs(np.diff(blk, axis=0)).max() + np.abs(np.diff(blk, axis=1)).max()
        S = max(fxm, fym) * (1 + np.linalg.norm(q)) ** 2 / q[2] ** 2
        assert h * S < 0.01
        tol = h * h * G * S ** 3 + 8 * 2.0 ** -53 * (np.abs(blk).max() + abs(Lf)) / h
        assert np.abs(fd - t["Ji"][k]).max() <= tol, (fd, t["Ji"][k], tol)
        differenced += 1
    assert differenced >= 5


def test_fp32_restatement_within_the_rounding_bound_of_float64():
    """|ri_32 - ri_64| at every pixel both forms give a photometric pair, against a per-pixel bound derived from the sequence.

    With u = 2^-24 and every input the same fp32 value on both sides: q_j is four operations on products of the pose and the point
    (the point itself three more), so |dq_j| <= 8 u Q_j, Q_j = sum_k |T_jk p_k| + |t_j|; xq = q_x / q_z: |dxq| <= u |xq| + (8 u Q_x +
    |xq| 8 u Q_z) / q_z; the model coordinate: |du| <= fxm |dxq| + 2 u (|fxm xq| + |cxm|), ub = u - 0.5 one more u |u|.  The interpolant
    is continuous across cells with slopes |gu|, |gv| <= G, the largest neighbour difference around the point (both forms' cells:
    the 4 x 4 block around the cell covers a flip), so the coordinates move Im by at most G (|du| + |dv|).  Its own operations:
    5 per luminance and 10 for the interpolation on values <= Lmax (16 Lmax u covers them), 7 for Lf on |c| <= Cmax (8), one for the
    difference: (16 Lmax + 8 Cmax + |ri|) u; the whole doubled for the second-order terms the first-order form leaves out."""
    case, a, b = _case(48, 64, 1)
    both = ~np.isnan(a["resid_photo"]) & ~np.isnan(b["resid_photo"])
    assert both.sum() > 0.9 * max(a["photo_count"], b["photo_count"]) > 100
    T = case["T"].astype(np.float32).astype(np.float64)
    fx, fy, cx, cy = (float(np.float32(k)) for k in case["K"])
    fxm, fym, cxm, cym = (float(np.float32(k)) for k in case["Km"])
    mc = case["mrgb"].astype(np.float64)
    L = (0.299 * mc[0] + 0.587 * mc[1]) + 0.114 * mc[2]
    worst = 0.0
    for y, x in zip(*np.nonzero(both)):
        d = float(case["depth"][y, x])
        p = np.array([((x + 0.5) - cx) / fx * d, ((y + 0.5) - cy) / fy * d, d])
        Q = np.abs(T[:, :3] * p[None, :]).sum(1) + np.abs(T[:, 3])
        q = T[:, :3] @ p + T[:, 3]
        xq, yq = q[0] / q[2], q[1] / q[2]
        dxq = U32 * abs(xq) + (8 * U32 * Q[0] + abs(xq) * 8 * U32 * Q[2]) / q[2]
        dyq = U32 * abs(yq) + (8 * U32 * Q[1] + abs(yq) * 8 * U32 * Q[2]) / q[2]
        u, v = fxm * xq + cxm, fym * yq + cym
        du = fxm * dxq + 2 * U32 * (abs(fxm * xq) + abs(cxm)) + U32 * abs(u)
        dv = fym * dyq + 2 * U32 * (abs(fym * yq) + abs(cym)) + U32 * abs(v)
        x0, y0 = int(np.floor(u - 0.5)), int(np.floor(v - 0.5))
        blk = L[max(y0 - 1, 0):y0 + 3, max(x0 - 1, 0):x0 + 3]
        blk = blk[np.isfinite(blk)]
        G, Lmax = blk.max() - blk.min(), np.abs(blk).max()
        aa, bb = (np.float32(w).astype(np.float64) for w in case["affine"])
        Cmax = np.abs(case["image"][:, y, x].astype(np.float64) * aa).max() + np.abs(bb).max()
        bound = 2 * (G * (du + dv) + (16 * Lmax + 8 * Cmax + abs(b["resid_photo"][y, x])) * U32)
        diff = abs(float(a["resid_photo"][y, x]) - b["resid_photo"][y, x])
        worst = max(worst, diff / bound)
        assert diff <= bound, (y, x, diff, bound)
    print("[icp photo] fp32 against float64 at %d pixels: worst |d ri| / bound %.3g" % (both.sum(), worst))


# ---- 2. the fixtures and the pixels that lose the term
@pytest.mark.parametrize("H,W,sub", pr.TERMS_SIZES[1:])
def test_seeded_inputs_reach_every_branch(H, W, sub):
    case, t, _ = _case(H, W, sub)
    geo = ir.terms_of(np.float32, case)
    assert np.array_equal(t["resid"].view(np.int32), geo["resid"].view(np.int32)) and t["count"] == geo["count"]
    assert np.array_equal(np.isnan(t["resid"]) | np.isnan(t["resid_photo"]), np.isnan(t["resid_photo"]))     # a term needs its pair
    print("[icp photo] %dx%d sub %d: %d geometric pairs, %d photometric" % (H, W, sub, t["count"], t["photo_count"]))
    assert t["photo_count"] <= t["count"]
    if (H // sub) * (W // sub) >= 256:
        assert 0 < t["photo_count"] < t["count"]
        ar = np.abs(t["ri"])
        assert (ar <= np.float32(0.1)).sum() > 5 and (ar > np.float32(0.1)).sum() > 5      # both sides of photo_huber
        loose = pr.terms_photo_of(np.float32, case, mutant="no_occlusion")
        assert loose["photo_count"] > t["photo_count"] + 5                                 # neighbours on another surface


def test_one_by_one_has_no_photometric_pair():
    case, t, _ = _case(1, 1, 1)
    assert t["photo_count"] == 0 and np.isnan(t["resid_photo"]).all()


def _flat_case():
    """A frontal plane at 2 m seen by coincident cameras, identity motion, constant colour: every pixel has both pairs but those whose
    2 x 2 neighbourhood leaves the map."""
    H, W = 12, 16
    K = (16.0, 16.0, 8.0, 6.0)                                      # a power of two: every coordinate is exact
    depth = np.full((H, W), 2.0, np.float32)
    mn = np.zeros((3, H, W), np.float32)
    mn[2] = -1.0
    img = np.full((3, H, W), 0.5, np.float32)
    rgb = np.full((3, H, W), 0.25, np.float32)
    return dict(depth=depth, K=K, sub=1, mdepth=depth.copy(), mnormal=mn, Km=K, T=np.eye(4, dtype=np.float32)[:3], dist_thr=0.3,
                huber=0.05, image=img, affine=None, mrgb=rgb)


def _flat(case):
    return pr.terms_photo(np.float32, case["depth"], case["K"], 1, case["mdepth"], case["mnormal"], case["Km"], case["T"], 0.3, 0.05,
                          case["image"], None, case["mrgb"])


def test_border_missed_neighbour_and_nan_colour_lose_the_term_alone():
    """With coincident cameras pixel (y, x) projects to its own centre, u - 0.5 = x: its cell is (x, y) .. (x + 1, y + 1), so the last
    row and the last column have no fourth neighbour.  A hole or a NaN colour at a neighbour takes the term from the (up to four)
    pixels whose cell holds it; the geometric pair goes only where the pixel's own model depth does."""
    base = _flat_case()
    t = _flat(base)
    H, W = base["depth"].shape
    assert t["count"] == H * W
    has = ~np.isnan(t["resid_photo"])
    assert has[:-1, :-1].all() and not has[-1, :].any() and not has[:, -1].any() and t["photo_count"] == (H - 1) * (W - 1)
    assert np.array_equal(t["resid_photo"][has], np.full(has.sum(), pr.luma(np.float32, *[np.float32(0.25)] * 3) - pr.luma(np.float32, *[np.float32(0.5)] * 3), np.float32))
    hole = dict(base, mdepth=base["mdepth"].copy())
    hole["mdepth"][5, 7] = 0.0
    t = _flat(hole)
    lost = ~np.isnan(t["resid"]) & np.isnan(t["resid_photo"])
    assert np.isnan(t["resid"][5, 7]) and t["count"] == H * W - 1
    assert lost[4, 6] and lost[4, 7] and lost[5, 6] and not np.isnan(t["resid_photo"][5, 8]) and not np.isnan(t["resid_photo"][6, 7])
    step = dict(base, mdepth=base["mdepth"].copy())
    step["mdepth"][5, 7] = 2.2                                      # a depth step of 0.2 m under dist_thr = 0.15: another surface
    tight = pr.terms_photo(np.float32, step["depth"], step["K"], 1, step["mdepth"], step["mnormal"], step["Km"], step["T"], 0.15, 0.05,
                           step["image"], None, step["mrgb"])
    assert tight["count"] == H * W - 1 and np.isnan(tight["resid_photo"][4, 6]) and not np.isnan(tight["resid"][4, 6])
    nan = dict(base, mrgb=base["mrgb"].copy())
    nan["mrgb"][1, 5, 7] = np.nan
    t = _flat(nan)
    lost = ~np.isnan(t["resid"]) & np.isnan(t["resid_photo"])
    assert t["count"] == H * W and t["photo_count"] == (H - 1) * (W - 1) - 4 and lost[4:6, 6:8].all()
    frame = dict(base, image=base["image"].copy())
    frame["image"][2, 3, 3] = np.inf
    t = _flat(frame)
    assert t["count"] == H * W and t["photo_count"] == (H - 1) * (W - 1) - 1 and np.isnan(t["resid_photo"][3, 3])
    assert np.isfinite(t["sums"]).all()


# ---- 3. the mutants: each leaves the gate it targets (the fp32 restatement stands in for the device)
def test_mutant_without_the_shift_changes_the_photometric_residual_bits():
    case, a, _ = _case(48, 64, 2)
    b = pr.terms_photo_of(np.float32, case, mutant="no_shift")
    assert np.array_equal(a["resid"].view(np.int32), b["resid"].view(np.int32))
    assert not np.array_equal(a["resid_photo"].view(np.int32), b["resid_photo"].view(np.int32))


def test_mutant_without_the_occlusion_test_changes_the_photometric_count():
    case, a, _ = _case(48, 64, 1)
    b = pr.terms_photo_of(np.float32, case, mutant="no_occlusion")
    assert b["photo_count"] != a["photo_count"] and b["count"] == a["count"]
    assert not np.array_equal(np.isnan(a["resid_photo"]), np.isnan(b["resid_photo"]))


@pytest.mark.parametrize("mutant", ["az_sign", "swap_g", "no_weight_g"])
def test_mutants_of_the_jacobian_and_the_weight_leave_the_sum_bound(mutant):
    """Both residual maps and both counts are the same; the sums are not: outside gamma_{n-1} S|t| on at least one of the 28."""
    case, a, _ = _case(48, 64, 1)
    b = pr.terms_photo_of(np.float32, case, mutant=mutant)
    assert np.array_equal(a["resid_photo"].view(np.int32), b["resid_photo"].view(np.int32)) and a["photo_count"] == b["photo_count"]
    assert (np.abs(b["sums"] - a["sums"]) > ir.sum_bound(a["abs_sums"], a["count"] + a["photo_count"])).any()


@pytest.mark.parametrize("mutant", ["swap_g"])
def test_a_mutant_of_the_gradient_does_not_track_the_plane(mutant):
    """The track gate catches it too: on the textured plane the mutant's schedule ends outside the tenth of the start's error the
    true one reaches."""
    field, color, truth, guess, depth, image, s, g = _plane()
    C = ir.CORNER
    m = pr.schedule_photo(np.float64, field, color, C["origin"], C["vs"], depth, image, None, guess, C["K"], dist_thr=C["dist_thr"],
                          huber=C["huber"], mutant=mutant)
    t0, r0 = ir.pose_error(guess, truth)
    t1, r1 = ir.pose_error(m["extM"], truth)
    assert m["flag"] != 0 or 10 * t1 > t0 or 10 * r1 > r0


def test_the_order_of_additions_stays_inside_the_bound():
    case, a, _ = _case(48, 64, 1)
    parts = np.array_split(a["terms"], 12)
    S = ir.add_records([p.sum(0) for p in parts])
    assert (np.abs(S - a["sums"]) <= ir.sum_bound(a["abs_sums"], a["count"] + a["photo_count"])).all()


# ---- 4. the textured plane: what geometry cannot see, texture pins
@functools.lru_cache(maxsize=None)
def _plane():
    C = ir.CORNER
    field, color, truth, guess = pr.plane_fixture()
    depth, image = pr.host_frame(field, color, truth)
    assert (depth > 0).all()
    s = pr.schedule_photo(np.float64, field, color, C["origin"], C["vs"], depth, image, None, guess, C["K"], dist_thr=C["dist_thr"],
                          huber=C["huber"])
    g = ir.schedule(np.float64, field, C["origin"], C["vs"], depth, guess, C["K"], dist_thr=C["dist_thr"], huber=C["huber"])
    return field, color, truth, guess, depth, image, s, g


def test_the_textured_plane_is_degenerate_without_and_converges_with_the_photometric_term():
    """float64, default levels, photo_weight = photo_huber = 0.1.  Measured: the geometric schedule flags DEGENERATE at its first step;
    the combined one goes from 5.22e-2 m / 2.06e-2 rad to 6.22e-5 m / 1.54e-5 rad, smallest relative pivot 1.64e-2 (min_pivot 1e-6),
    2920 photometric pairs for 2966 geometric ones at the finest level: more than a factor ten on every condition below."""
    field, color, truth, guess, depth, image, s, g = _plane()
    assert g["flag"] == ir.DEGENERATE and g["log"][0, 3] == ir.DEGENERATE
    t0, r0 = ir.pose_error(guess, truth)
    t1, r1 = ir.pose_error(s["extM"], truth)
    print("[icp photo] plane: %.3g m / %.3g rad -> %.3g m / %.3g rad, relative pivot %.3g, pairs %d photometric / %d geometric"
          % (t0, r0, t1, r1, s["rel_pivot"], s["photo_pairs"][-1], s["log"][-1, 0]))
    assert s["flag"] == 0 and 10 * t1 < t0 and 10 * r1 < r0
    assert s["rel_pivot"] > 100 * 1e-6
    assert s["photo_pairs"][-1] >= 0.9 * s["log"][-1, 0]


# ---- 5. the C entry
def test_the_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "nrgbd_icp_terms_photo_f32"
    decl = re.search(r"\bint %s\((.*?)\);" % name, code, flags=re.S).group(1)
    assert decl.count(",") + 1 == len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES["nrgbd_icp_terms_f32"][1]) + 7
    old = re.search(r"\bint nrgbd_icp_terms_f32\((.*?)\);", code, flags=re.S).group(1)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(decl).startswith(norm(old)[:-len(", void* stream")])      # the old entry's arguments come first, in its order
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert re.search(r"%s — no counterpart in the reference" % name, header)
    assert name in header[:header.index("#define NRGBD_INTERFACE_VERSION")]
    assert header.count('#define NRGBD_INTERFACE_VERSION "0.10"') == 1


P = ctypes.c_void_p(4096)                   # a non-NULL, aligned address: every refusal comes before anything touches the device
ODD = ctypes.c_void_p(4100)


def _floats(*v):
    return (ctypes.c_float * 3)(*v)


def test_the_entry_refuses_bad_arguments_without_a_gpu():
    fn = _lib.load().nrgbd_icp_terms_photo_f32
    A1, B0 = _floats(1, 1, 1), _floats(0, 0, 0)

    def call(null=None, H=48, W=64, sub=2, Hm=24, Wm=32, fx=60., fy=60., cx=32., cy=24., fxm=30., fym=30., cxm=16., cym=12., d_near=0.,
             d_far=INF, dist_thr=.3, huber=.05, gate=P, gate_thr=0., state=P, partial=P, nbytes=240 * 3, resid=P, aff_a=A1, aff_b=B0,
             pw=.1, ph=.1, resid_photo=P):
        # depth, mdepth, mnormal, state, partial, image, mrgb, aff_a, aff_b
        ptr = [None if i == null else p for i, p in enumerate((P, P, P, state, partial, P, P, aff_a, aff_b))]
        return fn(ptr[0], gate, gate_thr, H, W, d_near, d_far, fx, fy, cx, cy, sub, ptr[1], ptr[2], Hm, Wm, fxm, fym, cxm, cym, ptr[3],
                  dist_thr, huber, ptr[4], nbytes, resid, ptr[5], ptr[7], ptr[8], ptr[6], pw, ph, resid_photo, None)
    for i in range(9):
        assert call(null=i) == E_NULL, i
    for kw in (dict(H=0), dict(W=-1), dict(Hm=0), dict(Wm=0), dict(sub=0), dict(sub=49), dict(H=32769), dict(nbytes=240 * 3 - 1)):
        assert call(**kw) == E_SHAPE, kw
    for kw in (dict(fx=0.), dict(fym=NAN), dict(cx=NAN), dict(cym=INF), dict(dist_thr=0.), dict(huber=NAN), dict(d_near=1., d_far=1.),
               dict(gate_thr=NAN), dict(pw=0.), dict(pw=-1.), dict(pw=NAN), dict(pw=INF), dict(ph=0.), dict(ph=-.1), dict(ph=NAN),
               dict(ph=INF), dict(aff_a=_floats(1, NAN, 1)), dict(aff_a=_floats(INF, 1, 1)), dict(aff_b=_floats(0, 0, NAN)),
               dict(aff_b=_floats(0, -INF, 0))):
        assert call(**kw) == E_ARG, kw
    assert call(state=ODD) == E_ALIGN and call(partial=ODD) == E_ALIGN
    # the order: NULL, shape, argument, alignment — the new arguments in their class
    assert call(null=5, H=0, pw=0., state=ODD) == E_NULL and call(null=7, H=0) == E_NULL
    assert call(H=0, pw=0., state=ODD) == E_SHAPE and call(nbytes=1, ph=0., partial=ODD) == E_SHAPE
    assert call(pw=0., state=ODD) == E_ARG and call(aff_b=_floats(NAN, 0, 0), partial=ODD) == E_ARG
    assert call(gate=None, gate_thr=NAN, resid=None, resid_photo=None, state=ODD) == E_ALIGN      # the three optional maps may be NULL


def test_the_python_layers_refuse_without_a_gpu():
    from neuralrgbd_amd import ops, tracking

    class Colourless:
        color, device = None, "cpu"
    with pytest.raises(ValueError, match="colour volume"):
        tracking.FrameTracker(Colourless(), (48, 64), (60., 60., 32., 24.), photo=True)
    assert callable(ops.icp_terms_photo)
