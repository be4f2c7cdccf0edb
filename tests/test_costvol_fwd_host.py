"""The cost-volume forward's comparator, bound and input families (tests/costvol_fwd_exact.py) checked on the CPU at exactly the
(shape, family, dist, align) matrix tests/test_gpu_costvol_fwd.py runs: the fp32 oracle and a numpy fp32 evaluation fit the bound,
deliberately wrong rules do not (the inputs discriminate), and every family holds the population it is there for."""
import numpy as np
import pytest

import costvol_fwd_exact as fx
import warp_exact as wx

MATRIX = fx.matrix()
SHAPE_IDS = ["%dx%dx%d-V%d-C%d" % s for s, _ in fx.SHAPES]
# wrong rule -> the families that aim at it
SENSITIVE = {"reject_behind": ("behind", "on_plane"), "border_lt": ("border", "large", "behind"),
             "trunc": ("border", "large", "behind"), "shift": fx.FAMILIES}


def _id(p):
    shape, family, dist, align = p
    return "%dx%dx%d-V%d-C%d-%s-%s-align%d" % (shape + (family, dist, align))


def test_matrix_is_the_one_the_issue_sets():
    assert len(fx.SHAPES) == 7 and len(fx.FAMILIES) == 7 and len(MATRIX) == 7 * 2 * (7 + 3) and len(set(MATRIX)) == len(MATRIX)
    assert set(fx.FAMILIES) == {"small", "large", "behind", "zoom_far", "on_plane", "border", "scatter"}
    gens = dict(fx.SHAPES)
    assert gens[(24, 40, 40, 3, 67)] == ("quad", "lds") and gens[(24, 40, 12, 3, 65)] == ("quad",)
    assert gens[(20, 36, 8, 2, 7)] == ("lds", "gather") and gens[(20, 36, 8, 2, 21)] == ("gather",)
    assert all(gens[s] == ("quad", "lds", "gather") for s in ((17, 23, 9, 2, 64), (16, 32, 5, 4, 67), (24, 40, 12, 3, 67)))


@pytest.mark.parametrize("shape,family,dist,align", MATRIX, ids=[_id(p) for p in MATRIX])
def test_oracle_and_plain_fp32_fit_the_bound(shape, family, dist, align):
    case = fx.make_case(*shape, family)
    want, bound = fx.exact(case, dist, align)
    assert np.isfinite(want).all() and np.isfinite(bound).all() and (bound > 0).all()
    got = fx.oracle_cost(case, dist, align)
    assert np.isfinite(got).all()
    r_o, at, beyond = fx.worst_ratio(got, want, bound)
    assert beyond == 0, "oracle: %d beyond, worst %.3f at %s" % (beyond, r_o, at)
    r_p, at, beyond = fx.worst_ratio(fx.fp32_cost(case, dist, align, "plain"), want, bound)
    assert beyond == 0, "plain fp32: %d beyond, worst %.3f at %s" % (beyond, r_p, at)
    print("[parity] costvol_fwd host %-8s %s align=%d %s: oracle %.3f, numpy fp32 %.3f of the bound (largest bound %.1e, largest cost %.1f)"
          % (family, dist, align, shape, r_o, r_p, bound.max(), want.max()))
    # the log-probabilities of the oracle's own cost, through the tolerance the GPU test uses
    lp_want, lp_tol = fx.log_softmax64(-want), fx.logp_bound(bound)
    assert fx.worst_ratio(fx.log_softmax64(-got.astype(np.float64)), lp_want, lp_tol)[2] == 0


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("shape", [s for s, _ in fx.SHAPES], ids=SHAPE_IDS)
def test_wrong_rules_leave_the_bound(shape, align):
    """A condition on the INPUTS: each wrong rule has elements beyond the bound in the families that aim at it."""
    for variant, families in SENSITIVE.items():
        for family in families:
            case = fx.make_case(*shape, family)
            want, bound = fx.exact(case, "L2", align)
            ratio, at, beyond = fx.worst_ratio(fx.fp32_cost(case, "L2", align, variant), want, bound)
            print("[inputs] costvol_fwd %s align=%d %-13s in %-8s: worst error / bound %.3g, %d beyond" % (shape, align, variant, family, ratio, beyond))
            assert beyond > 0, (variant, family)


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("shape", [s for s, _ in fx.SHAPES], ids=SHAPE_IDS)
def test_families_hold_their_populations(shape, align):
    h, w, D, V, C = shape
    pops = {f: fx.population(fx.make_case(*shape, f), align) for f in ("behind", "large", "on_plane", "zoom_far", "border")}
    for f, p in pops.items():
        print("[inputs] costvol_fwd %s align=%d %-8s: %s" % (shape, align, f, {k: v for k, v in p.items() if not callable(v)}))
        assert p["samples"] == V * D * h * w
    n = V * D * h * w
    assert pops["behind"]["behind_in_image"] >= 0.05 * n
    assert pops["large"]["wholly_outside"] > 0.1 * n and pops["large"]["partly_outside"] > 0.005 * n
    assert pops["on_plane"]["planes_at_min_den"] == V
    assert pops["zoom_far"]["wholly_outside"] == 0 and pops["zoom_far"]["partly_outside"] == 0
    if (h, w) == wx.BORDER_POW2:
        b = pops["border"]
        if align:
            assert b["at_x"](0) > 0 and b["at_x"](w - 1) > 0 and b["at_y"](0) > 0 and b["at_y"](h - 1) > 0
        else:
            counts = [b["at_x"](val) for val in (-1, -0.5, 0, w - 1, w - 0.5, w)]
            print("[inputs] costvol_fwd border x positions on -1, -0.5, 0, w-1, w-0.5, w:", counts)
            assert all(c > 0 for c in counts)
            assert all(b["at_y"](val) > 0 for val in (-1, 0, h - 1, h))


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("shape,gens", fx.SHAPES, ids=SHAPE_IDS)
def test_cases_reach_the_branches_of_the_staged_generations(shape, gens, align):
    """A host restatement of the two footprint rules (fx.quad_branches, fx.lds_branches) says which branches the matrix reaches at
    this shape: a condition on the inputs and the launch rules, not on what a kernel returns."""
    h, w, D, V, C = shape
    if "quad" in gens:
        q = {f: fx.quad_branches(fx.make_case(*shape, f), align) for f in fx.FAMILIES}
        for f in fx.FAMILIES:
            print("[inputs] costvol_fwd %s align=%d quad %-8s: %s" % (shape, align, f, q[f]))
            assert q[f]["nchunk"] == (4 if D == 40 else 1) and q[f]["tiles"] == -(-h // 8) * -(-w // 8)
        z = q["zoom_far"]
        assert z["staged_interior"] > 0 and z["staged_apron"] == 0 and z["global_groups"] == 0 and z["bad_planes"] == 0
        assert z["longest_run"] == min(D, 10 if D == 40 else 32)                      # a whole chunk from one patch
        assert q["border"]["staged_apron"] > 0                                        # patches that hold the one-texel apron
        for f in ("behind", "on_plane"):
            assert q[f]["bad_planes"] > 0 and q[f]["global_groups"] > 0               # unbounded boxes: groups from global memory
        assert sum(q[f]["global_groups"] for f in fx.FAMILIES if q[f]["bad_planes"] == 0) > 0   # bounded footprints that do not fit as a pair
    if "lds" in gens:
        l = {f: fx.lds_branches(fx.make_case(*shape, f), align) for f in fx.FAMILIES}
        for f in fx.FAMILIES:
            print("[inputs] costvol_fwd %s align=%d lds  %-8s: %s" % (shape, align, f, l[f]))
            assert l[f]["nsingle"] == min(D, 8) and l[f]["groups"] == min(D, 8) + -(-max(D - 8, 0) // 8)
        assert l["zoom_far"]["gathered"] == 0 and l["zoom_far"]["nothing_in_view"] == 0 and l["zoom_far"]["staged_runs"].get(1, 0) > 0
        for f in ("behind", "on_plane"):
            assert l[f]["bad_planes"] > 0 and l[f]["gathered"] >= l[f]["bad_planes"]  # the direct-gather fallback
        assert l["large"]["nothing_in_view"] > 0                                      # the "nothing in view" return
        if D > 8:
            assert l["zoom_far"]["staged_runs"].get(min(8, D - 8), 0) > 0             # a whole group from one patch
        if D == 40:
            split = sum(l[f]["staged_runs"].get(n, 0) for f in fx.FAMILIES for n in (2, 4))
            overflow = sum(l[f]["gathered"] for f in fx.FAMILIES if l[f]["bad_planes"] == 0)
            assert split > 0 and overflow > 0        # the per-candidate split, and a footprint larger than the patch even alone


def test_logp_tolerances_are_what_the_docstring_derives():
    bound = np.array([[1e-3, 2e-3], [5e-3, 1e-6]])
    assert np.allclose(fx.logp_bound(bound), bound + np.array([[5e-3, 2e-3]]) + 1e-4, rtol=0, atol=1e-18)
    cost = np.array([[0.0, 3.0], [115.0, 1.0]], np.float32)
    want, tol = fx.logp_self_bound(cost)
    assert np.allclose(np.exp(want).sum(0), 1.0)
    assert abs(want[1, 0] + 115.0) < 1e-9 and abs(tol[1, 0] - (4 * fx.U * 230.0 + 5e-6)) < 1e-12
    nan = cost.copy()
    nan[0, 0] = np.nan
    assert fx.worst_ratio(nan, cost.astype(np.float64), np.ones_like(bound))[2] == 1      # a NaN is beyond every bound
