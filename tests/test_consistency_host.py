"""Host-side checks of the multi-view depth consistency filter (csrc/consistency.hip): the fp32 restatement of tests/consistency_ref.py
against its float64 yardstick on every pixel the yardstick can decide; what the filter does on the corner fixture (no seeded flying
pixel survives, the clean pixels do); the mutants each bit-for-bit gate of the GPU tests has to catch, with the fp32 restatement standing
in for the device; the C entry (declared, bound, exported, every refusal without a GPU and in the documented order).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import consistency_ref as cr
from conftest import ROOT
from neuralrgbd_amd import _lib

E_NULL, E_SHAPE, E_ARG = -1, -2, -4
NAN, INF = float("nan"), float("inf")
NAME = "nrgbd_depth_consistency_f32"


# ---- 1. fp32 against float64
def _decided_equal(a, b, what):
    und = b["undecided"]
    share = und.mean()
    print("[consistency] %s: undecided %.2f %% of %d pixels" % (what, 100 * share, und.size))
    assert share <= 0.02, "the fixture's poses are not generic: the yardstick cannot decide %.2f %% of the pixels" % (100 * share)
    assert np.array_equal(a["votes"][~und], b["votes"][~und]), what


def test_fp32_equals_float64_on_every_decided_pixel_of_the_corner_fixture():
    _decided_equal(cr.corner_votes(np.float32), cr.corner_votes(np.float64), "corner")
    clean = cr.corner_fixture()["clean"]
    _decided_equal(cr.corner_votes(np.float32, depth=clean), cr.corner_votes(np.float64, depth=clean), "corner, no outliers")


# ---- 2. what the filter does
def test_corner_fixture_no_flying_pixel_survives_and_the_clean_pixels_do():
    fx = cr.corner_fixture()
    v = cr.corner_votes(np.float32)["votes"]
    out, hit = fx["outlier"], fx["clean"] > 0
    assert hit.mean() > 0.9 and 100 < out.sum() < 250 and (fx["sources"] > 0).mean() > 0.9
    kept = {k: cr.filtered(fx["depth"], v, k) > 0 for k in (1, 2)}
    clean = hit & ~out
    share = {k: kept[k][clean].mean() for k in kept}
    print("[consistency] corner: %d injected outliers, %d kept at min_views = 2 (%d at 1); clean pixels kept %.1f %% at 2, %.1f %% at 1"
          % (out.sum(), kept[2][out].sum(), kept[1][out].sum(), 100 * share[2], 100 * share[1]))
    assert kept[2][out].sum() == 0
    assert share[2] >= 0.95
    assert share[1] >= 0.99
    assert np.array_equal(cr.filtered(fx["depth"], v, 2)[kept[2]], fx["clean"][kept[2]])     # what stays is the clean value
    assert (v[~hit] == -1).all() and v.max() <= 4
    # the condition of the GPU test on this fixture: with one confirming view the filter is exactly "the outliers zeroed by hand"
    assert np.array_equal(cr.filtered(fx["depth"], v, 1), np.where(out, np.float32(0), fx["depth"]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_frame_is_consistent_with_itself(dtype):
    """The identity onto its own map: q = p exactly, u = fx * xn + cx lands inside pixel x, ds = d: votes 1 on every valid pixel."""
    case = cr.make_case(48, 64, 0, True)
    got = cr.votes(dtype, case["depth"], case["K"], case["depth"][None], [0], np.eye(4)[None, :3], 1e-6, case["depth_range"], case["gate"],
                   case["gate_thr"], case["gate"][None])
    valid = cr.votes_of(np.float32, case)["votes"] == 0
    assert 0.5 < valid.mean() < 1 and np.array_equal(got["votes"], np.where(valid, 1, -1).astype(np.float32))
    assert np.array_equal(cr.filtered(case["depth"], got["votes"], 1), np.where(valid, case["depth"], 0).astype(np.float32))


@pytest.mark.parametrize("H,W", cr.SIZES[1:])
@pytest.mark.parametrize("gated", [False, True])
def test_seeded_inputs_reach_every_branch(H, W, gated):
    case = cr.make_case(H, W, 16, gated)
    v = cr.votes_of(np.float32, case)["votes"]
    print("[consistency] %dx%d gated %d: votes %s" % (H, W, gated, np.unique(v, return_counts=True)))
    assert (v == -1).any() and (v == 0).any() and (v > 2).any() and v.max() <= 14      # the two sources that see nothing never agree
    for s, why in ((1, "behind"), (2, "outside")):
        alone = cr.votes(np.float32, case["depth"], case["K"], case["src_depth"], case["src_slots"][s:s + 1], case["src_T"][s:s + 1],
                         case["rel_thr"], case["depth_range"], case["gate"], case["gate_thr"], case["src_gate"])["votes"]
        assert alone.max() == 0, why
    if gated:
        nogate = cr.votes(np.float32, case["depth"], case["K"], case["src_depth"], case["src_slots"], case["src_T"], case["rel_thr"],
                          case["depth_range"])["votes"]
        assert (nogate == -1).sum() < (v == -1).sum() and nogate.sum() > v.sum()
    if H * W > 1000:                                                # the fp32 and the float64 votes agree where the yardstick decides
        b = cr.votes_of(np.float64, case)
        assert b["undecided"].mean() < 0.25 and np.array_equal(v[~b["undecided"]], b["votes"][~b["undecided"]])


# ---- 3. the mutants: each changes the votes on at least one fixture (the fp32 restatement stands in for the device)
CATCHES = {"lt": "edge", "far_lt": "far", "round_u": "seeded", "no_qz": "look_away", "no_src_gate": "gate_plane", "rel_ds": "seeded",
           "no_slots": "permuted_slots"}


@pytest.mark.parametrize("mutant", cr.MUTANTS)
def test_every_mutant_changes_the_votes(mutant):
    assert sorted(CATCHES) == sorted(cr.MUTANTS)
    corner = not np.array_equal(cr.corner_votes(np.float32)["votes"], cr.corner_votes(np.float32, mutant)["votes"])
    case = cr.make_case(48, 64, 16, True) if CATCHES[mutant] == "seeded" else cr.SMALL_CASES[CATCHES[mutant]]()
    a, b = cr.votes_of(np.float32, case)["votes"], cr.votes_of(np.float32, case, mutant)["votes"]
    print("[consistency] mutant %s: corner fixture %s, %s case: %d votes differ"
          % (mutant, "caught" if corner else "blind", CATCHES[mutant], (a != b).sum()))
    assert (a != b).any()


def test_the_small_cases_are_what_they_claim():
    v = {k: cr.votes_of(np.float32, f())["votes"] for k, f in cr.SMALL_CASES.items()}
    assert (v["edge"] == 1).all() and (v["far"] == 1).all() and (v["look_away"] == 0).all() and (v["permuted_slots"] == 1).all()
    assert (v["gate_plane"][:, :4] == 1).all() and (v["gate_plane"][:, 4:] == 0).all()


# ---- 4. the C entry
def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint %s\((.*?)\);" % NAME, code, flags=re.S).group(1)
    assert decl.count(",") + 1 == len(_lib.SIGNATURES[NAME][1]) == 22
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert re.search(r"%s — no counterpart in the reference" % NAME, header)
    assert NAME in header[:header.index("#define NRGBD_INTERFACE_VERSION")]               # named in the list at the top
    assert header.count('#define NRGBD_INTERFACE_VERSION "0.10"') == 1                     # no entry changed or disappeared
    assert int(re.search(r"#define NRGBD_CONSISTENCY_MAX_SRC (\d+)", header).group(1)) == _lib.CONSISTENCY_MAX_SRC == cr.MAX_SRC == 16


P = ctypes.c_void_p(4096)                   # a non-NULL address: every refusal comes before anything touches the device


def test_refuses_bad_arguments_without_a_gpu():
    fn = _lib.load().nrgbd_depth_consistency_f32
    eye = np.eye(4, dtype=np.float32)[:3].reshape(-1)

    def call(depth=P, gate=P, gate_thr=0., H=48, W=64, d_near=0., d_far=INF, fx=60., fy=60., cx=32., cy=24., src_depth=P, src_gate=P,
             stride=48 * 64, slots=(1, 0), T=None, n_src=2, rel=.01, min_views=1, votes=P, out=P, no_slots=False, no_T=False):
        cs = None if no_slots else (ctypes.c_int * max(len(slots), 1))(*slots)
        t = np.ascontiguousarray(np.tile(eye, max(n_src, 1)) if T is None else np.asarray(T, np.float32))
        return fn(depth, gate, gate_thr, H, W, d_near, d_far, fx, fy, cx, cy, src_depth, src_gate, stride, cs,
                  None if no_T else ctypes.c_void_p(t.ctypes.data), n_src, rel, min_views, votes, out, None)
    for kw in (dict(depth=None), dict(votes=None, out=None), dict(src_depth=None), dict(no_slots=True), dict(no_T=True),
               dict(gate=None), dict(src_gate=None)):
        assert call(**kw) == E_NULL, kw
    for kw in (dict(H=0), dict(W=-1), dict(H=32769), dict(W=32769), dict(n_src=-1), dict(n_src=17), dict(stride=48 * 64 - 1), dict(stride=0),
               dict(slots=(0, -1)), dict(slots=(-3, 0)), dict(min_views=-1)):
        assert call(**kw) == E_SHAPE, kw
    def bad_T(i, v):
        t = np.tile(eye, 2)
        t[i] = v
        return t
    for kw in (dict(fx=0.), dict(fx=NAN), dict(fy=-1.), dict(fy=INF), dict(cx=NAN), dict(cy=INF), dict(cy=-INF), dict(rel=0.), dict(rel=-1.),
               dict(rel=NAN), dict(rel=INF), dict(d_near=1., d_far=1.), dict(d_near=2., d_far=1.), dict(d_near=NAN), dict(d_far=NAN),
               dict(gate_thr=NAN), dict(T=bad_T(3, NAN)), dict(T=bad_T(12, INF)), dict(T=bad_T(23, -INF))):
        assert call(**kw) == E_ARG, kw
    # the order: NULL, shape, argument
    assert call(depth=None, H=0, fx=0.) == E_NULL and call(H=0, fx=0.) == E_SHAPE and call(slots=(0, -1), rel=NAN) == E_SHAPE
    assert call(src_gate=None, n_src=17, T=bad_T(0, NAN)) == E_NULL and call(min_views=-1, T=bad_T(0, NAN)) == E_SHAPE
    # what is allowed is refused for the next reason only: no sources (their pointers, stride and gates are then unused), one output
    # alone, a NaN threshold without a gate
    none = dict(n_src=0, src_depth=None, src_gate=None, no_slots=True, no_T=True, stride=0)
    assert call(fx=0., **none) == E_ARG and call(fx=0., gate=None, **none) == E_ARG and call(fx=0., src_gate=None, n_src=0) == E_ARG
    assert call(fx=0., votes=None) == E_ARG and call(fx=0., out=None) == E_ARG and call(fx=0., out=P, depth=P) == E_ARG
    assert call(fx=0., gate=None, src_gate=None, gate_thr=NAN) == E_ARG and call(fx=0., n_src=16, slots=(0,) * 16, min_views=99) == E_ARG


def test_the_wrapper_checks_before_it_calls():
    """ops.depth_consistency needs CUDA tensors: a host tensor is refused by name, with no fallback."""
    import torch
    from neuralrgbd_amd import ops
    with pytest.raises(_lib.NrgbdError):
        ops.depth_consistency(torch.zeros(4, 6), (5., 5., 3., 2.), None, None, 0.01, 0)
    with pytest.raises(TypeError):
        ops.depth_consistency(np.zeros((4, 6), np.float32), (5., 5., 3., 2.), None, None, 0.01, 0)
