"""GPU: ops.depth_consistency (csrc/consistency.hip) against the fp32 restatement of tests/consistency_ref.py, bit for bit on votes and
on the filtered map: one pixel, partial tiles on both edges, more than one tile each way; no source, one, three (one behind the camera,
one out of sight) and the entry's sixteen, out of a stack of five maps through a reversed slot list with repeats; with and without
gates; NaN, +-inf, 0 and negative depths and NaN gates on both sides; either output alone, in place, twice, and replayed from a
captured graph.  The small cases of the host test's mutants run here as well."""
import functools

import numpy as np
import pytest
import torch

import consistency_ref as cr
from neuralrgbd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIN_VIEWS = {0: 0, 1: 1, 3: 1, 16: 3}


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)                  # a copy: the fixtures are read-only


def _bits(t):
    return t.cpu().numpy().view(np.int32)


@functools.lru_cache(maxsize=None)
def _want(H, W, n_src, gated):
    """(case, votes, filtered map) of the fp32 restatement, computed once per case."""
    case = cr.make_case(H, W, n_src, gated)
    v = cr.votes_of(np.float32, case)["votes"]
    return case, v, cr.filtered(case["depth"], v, MIN_VIEWS[n_src])


def _run(case, min_views, **kw):
    args = {k: _dev(case[k]) for k in ("depth", "gate", "src_depth", "src_gate") if k not in kw}
    args.update(kw)
    depth = args.pop("depth")
    return ops.depth_consistency(depth, case["K"], args.pop("src_depth"), case["src_T"], case["rel_thr"], min_views,
                                 depth_range=case["depth_range"], gate_thr=case["gate_thr"], src_slots=case["src_slots"], **args)


def _same(got, want, what):
    assert np.array_equal(_bits(got), want.view(np.int32)), "%s: %d of %d pixels differ" % (
        what, int((_bits(got) != want.view(np.int32)).sum()), want.size)


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("n_src", cr.N_SRC)
@pytest.mark.parametrize("H,W", cr.SIZES)
def test_votes_and_filtered_map_equal_the_restatement_bit_for_bit(H, W, n_src, gated):
    case, v, f = _want(H, W, n_src, gated)
    votes, out = _run(case, MIN_VIEWS[n_src])
    _same(votes, v, "votes")
    _same(out, f, "depth_out")
    if n_src:
        slots = case["src_slots"]
        assert slots[0] == cr.STACK - 1 and (n_src < 3 or (slots[-1] < slots[0] and len(set(slots)) < len(slots)))      # reversed, repeats


def test_non_finite_inputs_and_sources_that_see_nothing():
    """The seeded 48 x 64 case with three sources and gates, after the conditions on it: NaN, +inf, -inf, 0 and a negative depth in the
    reference and in the sources read, a NaN in both gates, source 1 behind the camera and source 2 out of sight — neither ever
    agrees, and every pixel the reference's own tests fail has -1 votes and a 0 in the filtered map."""
    case, v, f = _want(48, 64, 3, True)
    for a in (case["depth"], case["src_depth"][case["src_slots"][0]]):
        assert np.isnan(a).any() and (a == np.inf).any() and (a == -np.inf).any() and (a == 0).any() and (a < 0).any()
    assert np.isnan(case["gate"]).any() and np.isnan(case["src_gate"]).any()
    for s in (1, 2):
        alone = dict(case, src_slots=case["src_slots"][s:s + 1], src_T=case["src_T"][s:s + 1])
        votes, out = _run(alone, 1)
        assert np.array_equal(votes.cpu().numpy(), np.where(v >= 0, 0, -1).astype(np.float32)) and not out.any()
    votes, out = _run(case, 1)
    _same(votes, v, "votes")
    _same(out, f, "depth_out")
    d, g = case["depth"], case["gate"]
    with np.errstate(invalid="ignore"):
        bad = ~(np.isfinite(d) & (d > np.float32(0.1)) & (d <= np.float32(1.75)) & (g >= np.float32(case["gate_thr"])))
    assert bad.any() and (v[bad] == -1).all() and (v[~bad] >= 0).all() and (f[bad] == 0).all() and 0 < (f > 0).sum() < (~bad).sum()


@pytest.mark.parametrize("name", sorted(cr.SMALL_CASES))
def test_the_small_cases_of_the_mutants(name):
    """Exact equality at the agreement threshold and at d_far, a source that looks away where only `q_z > 0` refuses it (rel q_z
    underflows to -0), a source gate, a slot list that is no identity."""
    case = cr.SMALL_CASES[name]()
    v = cr.votes_of(np.float32, case)["votes"]
    votes, out = _run(case, 1)
    _same(votes, v, name)
    _same(out, cr.filtered(case["depth"], v, 1), name)


def test_either_output_alone_in_place_and_twice():
    case, v, f = _want(67, 130, 3, True)
    only_votes = _run(case, 1, depth_out=False)
    assert only_votes[1] is None
    _same(only_votes[0], v, "votes alone")
    only_out = _run(case, 1, votes=False)
    assert only_out[0] is None
    _same(only_out[1], f, "depth_out alone")
    with pytest.raises(ValueError):
        _run(case, 1, votes=False, depth_out=False)
    depth = _dev(case["depth"])
    given = torch.full_like(depth, 7.0)
    votes, out = _run(case, 1, depth=depth, votes=given, depth_out=depth)          # in place: a pixel reads its own value only
    assert votes is given and out is depth
    _same(votes, v, "votes, in place")
    _same(depth, f, "depth_out, in place")
    again = _run(case, 1)
    once = _run(case, 1)
    assert torch.equal(again[0].view(torch.int32), once[0].view(torch.int32)) and torch.equal(again[1].view(torch.int32), once[1].view(torch.int32))


def test_a_strided_stack_is_read_where_it_lies():
    """The history's layout seen through a view: maps further than H W apart."""
    case, v, f = _want(48, 64, 3, True)
    wide = [torch.full((cr.STACK, 50, 64), float("nan"), device=DEV) for _ in range(2)]
    wide[0][:, :48].copy_(_dev(case["src_depth"]))
    wide[1][:, :48].copy_(_dev(case["src_gate"]))
    votes, out = _run(case, 1, src_depth=wide[0][:, :48], src_gate=wide[1][:, :48])
    _same(votes, v, "votes")
    _same(out, f, "depth_out")


def test_captured_and_replayed():
    from neuralrgbd_amd.distributed import graph_capture_mode
    case, v, f = _want(48, 64, 16, True)
    args = {k: _dev(case[k]) for k in ("depth", "gate", "src_depth", "src_gate")}
    _run(case, 3, **args)                                           # once eagerly: the library is loaded
    votes, out = torch.zeros(48, 64, device=DEV), torch.zeros(48, 64, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=graph_capture_mode()):
        _run(case, 3, votes=votes, depth_out=out, **args)
    assert not votes.any() and not out.any()                        # a capture executes nothing
    g.replay()
    torch.cuda.synchronize()
    _same(votes, v, "votes, replayed")
    _same(out, f, "depth_out, replayed")
    args["depth"].copy_(args["src_depth"][4])                       # the transforms are baked in, the maps are read at replay
    g.replay()
    torch.cuda.synchronize()
    moved = dict(case, depth=case["src_depth"][4])
    v2 = cr.votes_of(np.float32, moved)["votes"]
    _same(votes, v2, "votes, replayed on another map")
    _same(out, cr.filtered(moved["depth"], v2, 3), "depth_out, replayed on another map")
    assert not np.array_equal(v, v2)
