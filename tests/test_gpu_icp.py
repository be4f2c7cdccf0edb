"""GPU: nrgbd_icp_terms_f32 and nrgbd_icp_update against the restatement of tests/icp_ref.py.

Gates.  The residual map equals the fp32 restatement bit for bit, the quiet NaNs included; the pair count is exact.  Every term of
the 28 sums has the same bits on both sides (promoted fp32 values, double products that round once), so a sum of N terms differs from
the comparator's fsum by the order of its additions alone: |S_gpu - S_ref| <= gamma_{N-1} S|t|, gamma_k = k 2^-53 / (1 - k 2^-53)
— derived, not measured.  The update has no library function and one lane: state, fp32 copy and log row equal the float64
restatement bit for bit.  Every buffer a kernel is handed lies between sentinel words that must be intact afterwards."""
import numpy as np
import pytest
import torch

import icp_ref as ir
from neuralrgbd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                    # guard words on either side of every buffer
SENT = {torch.float32: -12345.5, torch.float64: -12345.5}


class Guarded:
    """Named device buffers, each between GUARD sentinel words: `add(name, array)` uploads a copy, `add(name, shape, dtype)`
    makes a sentinel-filled one."""

    def __init__(self):
        self._outer, self._inner = {}, {}

    def add(self, name, array=None, shape=None, dtype=torch.float32):
        if array is not None:
            src = torch.from_numpy(np.ascontiguousarray(array))
            shape, dtype = tuple(src.shape), src.dtype
        n = int(np.prod(shape))
        outer = torch.full((n + 2 * GUARD,), SENT[dtype], dtype=dtype, device=DEV)
        inner = outer[GUARD:GUARD + n].view(shape)
        if array is not None:
            inner.copy_(src)
        self._outer[name], self._inner[name] = outer, inner
        return inner

    def __getitem__(self, name):
        return self._inner[name]

    def intact(self):
        ok = True
        for name, outer in self._outer.items():
            n = self._inner[name].numel()
            ok = ok and bool((outer[:GUARD] == SENT[outer.dtype]).all()) and bool((outer[GUARD + n:] == SENT[outer.dtype]).all())
        return ok


_CASES = {}


def _case(H, W, sub):
    """Inputs and both restatement records of one size, computed once and shared (never modified)."""
    key = (H, W, sub)
    if key not in _CASES:
        case = ir.make_terms_case(H, W, sub)
        _CASES[key] = (case, ir.terms_of(np.float32, case))
    return _CASES[key]


def _run_terms(case, with_resid=True):
    H, W = case["depth"].shape
    sub = case["sub"]
    g = Guarded()
    for name in ("depth", "gate", "mdepth", "mnormal"):
        g.add(name, case[name])
    nwg = ops.icp_workgroups(H // sub, W // sub)
    g.add("state", shape=(ops.ICP_STATE_WORDS,), dtype=torch.float64)
    g.add("partial", shape=(nwg, ops.ICP_RECORD_WORDS), dtype=torch.float64)
    g.add("resid", shape=(H, W))
    ops.icp_update(g["state"], 0, init=case["T"])
    got = ops.icp_terms(g["depth"], case["K"], sub, g["mdepth"], g["mnormal"], case["Km"], g["state"], g["partial"], case["dist_thr"],
                        case["huber"], depth_range=case["depth_range"], gate=g["gate"], gate_thr=case["gate_thr"],
                        resid=g["resid"] if with_resid else None)
    torch.cuda.synchronize()
    assert got == nwg == ir.workgroups(H // sub, W // sub)
    assert g.intact(), "a guard word was overwritten"
    return g


@pytest.mark.parametrize("H,W,sub", ir.TERMS_SIZES)
def test_terms_against_the_restatement(H, W, sub):
    case, want = _case(H, W, sub)
    g = _run_terms(case)
    state = g["state"].cpu().numpy()
    assert np.array_equal(state.view(np.int64), ir.state_words(case["T"], case["T"].astype(np.float32), 0, 0).view(np.int64))
    resid = g["resid"].cpu().numpy()
    assert np.array_equal(np.isnan(resid), np.isnan(want["resid"])), "the set of accepted pixels differs"
    assert np.array_equal(resid.view(np.int32), want["resid"].view(np.int32)), "residual bits differ"
    rec = g["partial"].cpu().numpy()
    count = int(rec[:, 28].view(np.int64).sum())
    assert count == want["count"] and not rec[:, 29].any()
    S = ir.add_records(rec[:, :28])                                 # the records in index order: what nrgbd_icp_update forms
    bound = ir.sum_bound(want["abs_sums"], want["count"])
    diff = np.abs(S - want["sums"])
    with np.errstate(all="ignore"):
        print("[icp] %dx%d sub %d: %d pairs in %d records, worst |S_gpu - fsum| / bound %.3g (worst diff %.3g)"
              % (H, W, sub, count, len(rec), np.nanmax(np.where(bound > 0, diff / bound, 0.0)) if count else 0.0, diff.max()))
    assert (diff <= bound).all(), (diff, bound)
    # the same inputs give the same bits; without a residual map the records are the same
    again = _run_terms(case, with_resid=False)
    assert torch.equal(again["partial"].view(torch.int64), g["partial"].view(torch.int64))
    assert bool((again["resid"] == SENT[torch.float32]).all())      # not touched


def _update_buffers(nwg, rows=3):
    g = Guarded()
    g.add("state", shape=(ops.ICP_STATE_WORDS,), dtype=torch.float64)
    g.add("log", shape=(rows, 4), dtype=torch.float64)
    return g


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("nwg", [1, 7, 256])
def test_update_equals_the_float64_restatement_bit_for_bit(nwg):
    g = _update_buffers(nwg)
    T0 = ir.init_motion()
    ops.icp_update(g["state"], 0, init=T0)
    T, Tf, flag, its = T0[:3], T0[:3].astype(np.float32), 0, 0
    assert np.array_equal(_bits(g["state"].cpu().numpy()), _bits(ir.state_words(T, Tf, flag, its)))
    for step in (1, 2):                                             # two iterations: the second starts from the first's state
        recs, counts = ir.make_records(nwg, "ok", seed=step)
        g.add("partial%d" % step, ir.pack_records(recs, counts))
        ops.icp_update(g["state"], step, g["partial%d" % step], nwg, min_pairs=6, min_pivot=1e-6, log=g["log"])
        T, Tf, flag, its, row, _ = ir.update(ir.add_records(recs), int(counts.sum()), T, flag, its, 6, 1e-6)
        torch.cuda.synchronize()
        assert flag == 0 and its == step
        assert np.array_equal(_bits(g["state"].cpu().numpy()), _bits(ir.state_words(T, Tf, flag, its))), "state bits differ at step %d" % step
        assert np.array_equal(_bits(g["log"][step - 1].cpu().numpy()), _bits(row)), "log row %d differs" % step
    assert bool((g["log"][2] == SENT[torch.float64]).all())         # rows that were not reached are not written
    assert g.intact()


def test_update_default_init_is_the_identity():
    g = _update_buffers(1)
    ops.icp_update(g["state"], 0)
    eye = np.eye(4)[:3]
    assert np.array_equal(_bits(g["state"].cpu().numpy()), _bits(ir.state_words(eye, eye.astype(np.float32), 0, 0))) and g.intact()


@pytest.mark.parametrize("kind,want", [("few", ir.FEW), ("nan", ir.NONFINITE), ("plane", ir.DEGENERATE), ("large", ir.LARGE)])
def test_update_flags_keep_the_motion_and_are_sticky(kind, want):
    nwg = 7
    g = _update_buffers(nwg)
    T0 = ir.init_motion()
    ops.icp_update(g["state"], 0, init=T0)
    before = g["state"].cpu().numpy().copy()
    T, flag, its = T0[:3], 0, 0
    for step, k in ((1, kind), (2, "ok")):                          # the flagged step, then a well-posed one
        recs, counts = ir.make_records(nwg, k, seed=step)
        g.add("partial%d" % step, ir.pack_records(recs, counts))
        ops.icp_update(g["state"], step, g["partial%d" % step], nwg, min_pairs=6, min_pivot=1e-6, log=g["log"])
        T, Tf, flag, its, row, _ = ir.update(ir.add_records(recs), int(counts.sum()), T, flag, its, 6, 1e-6)
        state = g["state"].cpu().numpy()
        assert flag == want and its == 0
        assert np.array_equal(_bits(state[:18]), _bits(before[:18])), "the motion changed its bits at step %d" % step
        assert np.array_equal(_bits(state), _bits(ir.state_words(T, Tf, flag, its)))
        got_row = g["log"][step - 1].cpu().numpy()
        assert np.array_equal(_bits(got_row), _bits(row)) and got_row[3] == want and got_row[0] == counts.sum()
    assert g.intact()


def test_wrapper_refusals_on_the_device():
    from neuralrgbd_amd._lib import NrgbdError
    case, _ = _case(16, 16, 1)
    g = Guarded()
    for name in ("depth", "mdepth", "mnormal"):
        g.add(name, case[name])
    state = g.add("state", shape=(ops.ICP_STATE_WORDS,), dtype=torch.float64)
    partial = g.add("partial", shape=(ops.ICP_RECORD_WORDS,), dtype=torch.float64)
    ops.icp_update(state, 0)
    args = (g["depth"], case["K"], 1, g["mdepth"], g["mnormal"], case["Km"], state, partial)
    with pytest.raises(NrgbdError, match="code -4"):
        ops.icp_terms(*args, 0.0, 0.05)
    with pytest.raises(NrgbdError, match="code -2"):
        ops.icp_terms(*args[:7], partial[:10], 0.3, 0.05)
    with pytest.raises(ValueError, match="state"):
        ops.icp_terms(*args[:6], state[:5], partial, 0.3, 0.05)
    with pytest.raises(NrgbdError, match="code -4"):
        ops.icp_update(state, 1, partial, 1, min_pairs=5, log=torch.zeros(4, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    assert g.intact()
