"""Host-side checks of the depth evaluation: the float64 comparator against hand arithmetic, metrics_from_record, the pairing of depth
frames with their ground truth, the refusals of the C entry (observable without a GPU), and that the inputs of the GPU tests
exercise what those tests claim."""
import ctypes
import math

import numpy as np
import pytest

import depth_eval_ref as ref
from neuralrgbd_amd import _lib, evaluate

LN2, LN125 = math.log(2.0), math.log(1.25)


def _hand_example():
    """6 pixels, every value exact in binary.  g = 2 with d = 2.5, 4, 1 (evaluated); a hole; g = 16 outside the range (1, 8); g = 2
    with d = 0 (bad).  Confidences 0.9, 0.3, 0.6 against the thresholds (0, 0.5): set 1 holds the first and the third pixel."""
    g = np.array([2, 2, 2, 0, 16, 2], np.float32)
    d = np.array([2.5, 4, 1, 3, 16, 0], np.float32)
    m = np.log(np.array([.9, .3, .6, .9, .9, .9])).astype(np.float32)
    return d, m, g


def test_comparator_against_hand_arithmetic():
    d, m, g = _hand_example()
    out = ref.evaluate(d, m, g, ref.log_thresholds((0., .5)), (1.0, 8.0))
    # pixel 0: e = .5, q = r = 1.25 (NOT < 1.25);  pixel 1: e = 2, q = r = 2;  pixel 2: e = -1, q = .5, r = 2
    want0 = [.5 + 2 + 1, .25 + 1 + .5, .125 + 2 + .5, .25 + 4 + 1, math.fsum([LN125 * LN125, LN2 * LN2, LN2 * LN2]), math.fsum([LN125, LN2, -LN2])]
    want1 = [.5 + 1, .25 + .5, .125 + .5, .25 + 1, math.fsum([LN125 * LN125, LN2 * LN2]), math.fsum([LN125, -LN2])]
    assert np.array_equal(out["sums"][:, :4], np.array([want0[:4], want1[:4]]))             # exact in binary
    assert np.allclose(out["sums"][:, 4:], np.array([want0[4:], want1[4:]]), rtol=0, atol=4 * 2.0 ** -53)    # numpy's log against libm's
    assert np.array_equal(out["counts"], np.array([[3, 0, 1, 1], [2, 0, 1, 1]]))
    assert np.array_equal(out["header"], np.array([1, 4, 1, 0]))
    assert np.array_equal(out["err_map"], np.array([.5, 2, 1, 0, 0, 2], np.float32))
    assert np.array_equal(out["abs_sums"][0, :4], out["sums"][0, :4]) and out["abs_sums"][0, 5] == pytest.approx(LN125 + 2 * LN2, rel=1e-15)


def test_metrics_from_record():
    d, m, g = _hand_example()
    out = ref.evaluate(d, m, g, ref.log_thresholds((0., .5)), (1.0, 8.0))
    r0, r1 = evaluate.metrics_from_record(out["sums"], out["counts"], out["header"], (0., .5))
    assert r0["n"] == 3 and r0["frames"] == 1 and r0["gt_valid"] == 4 and r0["conf_threshold"] == 0. and r1["conf_threshold"] == .5
    assert r0["mae"] == 3.5 / 3 and r0["abs_rel"] == 1.75 / 3 and r0["sq_rel"] == 2.625 / 3 and r0["rmse"] == math.sqrt(5.25 / 3)
    t4, t5 = out["sums"][0, 4] / 3, out["sums"][0, 5] / 3
    assert r0["rmse_log"] == math.sqrt(t4) and r0["sc_inv"] == math.sqrt(t4 - t5 * t5)
    assert (r0["delta1"], r0["delta2"], r0["delta3"]) == (0.0, 1 / 3, 1 / 3)
    assert r0["coverage"] == .75 and r0["bad"] == .25 and r1["coverage"] == .5 and r1["mae"] == .75
    # an empty set, and an empty record: NaN metrics, coverage 0, no exception, no warning
    with np.errstate(all="raise"):
        e0, e1 = evaluate.metrics_from_record(np.zeros((2, 6)), np.array([[5, 1, 2, 3], [0, 0, 0, 0]]), np.array([1, 10, 0, 0]))
        z, = evaluate.metrics_from_record(np.zeros((1, 6)), np.zeros((1, 4), np.int64), np.zeros(4, np.int64))
    assert e0["mae"] == 0 and e0["coverage"] == .5 and e1["coverage"] == 0 and z["coverage"] == 0
    assert all(math.isnan(e1[k]) and math.isnan(z[k]) for k in evaluate.METRICS)
    # sc_inv clamps a negative rounding residue
    c, = evaluate.metrics_from_record(np.array([[0, 0, 0, 0, 1.0, 1.0 + 2.0 ** -52]]), np.array([[1, 1, 1, 1]]), np.array([1, 1, 0, 0]))
    assert c["sc_inv"] == 0.0


def test_log_thresholds():
    thr = evaluate.log_thresholds((0., .5, .9))
    assert thr.dtype == np.float32 and thr[0] == -np.inf and np.array_equal(thr[1:], np.log(np.array([.5, .9])).astype(np.float32))
    for bad in ((.1,), (0., .5, .5), (0., .7, .6), (0., 1.0), (), tuple(np.linspace(0, .9, 9))):
        with pytest.raises(ValueError):
            evaluate.log_thresholds(bad)


# ---- the pairing ----------------------------------------------------------------------------------------------------------------

def _schedule(r, pipeline, n, nan_at):
    """What VideoDepthStream hands out per push (video.py: push / flush): the ref_index of the maps or None, then the flush."""
    R, out, have_bv, owed = 2 * r + 1, [], False, None
    for i in range(n):
        ref = None
        if i + 1 >= R:
            if any(k in nan_at for k in range(i - 2 * r, i + 1)):
                have_bv, owed = False, None
            else:
                ref, first, have_bv = i - r, not have_bv, True
                if pipeline and not first:
                    ref, owed = owed, ref
        out.append(ref)
    return out, owed


@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("pipeline", [False, True])
def test_every_depth_frame_meets_the_ground_truth_of_its_push(r, pipeline):
    n, nan_at, none_at = 6 * r + 12, {2 * r + 4}, {r + 1, 5 * r + 8}
    outs, last = _schedule(r, pipeline, n, nan_at)
    n_slots = 2 * r + 2
    assert [evaluate.gt_slot(i, n_slots) for i in range(n_slots + 1)] == list(range(n_slots)) + [0]
    ring = evaluate.GtRing(n_slots)
    content = [None] * n_slots                 # stands for the device maps: the push whose depth frame was last written into a slot
    read_at = {}
    for i, ref in enumerate(outs + [last]):
        if i < n:                              # EvalVideoStream.push: the ground truth of push i is stored before anything is read
            slot = ring.store(i, i not in none_at)
            if i not in none_at:
                content[slot] = i
        if ref is None:
            continue
        read_at[ref] = i
        slot = ring.lookup(ref)
        if ref in none_at:
            assert slot is None                # maps, but no update
        else:
            assert slot is not None and content[slot] == ref
    evaluated = sorted(read_at)
    assert evaluated == sorted(set(evaluated)) and len(evaluated) >= 3 * r
    assert not any(k in nan_at for c in evaluated for k in range(c - r, c + r + 1))           # no frame of an affected window
    assert any(c in none_at for c in evaluated) and (not pipeline or last is not None)
    for c, at in read_at.items():              # no slot is overwritten before it is read: the next writer of c's slot is push c + n_slots
        assert at < c + n_slots or at == n     # (at == n: the flush, after the last push)
        assert at - c in ((r, r + 1) if pipeline else (r,)) or at == n
    assert n - 1 - r + n_slots > n             # the flushed frame's slot outlives the sequence
    with pytest.raises(ValueError):
        evaluate.gt_slot(-1, n_slots)


# ---- the C entry without a GPU --------------------------------------------------------------------------------------------------

def _call(lib, n=8, J=2, thr=None, lo=0.5, hi=8.0, ws_bytes=None, nulls=(), totals=(1, 1, 1), ws_offset=0):
    """nrgbd_depth_eval with host memory standing in for device memory: every refusal comes before the first launch."""
    thr = np.array([-np.inf, -1.0, -.5, -.25, -.2, -.1, -.05, -.01][:max(J, 1)], np.float32) if thr is None else np.asarray(thr, np.float32)
    bufs = {k: np.zeros(4096, np.float64) for k in ("depth", "logconf", "gt", "ws", "fs", "fc", "fh", "ts", "tc", "th")}
    p = {k: ctypes.c_void_p(None if k in nulls else v.ctypes.data) for k, v in bufs.items()}
    for k, give in zip(("ts", "tc", "th"), totals):
        if not give:
            p[k] = ctypes.c_void_p(None)
    if ws_bytes is None:
        ws_bytes = bufs["ws"].nbytes - 8
    if ws_offset:
        p["ws"] = ctypes.c_void_p(bufs["ws"].ctypes.data + ws_offset)
    return lib.nrgbd_depth_eval(p["depth"], p["logconf"], p["gt"], n, lo, hi, ctypes.c_void_p(None if "thr" in nulls else thr.ctypes.data), J,
                                p["ws"], ws_bytes, p["fs"], p["fc"], p["fh"], p["ts"], p["tc"], p["th"], None, None)


def test_c_entry_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    E_NULL, E_SHAPE, E_ARG = -1, -2, -4
    for name in ("depth", "logconf", "gt", "thr", "ws", "fs", "fc", "fh"):
        assert _call(lib, nulls=(name,)) == E_NULL, name
    assert _call(lib, n=0) == E_SHAPE and _call(lib, n=-5) == E_SHAPE
    assert _call(lib, J=0) == E_SHAPE and _call(lib, J=_lib.DEPTH_EVAL_MAX_SETS + 1, thr=np.full(9, -np.inf)) == E_SHAPE
    assert _call(lib, thr=[-1.0, -.5]) == E_ARG                     # log_thr[0] != -inf
    assert _call(lib, thr=[np.nan, -.5]) == E_ARG and _call(lib, thr=[-np.inf, np.nan]) == E_ARG
    assert _call(lib, J=3, thr=[-np.inf, -.5, -1.0]) == E_ARG       # not ascending
    assert _call(lib, lo=2.0, hi=1.0) == E_ARG and _call(lib, lo=np.nan) == E_ARG and _call(lib, hi=np.nan) == E_ARG
    need = lib.nrgbd_depth_eval_workspace(8, 2)
    assert need == (10 * 2 + 2) * 8 * lib.nrgbd_depth_eval_workgroups(8)
    assert _call(lib, ws_bytes=need - 1) == E_SHAPE
    assert _call(lib, ws_offset=4) == -3                              # NRGBD_E_ALIGN: the workspace holds 8-byte words
    for totals in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        assert _call(lib, totals=totals) == E_NULL, totals
    assert lib.nrgbd_depth_eval_workgroups(0) < 0 and lib.nrgbd_depth_eval_workgroups(-1) < 0
    assert lib.nrgbd_depth_eval_workspace(0, 1) < 0 and lib.nrgbd_depth_eval_workspace(8, 0) < 0 and lib.nrgbd_depth_eval_workspace(8, 9) < 0
    assert _lib.DEPTH_EVAL_MAX_SETS == 8


def test_workgroups_and_workspace_are_monotone():
    lib = _lib.load()
    ns = [1, 2, 255, 256, 257, 1023, 1024, 1025, 64 * 96, 256 * 384, 768 * 1024, 10 ** 7, 2 ** 31 + 5, 2 ** 40]
    wg = [lib.nrgbd_depth_eval_workgroups(n) for n in ns]
    assert wg[0] == 1 and all(a <= b for a, b in zip(wg, wg[1:])) and wg[-1] > 256
    for J in range(1, 9):
        ws = [lib.nrgbd_depth_eval_workspace(n, J) for n in ns]
        assert ws[0] > 0 and all(a <= b for a, b in zip(ws, ws[1:]))
    for n in ns:
        ws = [lib.nrgbd_depth_eval_workspace(n, J) for J in range(1, 9)]
        assert all(a < b for a, b in zip(ws, ws[1:]))


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------

def n_past_the_finaliser():
    """The smallest n whose first launch writes more partial records than the finaliser has lanes (256), from the query."""
    lib = _lib.load()
    lo, hi = 1, 1
    while lib.nrgbd_depth_eval_workgroups(hi) <= 256:
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lib.nrgbd_depth_eval_workgroups(mid) <= 256 else (lo, mid)
    return hi


SMALL_N = (1, 255, 256, 257)
CONFS = {1: (0.,), 8: ref.CONF_8}


def case_seed(n, J):
    """Seeds for which test_inputs_of_the_gpu_tests_are_not_vacuous holds (n = 1: the one pixel is evaluated, with d != g)."""
    if n == 1:
        return {1: 4014, 8: 4088}[J]
    return 4000 + 10 * J + (n % 97)


@pytest.mark.parametrize("J", [1, 8])
def test_inputs_of_the_gpu_tests_are_not_vacuous(J):
    big = n_past_the_finaliser()
    assert _lib.load().nrgbd_depth_eval_workgroups(big) == 257 and _lib.load().nrgbd_depth_eval_workgroups(big - 1) == 256
    conf = CONFS[J]
    thr = ref.log_thresholds(conf)
    for n in (64 * 96, big):
        d, m, g = ref.make_inputs(n, case_seed(n, J), conf)
        out = ref.evaluate(d, m, g, thr, ref.GT_RANGE)
        assert out["counts"][:, 0].min() >= 16                                              # every confidence set
        c = out["counts"][0]
        assert c[1] > 0 and c[2] > c[1] and c[3] > c[2] and c[0] > c[3]                      # every delta class and the one beyond
        assert (g == 0).any() and ((g > 0) & (g < ref.GT_RANGE[0])).any() and (g > ref.GT_RANGE[1]).any() and out["header"][2] > 0
        ok = (g >= ref.GT_RANGE[0]) & (g <= ref.GT_RANGE[1]) & (d > 0) & np.isfinite(d) & ~np.isnan(m)
        for f in ref.RATIOS[1:]:                                                            # the exact boundary ratios, evaluated
            assert (ok & (d.astype(np.float64) / np.where(g > 0, g, 1).astype(np.float64) == f)).sum() >= 16
        for t in thr[1:]:
            assert (ok & (m == t)).sum() >= 4                                               # pixels exactly on every threshold
        assert (ok & (m == -np.inf)).any() and np.isnan(m).any() and np.isnan(d).any() and np.isinf(d).any() and (d == 0).any() and (d < 0).any()
    for n in SMALL_N:                                                                       # the small sizes evaluate something too
        d, m, g = ref.make_inputs(n, case_seed(n, J), conf)
        assert ref.evaluate(d, m, g, thr, ref.GT_RANGE)["counts"][0, 0] >= 1
