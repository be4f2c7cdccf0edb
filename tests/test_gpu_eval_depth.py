"""GPU: nrgbd_depth_eval / evaluate.DepthMetrics against the float64 comparator of tests/depth_eval_ref.py.

Gates.  Counts, headers and err_map are exact.  Every term has the same bits on both sides, so a sum of N terms differs from the
comparator's fsum by the order of its additions alone: |S_gpu - S_ref| <= gamma_{N-1} S|t|, gamma_k = k 2^-53 / (1 - k 2^-53).
The sums of t4 = l^2 and t5 = l get 2 U 2^-53 S|t| on top for the two logs, U = 2 max(U_dev, 1) + 1, where U_dev is the largest
distance of the device's double log from the host's long-double logl over the ratios of tools/probes/log_f64_ulp.hip, in ulps of the
result, measured once on an MI355X: the factor 2 is margin over one measurement on one chip, the + 1 numpy's own log.
"""
import numpy as np
import pytest
import torch

import depth_eval_ref as ref
from test_eval_host import CONFS, SMALL_N, case_seed, n_past_the_finaliser
from neuralrgbd_amd import evaluate, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U_DEV = 0.6011                                # tools/probes/log_f64_ulp.hip on an MI355X: 8,201 ratios, worst at q = 1.3457 (0.5000 ulp
                                              # within 1e-6 of 1; the host's own double log: 0.5005 ulp) — DESIGN.md row f9
U = 2 * max(U_DEV, 1.0) + 1
GUARD = 64                                    # guard words on either side of every buffer the kernels write
SENT_I64 = 0x5A5A5A5A5A5A5A5A
SENT_F32 = -12345.5


def _sizes():
    return SMALL_N + (64 * 96, n_past_the_finaliser())


_CASES = {}


def _case(n, J, seed=None):
    """Inputs and the comparator's record of one (n, J), computed once and shared by the tests (never modified)."""
    key = (n, J, seed)
    if key not in _CASES:
        conf = CONFS[J]
        d, m, g = ref.make_inputs(n, case_seed(n, J) if seed is None else seed, conf)
        _CASES[key] = (d, m, g, ref.evaluate(d, m, g, ref.log_thresholds(conf), ref.GT_RANGE))
    return _CASES[key]


def _dev(*arrays):
    return tuple(torch.from_numpy(a).to(DEV) for a in arrays)


class Guarded:
    """The buffers of one nrgbd_depth_eval call, each between GUARD sentinel words."""

    def __init__(self, n, J, with_total=True):
        self.J = J
        ws_words = ops.depth_eval_workspace(n, J) // 8
        self._i64 = {"ws": ws_words, "f_sums": 6 * J, "f_counts": 4 * J, "f_header": 4, "t_sums": 6 * J, "t_counts": 4 * J, "t_header": 4}
        self._bufs = {k: torch.full((w + 2 * GUARD,), SENT_I64, dtype=torch.int64, device=DEV) for k, w in self._i64.items()}
        self._err = torch.full((n + 2 * GUARD,), SENT_F32, dtype=torch.float32, device=DEV)
        inner = {k: b[GUARD:GUARD + self._i64[k]] for k, b in self._bufs.items()}
        self.workspace = inner["ws"]
        self.frame = (inner["f_sums"].view(torch.float64).view(J, 6), inner["f_counts"].view(J, 4), inner["f_header"])
        self.total = (inner["t_sums"].view(torch.float64).view(J, 6), inner["t_counts"].view(J, 4), inner["t_header"]) if with_total else None
        if with_total:
            for t in self.total:
                t.zero_()
        self.err_map = self._err[GUARD:GUARD + n]

    def intact(self):
        ok = all(bool((b[:GUARD] == SENT_I64).all()) and bool((b[GUARD + self._i64[k]:] == SENT_I64).all()) for k, b in self._bufs.items())
        return ok and bool((self._err[:GUARD] == SENT_F32).all()) and bool((self._err[GUARD + self.err_map.numel():] == SENT_F32).all())


def _check_record(got, want, n_counts=None, what=""):
    """got: (sums, counts, header) tensors; want: a comparator record.  Prints every figure before it asserts."""
    sums, counts, header = (t.cpu().numpy() for t in got)
    assert np.array_equal(counts, want["counts"]), what
    assert np.array_equal(header, want["header"]), what
    bound = ref.sum_bounds(want["abs_sums"], want["counts"][:, 0] if n_counts is None else n_counts, U)
    diff = np.abs(sums - want["sums"])
    with np.errstate(all="ignore"):
        print("[eval] %s worst |S_gpu - S_ref| / bound per term: %s" % (what, np.nanmax(np.where(bound > 0, diff / bound, 0.0), axis=0)))
    assert np.all(diff <= bound), "%s: %s over %s" % (what, diff, bound)


@pytest.mark.parametrize("J", [1, 8])
@pytest.mark.parametrize("n", _sizes())
def test_records_and_err_map_against_the_comparator(n, J):
    d, m, g, want = _case(n, J)
    dd, dm, dg = _dev(d, m, g)
    thr = ref.log_thresholds(CONFS[J])
    b = Guarded(n, J)
    ops.depth_eval(dd, dm, dg, thr, ref.GT_RANGE, b.workspace, b.frame, b.total, b.err_map)
    torch.cuda.synchronize()
    assert b.intact()
    _check_record(b.frame, want, what="n=%d J=%d frame" % (n, J))
    for f, t in zip(b.frame, b.total):                                       # zeroed totals + frame = frame, bit for bit
        assert torch.equal(f, t)
    assert np.array_equal(b.err_map.cpu().numpy().view(np.uint32), want["err_map"].view(np.uint32))
    # without totals (the three pointers NULL) and without err_map: the same frame record
    c = Guarded(n, J, with_total=False)
    ops.depth_eval(dd, dm, dg, thr, ref.GT_RANGE, c.workspace, c.frame, None, None)
    torch.cuda.synchronize()
    assert c.intact() and bool((c.err_map == SENT_F32).all())
    for f, f2 in zip(b.frame, c.frame):
        assert torch.equal(f, f2)


def test_err_map_at_holes_is_zero_whatever_the_depth():
    """Where g is not > 0 the kernel writes 0.f even for a depth that is not finite (numpy's NaN * 0 would be NaN there)."""
    g = np.array([0, 0, 0, 0, -1, np.nan, 2], np.float32)
    d = np.array([np.nan, np.inf, -np.inf, 3, 3, 3, np.nan], np.float32)
    m = np.zeros(7, np.float32)
    b = Guarded(7, 1)
    ops.depth_eval(*_dev(d, m, g), ref.log_thresholds((0.,)), (1e-3, np.inf), b.workspace, b.frame, b.total, b.err_map)
    e = b.err_map.cpu().numpy()
    assert np.array_equal(e[:6].view(np.uint32), np.zeros(6, np.uint32)) and np.isnan(e[6]) and b.intact()
    assert b.frame[2].tolist() == [1, 1, 1, 0] and b.frame[1].tolist() == [[0, 0, 0, 0]]


def _three_frames(n, J):
    return [_case(n, J, seed=7000 + 31 * i + J) for i in range(3)]


@pytest.mark.parametrize("J", [1, 8])
def test_totals_accumulate_and_are_bit_reproducible(J):
    n = 64 * 96
    frames = _three_frames(n, J)
    want = ref.add_records([f[3] for f in frames])
    evs = [evaluate.DepthMetrics(CONFS[J], ref.GT_RANGE, device=DEV) for _ in range(2)]
    for ev in evs:
        for d, m, g, w in frames:
            rec = ev.update(*_dev(d, m, g))
            assert rec is ev.frame
            _check_record(rec, w, what="J=%d frame" % J)
    _check_record(evs[0].total, want, what="J=%d total of three" % J)         # N = the sets' total pixel counts
    assert evs[0].total[2].tolist()[0] == 3
    for a, b in zip(evs[0].total + evs[0].frame, evs[1].total + evs[1].frame):
        assert torch.equal(a, b)                                             # two fresh evaluators: bit-identical records
    # result() = metrics_from_record of the comparator, the sums' gates carried through one division and one square root
    got, exp = evs[0].result(), evaluate.metrics_from_record(want["sums"], want["counts"], want["header"], CONFS[J])
    rel = ref.sum_bounds(want["abs_sums"], want["counts"][:, 0], U) / np.maximum(np.abs(want["abs_sums"]), 1e-300)
    for j, (a, b) in enumerate(zip(got, exp)):
        for k in ("n", "frames", "gt_valid", "conf_threshold", "delta1", "delta2", "delta3", "coverage", "bad"):
            assert a[k] == b[k], (j, k)
        eps = 2.0 ** -52                                                     # the division's and the root's own roundings
        for k, t in (("mae", 0), ("abs_rel", 1), ("sq_rel", 2), ("rmse", 3), ("rmse_log", 4)):
            assert abs(a[k] - b[k]) <= (rel[j, t] + 2 * eps) * abs(b[k]), (j, k, a[k], b[k])
        # sc_inv^2 = S4/n - (S5/n)^2: absolute error of the difference, then sqrt: |da| <= d(var) / (2 sc_inv)
        n_j = want["counts"][j, 0]
        s4, s5 = want["abs_sums"][j, 4] / n_j, want["abs_sums"][j, 5] / n_j
        dvar = (rel[j, 4] + 2 * eps) * s4 + 2 * (rel[j, 5] + 2 * eps) * s5 * s5 + 2 * eps * s4
        assert abs(a["sc_inv"] - b["sc_inv"]) <= dvar / (2 * b["sc_inv"]) + 2 * eps * b["sc_inv"], (j, a["sc_inv"], b["sc_inv"])
    evs[0].reset()
    torch.cuda.synchronize()
    assert all(not t.any() for t in evs[0].total)
    z = evs[0].result()
    assert z[0]["n"] == 0 and z[0]["coverage"] == 0 and np.isnan(z[0]["mae"])


def test_update_captured_into_a_graph_replays_bit_for_bit():
    n, J = 64 * 96, 8
    frames = _three_frames(n, J)
    eager = evaluate.DepthMetrics(CONFS[J], ref.GT_RANGE, device=DEV)
    eager_frames = []
    for d, m, g, _ in frames:
        eager.update(*_dev(d, m, g))
        eager_frames.append([t.clone() for t in eager.frame])
    ev = evaluate.DepthMetrics(CONFS[J], ref.GT_RANGE, device=DEV)
    sd, sm, sg = (torch.zeros(n, device=DEV) for _ in range(3))
    err = torch.empty(n, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ev.update(sd, sm, sg, err)                                           # warm-up: sizes the workspace
    torch.cuda.current_stream().wait_stream(side)
    ev.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                            # one update: two kernel nodes in a single chain
        ev.update(sd, sm, sg, err)
    ev.reset()
    for (d, m, g, w), ef in zip(frames, eager_frames):
        for dst, src in zip((sd, sm, sg), _dev(d, m, g)):
            dst.copy_(src)
        graph.replay()
        for a, b in zip(ev.frame, ef):
            assert torch.equal(a, b)
        assert np.array_equal(err.cpu().numpy().view(np.uint32), w["err_map"].view(np.uint32))
    for a, b in zip(ev.total, eager.total):
        assert torch.equal(a, b)
    assert ev.total[2].tolist()[0] == 3


def test_update_dpv_reads_planar_and_channels_last_volumes():
    D, H, W = 64, 16, 24
    rng = np.random.RandomState(77)
    vol = torch.log_softmax(torch.from_numpy((rng.randn(1, D, H, W) * 3).astype(np.float32)).to(DEV), dim=1).contiguous()
    rows = vol[0].permute(1, 2, 0).contiguous()                              # [H,W,D] memory
    view = rows.permute(2, 0, 1)[None]                                       # the R-Net's channels-last view of it
    assert ops.is_channels_last_view(view[0]) and not ops.is_channels_last_view(vol[0]) and torch.equal(view, vol)
    d_candi = np.linspace(.5, 8, D)
    depth, conf = ops.depth_regress(vol[0], torch.from_numpy(d_candi.astype(np.float32)).to(DEV))
    g = (rng.randint(512, 8193, (H, W)) / 1024.0).astype(np.float32)
    g[rng.rand(H, W) < .2] = 0
    gt = torch.from_numpy(g).to(DEV)
    conf_thr = (0., .05, .1)
    evs = [evaluate.DepthMetrics(conf_thr, ref.GT_RANGE, device=DEV) for _ in range(3)]
    errs = [torch.empty(H, W, device=DEV) for _ in range(3)]
    evs[0].update_dpv(vol, d_candi, gt[None], errs[0])
    evs[1].update_dpv(view, d_candi, gt, errs[1])
    evs[2].update(depth, conf, gt, errs[2])
    for ev, e in zip(evs[1:], errs[1:]):
        for a, b in zip(evs[0].frame + evs[0].total, ev.frame + ev.total):
            assert torch.equal(a, b)
        assert torch.equal(e, errs[0])
    want = ref.evaluate(depth.cpu().numpy(), conf.cpu().numpy(), g, ref.log_thresholds(conf_thr), ref.GT_RANGE)
    _check_record(evs[0].frame, want, what="update_dpv")
    assert want["counts"][:, 0].min() >= 16
    # an up-sampled volume (4 D planes) goes over misc.d_candi_up4(d_candi)
    from neuralrgbd_amd import misc
    vol4 = torch.log_softmax(torch.from_numpy((rng.randn(1, 4 * D, H, W) * 3).astype(np.float32)).to(DEV), dim=1).contiguous()
    d4, c4 = ops.depth_regress(vol4[0], torch.from_numpy(misc.d_candi_up4(d_candi).astype(np.float32)).to(DEV))
    a, b = evaluate.DepthMetrics(conf_thr, ref.GT_RANGE, device=DEV), evaluate.DepthMetrics(conf_thr, ref.GT_RANGE, device=DEV)
    a.update_dpv(vol4, d_candi, gt)
    b.update(d4, c4, gt)
    for x, y in zip(a.frame, b.frame):
        assert torch.equal(x, y)
    with pytest.raises(ValueError):
        a.update_dpv(vol4[:, :100], d_candi, gt)


def test_wrapper_refusals_on_the_device():
    from neuralrgbd_amd._lib import NrgbdError
    n, J = 256, 1
    d, m, g, _ = _case(n, J)
    dd, dm, dg = _dev(d, m, g)
    b = Guarded(n, J)
    thr = ref.log_thresholds((0.,))
    with pytest.raises(NrgbdError):
        ops.depth_eval(dd, dm, dg, np.array([-1.0], np.float32), ref.GT_RANGE, b.workspace, b.frame, b.total)
    with pytest.raises(NrgbdError):
        ops.depth_eval(dd, dm, dg, thr, (2.0, 1.0), b.workspace, b.frame, b.total)
    with pytest.raises(NrgbdError):
        ops.depth_eval(dd, dm, dg, thr, ref.GT_RANGE, b.workspace[:1], b.frame, b.total)
    with pytest.raises(ValueError):
        ops.depth_eval(dd, dm[:-1], dg, thr, ref.GT_RANGE, b.workspace, b.frame, b.total)
    with pytest.raises(NrgbdError):
        ops.depth_eval(dd.cpu(), dm, dg, thr, ref.GT_RANGE, b.workspace, b.frame, b.total)
    torch.cuda.synchronize()
    assert b.intact() and bool((b.frame[2] == SENT_I64).all())                # nothing was launched
