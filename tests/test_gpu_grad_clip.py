"""Global-norm gradient clipping on csrc/optim.hip: the multi-tensor norm, the coefficient, the Adam update with the scale folded
into its gradient read (FusedAdam(max_grad_norm=...)), the in-place form (optim.clip_grad_norm_), capture into a hipGraph and the
non-finite step — against float64 (tests/grad_clip_ref.py), against torch, and the three forms against each other bit for bit.

Shapes: tensors of 1, 63, 64, 255, 2047, 2048, 2049, 4097 and 70001 elements (below, at and above a 2,048-element chunk, several
chunks, more than one workgroup), 97 tensors (slabs of 48 + 48 + 1), per-tensor gradient scales 10^(i mod 7 - 3), parameters
without a gradient in some steps."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import grad_clip_ref as ref
from neuralrgbd_amd import _lib, optim
from neuralrgbd_amd.optim import FusedAdam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 63, 64, 255, 2047, 2048, 2049, 4097, 70001] + [17 + i for i in range(88)]
assert len(SIZES) == 97
HALF = len(SIZES) // 2
STEPS = 4
U = 2.0 ** -24
# Roundings on the longest path of one chunk's sum in sumsq_kernel (csrc/optim.hip), read off the code: `q = x * x` (1); a thread's
# `s = j == 0 ? q : s + q` over j = 0..7 (7 additions); wave_sum's xor-shuffle tree, offsets 32..1 (6 additions);
# `((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]` (3 additions): R = 17.  All terms are >= 0, so each partial is within (1 + U)^17 of its
# exact value; norm_finalize_kernel adds the partials in double (below 2^-40 here) and takes (float)sqrt: the square root halves the
# relative error, the conversion adds one rounding.  (R + 2) U bounds the total with room to spare.
R = 1 + 7 + 6 + 3
NORM_BOUND = (R + 2) * U


def _groups(ps):
    return [{"params": ps[:HALF]}, {"params": ps[HALF:], "weight_decay": 0.01, "lr": 3e-3, "maximize": True}]


@functools.lru_cache(maxsize=None)
def _data():
    """Initial parameters and STEPS + 2 steps of gradients (CPU fp32; None: no gradient in that step), made once."""
    g = torch.Generator().manual_seed(3)
    p0 = [torch.randn(n, generator=g) for n in SIZES]
    grads = []
    for it in range(STEPS + 2):
        grads.append([None if (i + it) % 5 == 0 else torch.randn(n, generator=g) * (10.0 ** ((i % 7) - 3)) for i, n in enumerate(SIZES)])
    norms = [ref.total_norm(gs) for gs in grads]
    return p0, grads, norms


def _params():
    return [p.clone().to(DEV).requires_grad_(True) for p in _data()[0]]


def _set_grads(ps, gs, fn=None):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else (g.to(DEV) if fn is None else fn(g.to(DEV)))


def _state(ps, opt):
    out = {}
    for i, p in enumerate(ps):
        out["p%d" % i] = p.detach().clone()
        st = opt.state.get(p, {})
        for k in ("exp_avg", "exp_avg_sq", "step"):
            if k in st:
                out["%s%d" % (k, i)] = st[k].detach().clone()
    return out


def _assert_same(tag, a, b):
    assert list(a) == list(b), tag
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, "%s: %d of %d tensors differ, first %s" % (tag, len(bad), len(a), bad[0])


def _bits(t):
    return int(np.float32(float(t)).view(np.uint32))


# ---- 1. the norm ------------------------------------------------------------------------------------------------------------------

def test_norm_against_float64_and_reproducible_across_calls_and_streams():
    """|last_grad_norm - norm64| <= (R + 2) 2^-24 norm64 with R = 17 (derived above from sumsq_kernel), for the free function and for
    the optimizer's record; the same bits from a second call, from another stream and after an unrelated launch."""
    _, grads, norms = _data()
    worst = 0.0
    for it in (0, 1):
        ps = _params()
        _set_grads(ps, grads[it])
        n1 = optim.grad_norm(ps)
        n2 = optim.grad_norm(ps)
        junk = torch.randn(300000, device=DEV).square_().sum()                 # an unrelated launch in between
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            n3 = optim.grad_norm(ps)
        side.synchronize()
        opt = FusedAdam(_groups(ps), lr=1e-3, max_grad_norm=math.inf)
        opt.step()
        n4 = opt.last_grad_norm
        torch.cuda.synchronize()
        assert n1.dim() == 0 and n1.is_cuda and bool(torch.isfinite(junk))
        assert _bits(n1) == _bits(n2) == _bits(n3) == _bits(n4)
        ratio = abs(float(n1) - norms[it]) / norms[it]
        worst = max(worst, ratio)
        print("[clip] step %d: norm %.9g vs float64 %.17g, |d| / norm = %.3e (bound %.3e)" % (it, float(n1), norms[it], ratio, NORM_BOUND))
        assert ratio <= NORM_BOUND
        assert float(opt.last_clip_coef) == 1.0 and float(opt.nonfinite_steps) == 0.0
        for p, g in zip(ps, grads[it]):                                         # grad_norm scales nothing
            assert g is None or torch.equal(p.grad.cpu(), g)
    print("[clip] worst |norm - norm64| / norm64 = %.3e = %.2f x 2^-24" % (worst, worst / U))
    # single tensors at the chunk boundaries, all ones: the norm is sqrt(n) to one rounding
    for n in (1, 2047, 2048, 2049, 70001):
        p = torch.zeros(n, device=DEV, requires_grad=True)
        p.grad = torch.ones(n, device=DEV)
        assert abs(float(optim.grad_norm([p])) - math.sqrt(n)) <= 2 * U * math.sqrt(n), n
    assert float(optim.grad_norm(p)) == float(optim.grad_norm([p]))             # a single tensor, as torch takes it


# ---- 2. the coefficient -----------------------------------------------------------------------------------------------------------

def test_coef_is_recomputable_bit_for_bit_from_the_published_norm():
    _, grads, norms = _data()
    ps = _params()
    _set_grads(ps, grads[0])
    opt = FusedAdam(_groups(ps), lr=1e-3)
    for m in (0.5 * norms[0], 0.999 * norms[0], 1e-3, 1.5 * norms[0], 1e9, math.inf):
        opt.step(max_grad_norm=m)
        norm, coef = np.float32(float(opt.last_grad_norm)), np.float32(float(opt.last_clip_coef))
        want = np.float32(min(1.0, m / (np.float64(norm) + 1e-6)))
        print("[clip] M = %-12.6g norm %.9g coef %.9g (recomputed %.9g)" % (m, norm, coef, want))
        assert coef.view(np.uint32) == want.view(np.uint32)
        assert (coef == np.float32(1.0)) == (float(norm) <= m) and (m < norms[0]) == (coef < 1.0)
    opt.max_grad_norm = float(np.float32(float(opt.last_grad_norm)))             # M = the norm itself: no clipping
    opt.step()
    assert float(opt.last_clip_coef) == 1.0
    # the free function publishes the same norm and scales by the same coefficient
    m = 0.5 * norms[0]
    before = [None if p.grad is None else p.grad.clone() for p in ps]
    got = optim.clip_grad_norm_(ps, m)
    assert _bits(got) == _bits(opt.last_grad_norm)
    coef = torch.tensor(np.float32(min(1.0, m / (np.float64(np.float32(float(got))) + 1e-6))), device=DEV)
    for p, b in zip(ps, before):
        assert b is None or torch.equal(p.grad, torch.mul(b, coef))


# ---- 3 / 4. fused = in place = pre-scaled; against torch and float64 --------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _twins():
    """Four steps from the same state: (a) FusedAdam(max_grad_norm=M); (b) optim.clip_grad_norm_ then plain FusedAdam; (c) plain
    FusedAdam on torch.mul(g, coef) with (a)'s published coef; (t) torch's clip_grad_norm_ + torch.optim.Adam; (r) float64."""
    p0, grads, norms = _data()
    m = 0.5 * min(norms[:STEPS])                  # every step clips
    kw = dict(lr=1e-3, betas=(.9, .999), eps=1e-8)
    pa, pb, pc, pt = _params(), _params(), _params(), _params()
    oa, ob, oc = FusedAdam(_groups(pa), max_grad_norm=m, **kw), FusedAdam(_groups(pb), **kw), FusedAdam(_groups(pc), **kw)
    ot = torch.optim.Adam(_groups(pt), **kw)
    rp = [p.double() for p in p0]
    rm, rv, rt = [torch.zeros_like(p) for p in rp], [torch.zeros_like(p) for p in rp], [0] * len(rp)
    log = []
    for it in range(STEPS):
        gs = grads[it]
        _set_grads(pa, gs); _set_grads(pb, gs); _set_grads(pt, gs)
        oa.step()
        coef = oa.last_clip_coef.clone()
        nb = optim.clip_grad_norm_(pb, m)
        ob.step()
        _set_grads(pc, gs, lambda g: torch.mul(g, coef))
        oc.step()
        ntorch = torch.nn.utils.clip_grad_norm_(pt, m)
        ot.step()
        c64 = ref.clip_coef(norms[it], m)
        for lo, hi, g_ in ((0, HALF, {}), (HALF, len(SIZES), dict(weight_decay=0.01, lr=3e-3, maximize=True))):
            steps = rt[lo:hi]                     # the norm is global: the coefficient of all tensors goes to both groups
            ref.clipped_adam_step(rp[lo:hi], gs[lo:hi], rm[lo:hi], rv[lo:hi], steps, m, coef=c64, **dict(kw, **g_))
            rt[lo:hi] = steps
        log.append((float(oa.last_grad_norm), float(coef), float(nb), float(ntorch), norms[it], c64))
        for p, g in zip(pa, gs):                  # the fused form leaves the gradients in memory as they were
            assert g is None or torch.equal(p.grad.cpu(), g)
    torch.cuda.synchronize()
    return dict(a=_state(pa, oa), b=_state(pb, ob), c=_state(pc, oc), t=(pt, ot), r=(rp, rm, rv, rt), log=log, m=m)


def test_fused_equals_in_place_equals_prescaled_bit_for_bit():
    tw = _twins()
    for it, (na, ca, nb, nt_, n64, c64) in enumerate(tw["log"]):
        print("[clip] step %d: norm %.9g coef %.9g | clip_grad_norm_ %.9g | torch %.9g | float64 %.12g %.12g" % (it, na, ca, nb, nt_, n64, c64))
        assert na == nb and ca < 1.0
    assert sum(1 for k in tw["a"] if k.startswith("step")) == len(SIZES)
    _assert_same("fused vs clip_grad_norm_ + plain step", tw["a"], tw["b"])
    _assert_same("fused vs plain step on torch.mul(g, coef)", tw["a"], tw["c"])
    for i in range(len(SIZES)):                   # parameters without a gradient in a step lag, as in torch
        assert float(tw["a"]["step%d" % i]) == STEPS - sum(1 for it in range(STEPS) if (i + it) % 5 == 0)


def test_max_norm_above_every_norm_equals_the_plain_step_bit_for_bit():
    _, grads, norms = _data()
    pa, pd = _params(), _params()
    oa, od = FusedAdam(_groups(pa), lr=1e-3, max_grad_norm=4.0 * max(norms)), FusedAdam(_groups(pd), lr=1e-3)
    assert od.max_grad_norm is None and od.skip_nonfinite is False
    for it in range(STEPS):
        _set_grads(pa, grads[it]); _set_grads(pd, grads[it])
        oa.step(); od.step()
        assert float(oa.last_clip_coef) == 1.0
    _assert_same("max_grad_norm above every norm vs no clipping", _state(pa, oa), _state(pd, od))
    assert od._clip_bufs is None                  # the plain step never touched the clipping path


def test_fused_clipped_step_against_torch_and_float64():
    """The gate of test_fused_adam_vs_torch_adam_and_under_a_hipgraph: parameters to 2e-6 of max(1, max|p|), second moments to 1e-6
    of their largest entry, step counts equal — against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the GPU and against
    the float64 comparator."""
    tw = _twins()
    pt, ot = tw["t"]
    rp, rm, rv, rt = tw["r"]
    worst = {"torch p": 0.0, "torch v": 0.0, "f64 p": 0.0, "f64 v": 0.0}
    for i in range(len(SIZES)):
        a, v = tw["a"]["p%d" % i].cpu().double(), tw["a"]["exp_avg_sq%d" % i].cpu().double()
        for tag, b, bv, steps in (("torch", pt[i].detach().cpu().double(), ot.state[pt[i]]["exp_avg_sq"].cpu().double(),
                                   int(ot.state[pt[i]]["step"].item())), ("f64", rp[i], rv[i], rt[i])):
            ep = (a - b).abs().max().item() / max(1.0, b.abs().max().item())
            ev = (v - bv).abs().max().item() / max(1e-30, bv.abs().max().item())
            worst[tag + " p"], worst[tag + " v"] = max(worst[tag + " p"], ep), max(worst[tag + " v"], ev)
            assert int(tw["a"]["step%d" % i].item()) == steps, (tag, i)
    print("[clip] fused clipped step, worst relative differences: %s (gates 2e-6 / 1e-6)" % worst)
    assert worst["torch p"] <= 2e-6 and worst["f64 p"] <= 2e-6
    assert worst["torch v"] <= 1e-6 and worst["f64 v"] <= 1e-6


# ---- 5. under a hipGraph ----------------------------------------------------------------------------------------------------------

def test_clipped_step_captured_into_a_hipgraph():
    _, grads, norms = _data()
    m = 0.5 * min(norms)
    pa, pb = _params(), _params()
    oa, ob = FusedAdam(_groups(pa), lr=1e-3, max_grad_norm=m), FusedAdam(_groups(pb), lr=1e-3, max_grad_norm=m)
    full = [[torch.randn(n, generator=torch.Generator().manual_seed(100 * k + i)) * (10.0 ** ((i % 7) - 3)) for i, n in enumerate(SIZES)]
            for k in range(3)]
    _set_grads(pa, full[0]); _set_grads(pb, full[0])
    oa.step(); ob.step()                          # one eager step: state, record and pointer tables exist
    static = [p.grad for p in pa]
    s_ = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s_):
        with torch.cuda.graph(graph, stream=s_):
            oa.step()
    seen = [_bits(oa.last_grad_norm)]
    for k in (1, 2):
        for sg, g in zip(static, full[k]):
            sg.copy_(g)
        graph.replay()
        oa.mark_updated()
        _set_grads(pb, full[k])
        ob.step()
        torch.cuda.synchronize()
        seen.append(_bits(oa.last_grad_norm))
        assert _bits(oa.last_grad_norm) == _bits(ob.last_grad_norm) and _bits(oa.last_clip_coef) == _bits(ob.last_clip_coef)
        assert float(oa.last_clip_coef) < 1.0
    assert len(set(seen)) == 3                    # the record is rewritten by every replay
    _assert_same("two replays vs two eager steps", _state(pa, oa), _state(pb, ob))
    assert float(oa.state[pa[0]]["step"]) == 3.0


# ---- 6. a non-finite gradient -----------------------------------------------------------------------------------------------------

NF_SIZES = [63, 2049, 1, 4097]


def _nf_setup(max_norm, skip):
    g = torch.Generator().manual_seed(9)
    p0 = [torch.randn(n, generator=g) for n in NF_SIZES]
    gs = [[torch.randn(n, generator=g) for n in NF_SIZES] for _ in range(4)]
    ps = [p.clone().to(DEV).requires_grad_(True) for p in p0]
    opt = FusedAdam([{"params": ps[:2]}, {"params": ps[2:], "weight_decay": 0.01}], lr=1e-2, max_grad_norm=max_norm, skip_nonfinite=skip)
    return ps, opt, gs


@pytest.mark.parametrize("where", ["last", "first"])
@pytest.mark.parametrize("max_norm", [1.0, None])
def test_skip_nonfinite_leaves_the_step_out(where, max_norm):
    """inf, then NaN, in the last element of the last tensor / in element 0 of the first: with skip_nonfinite=True nothing changes,
    the counter goes to 1, then 2, and the next finite step continues from the un-advanced step count — as on a twin that never saw
    the bad steps.  (Arithmetic only: nothing here faults the device.)"""
    ps, opt, gs = _nf_setup(max_norm, True)
    pt, twin, _ = _nf_setup(max_norm, True)
    ti, ei = (len(NF_SIZES) - 1, -1) if where == "last" else (0, 0)
    _set_grads(ps, gs[0]); _set_grads(pt, gs[0])
    opt.step(); twin.step()
    before = _state(ps, opt)
    for k, bad in enumerate((math.inf, math.nan)):
        g = [t.clone() for t in gs[1 + k]]
        g[ti][ei] = bad
        _set_grads(ps, g)
        opt.step()
        torch.cuda.synchronize()
        _assert_same("skipped step %d (%s)" % (k, bad), before, _state(ps, opt))
        assert float(opt.nonfinite_steps) == k + 1
        assert not math.isfinite(float(opt.last_grad_norm))
    _set_grads(ps, gs[3]); _set_grads(pt, gs[3])
    opt.step(); twin.step()
    torch.cuda.synchronize()
    _assert_same("finite step after two skipped ones vs a twin without them", _state(ps, opt), _state(pt, twin))
    assert float(opt.state[ps[0]]["step"]) == 2.0 and float(opt.nonfinite_steps) == 2.0 and float(twin.nonfinite_steps) == 0.0
    assert math.isfinite(float(opt.last_grad_norm))


@pytest.mark.parametrize("bad", [math.inf, math.nan])
def test_without_skip_a_nonfinite_gradient_goes_through_as_in_torch(bad):
    """The default (skip_nonfinite=False) is torch's arithmetic: an inf makes the norm inf and the coefficient 0, and inf * 0 = NaN
    reaches the parameter that held it; a NaN makes the coefficient NaN and every parameter NaN.  Pinned against torch itself."""
    ps, opt, gs = _nf_setup(1.0, False)
    pt = [p.detach().clone().requires_grad_(True) for p in ps]
    ot = torch.optim.Adam([{"params": pt[:2]}, {"params": pt[2:], "weight_decay": 0.01}], lr=1e-2)
    g = [t.clone() for t in gs[0]]
    g[-1][-1] = bad
    _set_grads(ps, g); _set_grads(pt, g)
    opt.step()
    torch.nn.utils.clip_grad_norm_(pt, 1.0)
    ot.step()
    torch.cuda.synchronize()
    n_bad = 0
    for a, b in zip(ps, pt):
        assert torch.equal(torch.isfinite(a), torch.isfinite(b))
        n_bad += int((~torch.isfinite(a)).sum())
    assert not bool(torch.isfinite(ps[-1][-1])) and n_bad == (1 if math.isinf(bad) else sum(NF_SIZES))
    assert float(opt.nonfinite_steps) == 1.0 and float(opt.last_clip_coef) != 1.0
    assert float(opt.state[ps[0]]["step"]) == 1.0                                # the step counted


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------

def test_c_abi_refusals_launch_nothing():
    lib = _lib.load()
    P, L = ctypes.c_void_p, ctypes.c_long
    g = [torch.ones(2049, device=DEV), torch.ones(5, device=DEV)]
    gp, n = (P * 2)(*[t.data_ptr() for t in g]), (L * 2)(2049, 5)
    need = lib.nrgbd_grad_norm_workspace(n, 2)
    assert need == 3 * 4
    ws = torch.full((need // 4,), -7.0, device=DEV)
    clip = torch.full((4,), -7.0, device=DEV)
    cnt = torch.zeros(1, device=DEV)
    st = P(torch.cuda.current_stream().cuda_stream)
    w, c, k = P(ws.data_ptr()), P(clip.data_ptr()), P(cnt.data_ptr())
    E_NULL, E_SHAPE, E_ARG = -1, -2, -4
    assert lib.nrgbd_grad_norm(gp, n, 2, 1.0, w, need - 4, c, k, st) == E_SHAPE                  # workspace too small
    for bad in (0.0, -1.0, math.nan):
        assert lib.nrgbd_grad_norm(gp, n, 2, bad, w, need, c, k, st) == E_SHAPE
    assert lib.nrgbd_grad_norm(None, n, 2, 1.0, w, need, c, k, st) == E_NULL
    assert lib.nrgbd_grad_norm(gp, None, 2, 1.0, w, need, c, k, st) == E_NULL
    assert lib.nrgbd_grad_norm(gp, n, 2, 1.0, None, need, c, k, st) == E_NULL
    assert lib.nrgbd_grad_norm(gp, n, 2, 1.0, w, need, None, k, st) == E_NULL
    assert lib.nrgbd_grad_norm((P * 2)(g[0].data_ptr(), None), n, 2, 1.0, w, need, c, k, st) == E_NULL
    assert lib.nrgbd_grad_norm(gp, (L * 2)(2049, 0), 2, 1.0, w, need, c, k, st) == E_SHAPE
    assert lib.nrgbd_scale_tensors(gp, n, 2, None, st) == E_NULL and lib.nrgbd_scale_tensors(None, n, 2, c, st) == E_NULL
    assert lib.nrgbd_scale_tensors((P * 2)(None, g[1].data_ptr()), n, 2, c, st) == E_NULL
    a = [(P * 2)(*[t.data_ptr() for t in g]) for _ in range(5)]
    assert lib.nrgbd_adam_step_clipped(a[0], a[1], a[2], a[3], a[4], n, 2, 1e-3, .9, .999, 1e-8, 0.0, 0, None, 0, st) == E_NULL
    assert lib.nrgbd_adam_step_clipped(a[0], a[1], a[2], a[3], a[4], n, 2, 1e-3, .9, .999, 1e-8, 0.0, 0, c, 2, st) == E_ARG
    torch.cuda.synchronize()
    assert bool((ws == -7).all()) and bool((clip == -7).all()) and float(cnt) == 0.0 and all(bool((t == 1).all()) for t in g)
    # and the accepted call: the nullable counter, max_norm = inf
    assert lib.nrgbd_grad_norm(gp, n, 2, math.inf, w, need, c, None, st) == 0
    torch.cuda.synchronize()
    assert clip.tolist() == [float(np.float32(math.sqrt(2054.0))), 1.0, 0.0, 0.0]
    with pytest.raises(_lib.NrgbdError):
        optim.clip_grad_norm_([torch.nn.Parameter(torch.ones(3, device=DEV))], 1.0, norm_type=1)
    two = torch.nn.Parameter(torch.ones(3, device=DEV, dtype=torch.float16))
    two.grad = torch.ones(3, device=DEV, dtype=torch.float16)
    with pytest.raises(_lib.NrgbdError):
        optim.clip_grad_norm_([two], 1.0)         # never a silent ATen route
