"""The three generations of the fused plane-sweep cost volume (csrc/costvol.hip `gather`, csrc/costvol_lds.hip `lds`,
csrc/costvol_quad.hip `quad`) held element by element against the exact-position float64 comparator of tests/costvol_fwd_exact.py
at constructed edge poses: planes behind the source camera, a denominator of exactly 1e-10 on whole planes, positions exactly on
-1, 0, w - 1 and w, candidates in a non-monotonic order.  |cost - exact| <= bound on EVERY element (the bound is derived there from
the arithmetic, never from what a kernel gives); the log-probabilities against the exact cost and against the kernel's own cost;
cost + logp, logp alone and a second call give equal bits; the automatic choice is the quad kernel bit for bit.  Every output
buffer goes in filled with NaN through the C entry nrgbd_costvol_fwd_gen: an element a kernel does not write fails every check.
tests/test_costvol_fwd_host.py checks the comparator, the bound and the input families on the same matrix without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import costvol_fwd_exact as fx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RUNS = [(shape, family, dist, align, gen) for shape, family, dist, align in fx.matrix() for gen in dict(fx.SHAPES)[shape]]
_worst = {}
_uploaded = {}


def _id(r):
    shape, family, dist, align, gen = r
    return "%dx%dx%d-V%d-C%d-%s-%s-align%d-%s" % (shape + (family, dist, align, gen))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _upload(case):
    """The device inputs of a case, once: packed texels (reference, sources) and the geometry."""
    if case["key"] not in _uploaded:
        from neuralrgbd_amd import ops
        V = case["src"].shape[0]
        tex = ops.pack_nhwc(_dev(np.concatenate([case["src"], case["ref"][None]], 0)))
        _uploaded[case["key"]] = (tex[V].contiguous(), tex[:V].contiguous(), _dev(case["KR"]).reshape(V, 9), _dev(case["Kt"]),
                                  _dev(case["rays"]), _dev(case["d_candi"]))
        torch.cuda.synchronize()
    return _uploaded[case["key"]]


def _call(case, dist, align, gen, want_cost=True, want_logp=True):
    """One nrgbd_costvol_fwd_gen call into NaN-filled outputs -> (cost | None, logp | None) as numpy; raises NrgbdError on a refusal."""
    from neuralrgbd_amd import _lib, ops
    ref, src, KR, Kt, rays, dc = _upload(case)
    V, C, h, w = case["src"].shape
    D = len(case["d_candi"])
    cost = torch.full((D, h, w), float("nan"), device=DEV) if want_cost else None
    logp = torch.full((D, h, w), float("nan"), device=DEV) if want_logp else None
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    rc = _lib.load().nrgbd_costvol_fwd_gen(p(ref), p(src), p(KR), p(Kt), p(rays), p(dc), case["cx"], case["cy"], case["sigma"],
                                           ops.DIST[dist], int(bool(align)), p(cost), p(logp), V, C, src.shape[-1], D, h, w,
                                           ops.GENERATION[gen], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "nrgbd_costvol_fwd_gen")
    torch.cuda.synchronize()
    return (None if cost is None else cost.cpu().numpy()), (None if logp is None else logp.cpu().numpy())


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), ratio)


def _same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("shape,family,dist,align,gen", RUNS, ids=[_id(r) for r in RUNS])
def test_generation_vs_exact_cost(shape, family, dist, align, gen):
    case = fx.make_case(*shape, family)
    want, bound = fx.exact(case, dist, align)
    cost, lp = _call(case, dist, align, gen)
    name = "%-6s %-8s %s align=%d %dx%dx%d V%d C%d" % ((gen, family, dist, align) + shape)

    ratio, at, beyond = fx.worst_ratio(cost, want, bound)
    print("[parity] costvol_fwd %s: worst error / bound %.3f at (k, y, x) = %s, %d beyond, %d NaN"
          % (name, ratio, at, beyond, int(np.isnan(cost).sum())))
    _note(gen, ratio)

    lp_ratio, lp_at, lp_beyond = fx.worst_ratio(lp, fx.log_softmax64(-want), fx.logp_bound(bound))
    print("[parity] costvol_fwd %s: logp vs exact cost, worst error / tolerance %.3f at %s, %d beyond" % (name, lp_ratio, lp_at, lp_beyond))
    _note("logp vs the exact cost", lp_ratio)

    own_want, own_tol = fx.logp_self_bound(cost)
    own_ratio, own_at, own_beyond = fx.worst_ratio(lp, own_want, own_tol)
    print("[parity] costvol_fwd %s: logp vs its own cost, worst error / tolerance %.3f at %s, %d beyond" % (name, own_ratio, own_at, own_beyond))
    _note("logp vs the kernel's own cost", own_ratio)

    assert beyond == 0, "%s: cost, %d elements beyond the bound, worst %.3g at %s" % (name, beyond, ratio, at)
    assert lp_beyond == 0, "%s: logp vs the exact cost, %d beyond, worst %.3g at %s" % (name, lp_beyond, lp_ratio, lp_at)
    assert own_beyond == 0, "%s: logp vs the kernel's own cost, %d beyond, worst %.3g at %s" % (name, own_beyond, own_ratio, own_at)

    _, lp_only = _call(case, dist, align, gen, want_cost=False)
    assert _same_bits(lp_only, lp), name + ": logp alone differs in bits from logp with the cost"
    cost_only, _ = _call(case, dist, align, gen, want_logp=False)
    assert _same_bits(cost_only, cost), name + ": cost alone differs in bits from cost with logp"
    cost2, lp2 = _call(case, dist, align, gen)
    assert _same_bits(cost2, cost) and _same_bits(lp2, lp), name + ": two calls differ in bits"
    if gen == "quad":
        cost0, lp0 = _call(case, dist, align, "auto")
        assert _same_bits(cost0, cost) and _same_bits(lp0, lp), name + ": the automatic choice is not the quad kernel's bits"


@pytest.mark.parametrize("shape,gen", [(s, g) for s, gens in fx.UNSUPPORTED for g in gens])
def test_unsupported_generation_is_refused(shape, gen):
    """Cp / 4 = 6 has no instantiation of the staged generations: an explicit request is an error, never a substitution."""
    from neuralrgbd_amd import _lib
    case = fx.make_case(*shape, "small")
    with pytest.raises(_lib.NrgbdError):
        _call(case, "L2", False, gen)


def test_report_worst_fraction_of_the_bound():
    """Last in the file: the worst observed fraction of the bound per generation and of the two logp tolerances over the tests above."""
    for key in sorted(_worst):
        print("[parity] costvol_fwd %-30s worst error / bound over this file: %.3f" % (key, _worst[key]))
    assert all(v <= 1.0 for v in _worst.values())
