"""train(..., grad_clip_max=M) and TrainGraph(..., grad_clip_max=M): the reference's `--grad_clip --grad_clip_max M` on the training
call surface.  The window of tests/test_gpu_train_det.py: 256x256 images, D = 8, seeded state dict, deterministic=True, three
iterations (a first frame, then two updates), so that every comparison between two forms of the same arithmetic is bit for bit."""
import functools
import socket

import numpy as np
import pytest
import torch

import grad_clip_ref as ref
import neuralrgbd_amd
from neuralrgbd_amd import camera, optim, synth
from neuralrgbd_amd.optim import FusedAdam
from neuralrgbd_amd.test_step import test as infer
from neuralrgbd_amd.train_step import TrainGraph, train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, D = 256, 256, 8
CAM = camera.scannet_intrinsics(W // 4, H // 4)
D_CANDI = np.linspace(0.1, 5, D)
NORM_BOUND = (17 + 2) * 2.0 ** -24               # tests/test_gpu_grad_clip.py derives it from sumsq_kernel


def _model():
    m = neuralrgbd_amd.KVNET(64, CAM, D_CANDI, 10.0, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=2)
    m.load_state_dict(synth.seeded_state_dict(m, 0))
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _windows(n, seed):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        r, s, p = synth.noise_window(5000 + 10 * seed + i, H, W)
        out.append((r.to(DEV), s.to(DEV), p.to(DEV), torch.from_numpy(rng.randint(0, D, (1, H // 4, W // 4))).to(DEV),
                    torch.from_numpy(rng.randint(0, D, (1, H, W))).to(DEV)))
    return tuple(out)


def _train_call(model, opt, ws, preds, **kw):
    """One train() call on the len(ws) windows of an optimizer step (accum_steps = len(ws)); preds: None or one volume per window."""
    A = len(ws)
    bv = None if preds is None else (preds[0] if A == 1 else list(preds))
    out = train(1, model, opt, 2, D_CANDI, [{"img": w_[0], "dmap": w_[3], "dmap_imgsize_digit": w_[4]} for w_ in ws],
                [[{"img": w_[1][0, v:v + 1]} for v in range(4)] for w_ in ws], torch.cat([w_[2] for w_ in ws], 0), bv, [CAM],
                accum_steps=A, deterministic=True, **kw)
    return out, [t.clone() for t in out[1].split(1, 0)]


def _same(tag, a, b):
    assert list(a) == list(b), tag
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    print("[clip] %s: %d tensors compared, %d differ" % (tag, len(a), len(bad)))
    assert not bad, "%s: first differing tensor %s (%d differ)" % (tag, bad[0], len(bad))


def _state(model, opt):
    out = {"model." + k: v.detach().clone() for k, v in model.state_dict().items()}
    names = {p: n for n, p in model.named_parameters()}
    for p, st in opt.state.items():
        for key in ("exp_avg", "exp_avg_sq", "step"):
            out["adam.%s.%s" % (names[p], key)] = st[key].detach().clone()
    return out


def _first_preds(model, wins, A):
    with torch.no_grad():
        return [infer(model, D_CANDI, [CAM], 2, [{"img": w_[0]}], [[{"img": w_[1][0, v:v + 1]} for v in range(4)]], w_[2], None)[1].clone()
                for w_ in wins[:A]]


class _ClipThenStep(FusedAdam):
    """The twin's optimizer: optim.clip_grad_norm_ in place, then the plain fused step."""

    def __init__(self, params, m, **kw):
        super().__init__(params, **kw)
        self.m = m

    def step(self, closure=None):
        optim.clip_grad_norm_([p for group in self.param_groups for p in group["params"]], self.m)
        return super().step(closure)


@functools.lru_cache(maxsize=None)
def _max_norm(A):
    """Half the gradient norm of an unclipped first iteration (at this accum_steps: the norm of the averaged gradient)."""
    model = _model()
    _train_call(model, FusedAdam(model.parameters(), lr=1e-4), _windows(4 * A, A)[:A], None)
    return 0.5 * float(optim.grad_norm(model.parameters()))


@functools.lru_cache(maxsize=None)
def _eager_run(A, form, reducer=False, first_frame=True):
    """Three optimizer steps of A windows each: a first frame and two updates, or (first_frame=False) three updates after an
    inference pass over the first windows.  form: "fused" = train(grad_clip_max=M) on FusedAdam, "twin" = train() on _ClipThenStep,
    "off" = train(grad_clip_max=None, skip_nonfinite=False), "parent" = train() as before."""
    wins, m = _windows(4 * A, A), _max_norm(A)
    model = _model()
    opt = _ClipThenStep(model.parameters(), m, lr=1e-4) if form == "twin" else FusedAdam(model.parameters(), lr=1e-4)
    kw = {"fused": dict(grad_clip_max=m), "off": dict(grad_clip_max=None, skip_nonfinite=False)}.get(form, {})
    if reducer:
        from neuralrgbd_amd import distributed as nd
        kw["grad_reducer"] = nd.GradAllReduce(model, bucket_mb=2.0, always_collective=True)
    preds, trace, coefs, norms = None, {}, [], []
    if not first_frame:
        preds, wins = _first_preds(model, wins, A), wins[A:]
    for it in range(3):
        (_, pred, loss, lo, hi), preds = _train_call(model, opt, wins[A * it:A * (it + 1)], preds, **kw)
        trace["loss%d" % it], trace["pred%d" % it], trace["lo%d" % it], trace["hi%d" % it] = loss.clone(), pred.clone(), lo.clone(), hi.clone()
        if form == "fused":
            coefs.append(float(opt.last_clip_coef))
            norms.append((float(opt.last_grad_norm), ref.total_norm([p.grad for p in model.parameters()])))
    torch.cuda.synchronize()
    return trace, _state(model, opt), coefs, norms


@pytest.mark.parametrize("A", [1, 2])
def test_train_with_grad_clip_max_equals_clip_in_place_then_step(A):
    """train(grad_clip_max=M) on FusedAdam (scale folded into the update) against a twin whose optimizer scales the gradients in place
    with optim.clip_grad_norm_ and then steps: weights, BatchNorm statistics, moments, losses and predicted volumes bit for bit.  The
    fused form leaves the .grad tensors unscaled and A-averaged: their float64 norm is the norm the step published — clipping comes
    after the division by accum_steps."""
    t1, s1, coefs, norms = _eager_run(A, "fused")
    t2, s2, _, _ = _eager_run(A, "twin")
    print("[clip] accum %d: M = %.6g, coef per step %s, norm (published, float64 of .grad) %s" % (A, _max_norm(A), coefs, norms))
    assert sum(1 for c in coefs if c < 1.0) >= 2               # else the comparison shows nothing
    assert all(bool(torch.isfinite(t1["loss%d" % i])) for i in range(3))
    for got, want in norms:
        assert abs(got - want) <= NORM_BOUND * want
    _same("accum %d, losses and predictions" % A, t1, t2)
    _same("accum %d, weights, BN statistics, Adam moments" % A, s1, s2)
    off = _eager_run(A, "parent")[1]
    assert sum(1 for k in s1 if k.startswith("model.") and not torch.equal(s1[k], off[k])) > 200       # and clipping changed the run


def test_grad_clip_max_none_is_the_parent_behaviour():
    t1, s1, _, _ = _eager_run(1, "off")
    t2, s2, _, _ = _eager_run(1, "parent")
    _same("grad_clip_max=None vs no keyword, losses and predictions", t1, t2)
    _same("grad_clip_max=None vs no keyword, state", s1, s2)


def test_clipping_after_a_one_rank_rccl_all_reduce_equals_the_reducer_free_run():
    """GradAllReduce(always_collective=True) on a one-rank RCCL group: the clipped step reads the all-reduced bucket views; every rank
    of a larger group computes the norm from the same reduced buffers, so the decision needs no collective of its own.
    Three update iterations: everything is bit-identical to the reducer-free twin.  The sequence of the other tests (a first frame,
    then two updates) is bit-identical up to and including the second step's norm, coefficient, loss and prediction — and must part
    there, clipping or not: the reducer hands EVERY parameter a gradient (zeros for the K-Net on a first frame: distributed.py,
    "parameters unused in the step contribute zeros"), so Adam counts a step for the K-Net that the reducer-free run, whose K-Net
    gradients are None, does not; the bias correction of the next update differs.  That count is asserted (3 vs 2)."""
    import torch.distributed as dist
    assert not dist.is_initialized()
    torch.cuda.set_device(0)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    want_t, want_s, want_c, _ = _eager_run(1, "fused", False, False)
    ff_t, ff_s, ff_c, _ = _eager_run(1, "fused")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        got_t, got_s, got_c, _ = _eager_run(1, "fused", True, False)
        gff_t, gff_s, gff_c, _ = _eager_run(1, "fused", True)
    finally:
        dist.destroy_process_group()
    print("[clip] one-rank RCCL: coef per step, three updates %s vs %s; first frame + two updates %s vs %s" % (got_c, want_c, gff_c, ff_c))
    assert got_c == want_c and sum(1 for c in got_c if c < 1.0) >= 2
    _same("one-rank RCCL reducer vs none, three updates, losses and predictions", got_t, want_t)
    _same("one-rank RCCL reducer vs none, three updates, state", got_s, want_s)
    assert gff_c[:2] == ff_c[:2]
    for k in ("loss0", "pred0", "lo0", "hi0", "loss1", "pred1", "lo1", "hi1"):
        assert torch.equal(gff_t[k], ff_t[k]), k
    key = "adam.kv_net.dres1.0.0.weight.step"
    assert float(gff_s[key]) == 3.0 and float(ff_s[key]) == 2.0 and float(got_s[key]) == 3.0 == float(want_s[key])


def _graph_wins(A):
    return _windows(5 * A, 10 + A)


def _graph_run(A):
    wins, m = _graph_wins(A), _max_norm(A)
    model = _model()
    opt = FusedAdam(model.parameters(), lr=1e-4)
    tg = TrainGraph(model, opt, 2, D_CANDI, CAM, warmup=1, accum_steps=A, deterministic=True, grad_clip_max=m)
    preds = _first_preds(model, wins, A)
    trace, coefs = {}, []
    for it in range(4):                               # eager warm-up, capture + first replay, two more replays
        ws = wins[A * (it + 1):A * (it + 2)]
        if A == 1:
            loss, nxt = tg.step(*ws[0], preds[0])
            preds = [nxt.clone()]
        else:
            loss, preds = tg.step_windows([w_ + (preds[k],) for k, w_ in enumerate(ws)])
        assert (tg._graph is None) == (it == 0)
        trace["loss%d" % it] = loss.clone()
        for k, p in enumerate(preds):
            trace["pred%d.%d" % (it, k)] = p.clone()
        coefs.append(float(opt.last_clip_coef))
    torch.cuda.synchronize()
    return trace, _state(model, opt), coefs


def _eager_seq(A):
    """The same four optimizer steps as _graph_run, through train(grad_clip_max=M)."""
    wins, m = _graph_wins(A), _max_norm(A)
    model = _model()
    opt = FusedAdam(model.parameters(), lr=1e-4)
    preds = _first_preds(model, wins, A)
    trace, coefs = {}, []
    for it in range(4):
        (_, _, loss, _, _), preds = _train_call(model, opt, wins[A * (it + 1):A * (it + 2)], preds, grad_clip_max=m)
        trace["loss%d" % it] = loss.clone()
        for k, p in enumerate(preds):
            trace["pred%d.%d" % (it, k)] = p.clone()
        coefs.append(float(opt.last_clip_coef))
    torch.cuda.synchronize()
    return trace, _state(model, opt), coefs


@pytest.mark.parametrize("A", [1, 2])
def test_train_graph_with_grad_clip_max(A):
    """A = 1: the one-graph form; A = 2: the split form (the clipped step is graph 2).  Two runs are bit-identical.  Against the eager
    train(grad_clip_max=M) sequence on the same windows the gates are those of the existing graph-vs-eager tests
    (tests/test_gpu_train.py: loss to 1e-3 relative, predicted volume mean |d| < 1e-3 — max |d| < 5e-2 in the split form —,
    kv_net.dres1 weights to 5e-4): no existing test holds that comparison to be exact.  The number of differing tensors is printed
    (measured on an MI355X: none of the 8 / 12 trace tensors and none of the 1,158 state tensors differ, in either form)."""
    t1, s1, c1 = _graph_run(A)
    t2, s2, c2 = _graph_run(A)
    te, se, ce = _eager_seq(A)
    print("[clip] TrainGraph accum %d: losses %s, coef per step graph %s eager %s" % (A, [float(t1["loss%d" % i]) for i in range(4)], c1, ce))
    assert all(bool(torch.isfinite(t1["loss%d" % i])) for i in range(4))
    assert sum(1 for c in c1 if c < 1.0) >= 2 and c1 == c2
    _same("TrainGraph(grad_clip_max) accum %d, two runs, losses and predictions" % A, t1, t2)
    _same("TrainGraph(grad_clip_max) accum %d, two runs, state" % A, s1, s2)
    print("[clip] TrainGraph vs eager accum %d: %d of %d trace tensors and %d of %d state tensors differ" % (
        A, sum(1 for k in t1 if not torch.equal(t1[k], te[k])), len(t1), sum(1 for k in s1 if not torch.equal(s1[k], se[k])), len(s1)))
    assert list(t1) == list(te) and list(s1) == list(se)
    for it in range(4):
        le = float(te["loss%d" % it])
        assert abs(float(t1["loss%d" % it]) - le) < 1e-3 * abs(le)
        for k in range(A):
            d = (t1["pred%d.%d" % (it, k)] - te["pred%d.%d" % (it, k)]).abs()
            assert d.mean().item() < 1e-3 and (A == 1 or d.max().item() < 5e-2)
    key = "model.kv_net.dres1.0.0.weight"
    assert (s1[key] - se[key]).abs().max().item() < 5e-4
    assert float(s1["adam.kv_net.dres1.0.0.weight.step"]) == 4.0 == float(se["adam.kv_net.dres1.0.0.weight.step"])
