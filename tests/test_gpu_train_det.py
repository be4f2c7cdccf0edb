"""Bit-reproducible training (train(..., deterministic=True), TrainGraph(..., deterministic=True)): two identical runs give identical
losses, predicted volumes, weights, BatchNorm statistics and Adam moments.  The window of the other training tests: 256x256 images,
D = 8, seeded state dict, FusedAdam."""
import numpy as np
import pytest
import torch

import neuralrgbd_amd
from neuralrgbd_amd import camera, synth
from neuralrgbd_amd.optim import FusedAdam
from neuralrgbd_amd.test_step import test as infer
from neuralrgbd_amd.train_step import TrainGraph, train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, D = 256, 256, 8
CAM = camera.scannet_intrinsics(W // 4, H // 4)
D_CANDI = np.linspace(0.1, 5, D)


def _model():
    m = neuralrgbd_amd.KVNET(64, CAM, D_CANDI, 10.0, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=2)
    m.load_state_dict(synth.seeded_state_dict(m, 0))
    return m.to(DEV)


def _windows(n, seed):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        r, s, p = synth.noise_window(4000 + 10 * seed + i, H, W)
        out.append((r.to(DEV), s.to(DEV), p.to(DEV), torch.from_numpy(rng.randint(0, D, (1, H // 4, W // 4))).to(DEV),
                    torch.from_numpy(rng.randint(0, D, (1, H, W))).to(DEV)))
    return out


def _train_call(model, opt, w_, pred, deterministic):
    r, s, p, dm, dmf = w_
    return train(1, model, opt, 2, D_CANDI, [{"img": r, "dmap": dm, "dmap_imgsize_digit": dmf}],
                 [[{"img": s[0, v:v + 1]} for v in range(4)]], p, pred, [CAM], deterministic=deterministic)


def _first_difference(tag, a, b):
    """Names of the tensors of two {name: tensor} dicts that differ, in order; asserts there is none."""
    assert list(a) == list(b)
    bad = [(k, int((a[k] != b[k]).sum()), a[k].numel(), float((a[k].double() - b[k].double()).abs().max())) for k in a
           if not torch.equal(a[k], b[k])]
    print("[det] %s: %d tensors compared, %d differ%s" % (tag, len(a), len(bad), "".join(
        "\n      %s: %d of %d elements, max |d| %.3e" % x for x in bad[:8])))
    assert not bad, "%s: first differing tensor %s (%d differ)" % (tag, bad[0][0], len(bad))


def _state(model, opt):
    out = {"model." + k: v.detach().clone() for k, v in model.state_dict().items()}
    names = {p: n for n, p in model.named_parameters()}
    for p, st in opt.state.items():
        for key in ("exp_avg", "exp_avg_sq", "step"):
            if key in st and isinstance(st[key], torch.Tensor):
                out["adam.%s.%s" % (names[p], key)] = st[key].detach().clone()
    return out


def _eager_run(wins):
    model = _model()
    opt = FusedAdam(model.parameters(), lr=1e-4)
    pred, trace = None, {}
    for i, w_ in enumerate(wins):                     # first frame (no predicted volume), then update iterations
        _, pred, loss, lo, hi = _train_call(model, opt, w_, pred, True)
        trace["loss%d" % i], trace["pred%d" % i], trace["lo%d" % i], trace["hi%d" % i] = loss.clone(), pred.clone(), lo.clone(), hi.clone()
    torch.cuda.synchronize()
    return trace, _state(model, opt)


def test_eager_training_is_bit_reproducible():
    from neuralrgbd_amd import autograd as ag
    wins = _windows(3, 1)
    t1, s1 = _eager_run(wins)
    t2, s2 = _eager_run(wins)
    assert ag.is_deterministic() is False             # train() restored the switch
    n_par = sum(1 for k in s1 if k.startswith("model."))
    n_adam = sum(1 for k in s1 if k.endswith(".exp_avg"))
    print("[det] eager: %d state-dict tensors, %d parameters with Adam moments, losses %s"
          % (n_par, n_adam, [float(t1["loss%d" % i]) for i in range(3)]))
    assert n_adam == len(list(_model().parameters())) and all(bool(torch.isfinite(t1["loss%d" % i])) for i in range(3))
    _first_difference("eager train(deterministic=True), losses and predictions", t1, t2)
    _first_difference("eager train(deterministic=True), weights, BN statistics, Adam moments", s1, s2)
    # the weights moved: the comparison is not between two untouched copies
    fresh = _model().state_dict()
    assert sum(1 for k, v in fresh.items() if not torch.equal(v, s1["model." + k])) > 200


def _graph_run(wins, accum):
    model = _model()
    opt = FusedAdam(model.parameters(), lr=1e-4)
    tg = TrainGraph(model, opt, 2, D_CANDI, CAM, warmup=1, accum_steps=accum, deterministic=True)
    with torch.no_grad():
        preds = [infer(model, D_CANDI, [CAM], 2, [{"img": w_[0]}], [[{"img": w_[1][0, v:v + 1]} for v in range(4)]], w_[2], None)[1].clone()
                 for w_ in wins[:accum]]
    trace = {}
    for it in range(4):                               # eager warm-up, capture + first replay, two more replays
        ws = wins[accum * (it + 1):accum * (it + 2)]
        if accum == 1:
            loss, nxt = tg.step(*ws[0], preds[0])
            preds = [nxt.clone()]
        else:
            loss, preds = tg.step_windows([w_ + (preds[k],) for k, w_ in enumerate(ws)])
        assert (tg._graph is None) == (it == 0)
        trace["loss%d" % it] = loss.clone()
        for k, p in enumerate(preds):
            trace["pred%d.%d" % (it, k)] = p.clone()
    torch.cuda.synchronize()
    return trace, _state(model, opt)


@pytest.mark.parametrize("accum", [1, 2])
def test_train_graph_is_bit_reproducible(accum):
    """accum 1: the one-graph form; accum 2: the split form (forward/backward graph replayed per window, optimizer graph) without
    a reducer."""
    wins = _windows(5 * accum, 2 + accum)
    t1, s1 = _graph_run(wins, accum)
    t2, s2 = _graph_run(wins, accum)
    print("[det] TrainGraph accum %d: losses %s" % (accum, [float(t1["loss%d" % i]) for i in range(4)]))
    assert all(bool(torch.isfinite(t1["loss%d" % i])) for i in range(4))
    _first_difference("TrainGraph(deterministic=True) accum %d, losses and predictions" % accum, t1, t2)
    _first_difference("TrainGraph(deterministic=True) accum %d, weights, BN statistics, Adam moments" % accum, s1, s2)


def test_deterministic_gradient_equals_the_default_gradient():
    """One update iteration with the switch on and off: the gradients agree to 1e-3 of each tensor's largest entry (the gate of
    tests/test_gpu_dist.py for the same kind of comparison: the default mode's own run-to-run noise lies inside it)."""
    wins = _windows(2, 7)
    grads = {}
    for flag in (True, False):
        model = _model()
        opt = FusedAdam(model.parameters(), lr=1e-5)
        with torch.no_grad():
            pred = infer(model, D_CANDI, [CAM], 2, [{"img": wins[0][0]}], [[{"img": wins[0][1][0, v:v + 1]} for v in range(4)]],
                         wins[0][2], None)[1].clone()
        _train_call(model, opt, wins[1], pred, flag)
        torch.cuda.synchronize()
        grads[flag] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    assert set(grads[True]) == set(grads[False]) and len(grads[True]) > 200
    worst = 0.0
    for k, want in grads[False].items():
        scale = want.abs().max().item()
        err = (grads[True][k] - want).abs().max().item()
        worst = max(worst, err / max(scale, 1e-20))
        assert err <= 1e-3 * scale + 1e-12, (k, err, scale)
    print("[det] gradient, switch on vs off: %d tensors, worst max|d| / max|g| = %.2e" % (len(grads[True]), worst))
