"""Global-norm gradient clipping, host side: the float64 comparator of the GPU tests (tests/grad_clip_ref.py) against
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the CPU, and the argument checks of FusedAdam / train() / clip_grad_norm_ that
need no GPU."""
import copy
import math
import pickle

import numpy as np
import pytest
import torch

import grad_clip_ref as ref
from neuralrgbd_amd._lib import NrgbdError
from neuralrgbd_amd.optim import FusedAdam, clip_grad_norm_, grad_norm

SHAPES = [(1,), (63,), (5, 7), (2049,), (3, 4, 3, 3)]


def _case(kind):
    """(parameters, four steps of gradients, max_norm): the norm below max_norm, above it, or one gradient holding inf (step 2)."""
    g = torch.Generator().manual_seed(11)
    ps = [torch.randn(*s, generator=g, dtype=torch.float64) for s in SHAPES]
    steps = []
    for it in range(4):
        gs = [torch.randn(*s, generator=g, dtype=torch.float64) * 10.0 ** (i % 3 - 1) for i, s in enumerate(SHAPES)]
        if it % 2 == 1:
            gs[1] = None                          # a parameter without a gradient in some steps
        steps.append(gs)
    norms = [ref.total_norm(gs) for gs in steps]
    if kind == "below":
        m = 2.0 * max(norms)
    elif kind == "above":
        m = 0.25 * min(norms)
    else:
        m = 0.25 * min(norms)
        steps[2][3][-1] = math.inf
    return ps, steps, m


def _close(a, b):
    """Same NaN pattern, and the finite entries within 1e-12 of the tensor's largest magnitude (float64: eps 1.1e-16 over a handful
    of operations; the moments are signed sums, so the bound is relative to the tensor, not to each entry)."""
    a, b = a.detach(), b.detach()
    if not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    ok = ~torch.isnan(b)
    return not bool(ok.any()) or float((a[ok] - b[ok]).abs().max()) <= 1e-12 * float(b[ok].abs().max())


@pytest.mark.parametrize("kind", ["below", "above", "inf"])
@pytest.mark.parametrize("wd,maximize", [(0.0, False), (0.01, True)])
def test_comparator_equals_torch_clip_grad_norm_and_adam_in_float64(kind, wd, maximize):
    ps, steps, m = _case(kind)
    tp = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.Adam(tp, lr=1e-2, betas=(.9, .999), eps=1e-8, weight_decay=wd, maximize=maximize, foreach=False)
    rp = [p.clone() for p in ps]
    rm, rv, rt = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps], [0] * len(ps)
    for it, gs in enumerate(steps):
        for p, g in zip(tp, gs):
            p.grad = None if g is None else g.clone()
        want_norm = float(torch.nn.utils.clip_grad_norm_(tp, m))
        opt.step()
        norm, coef = ref.clipped_adam_step(rp, gs, rm, rv, rt, m, lr=1e-2, betas=(.9, .999), eps=1e-8, weight_decay=wd, maximize=maximize)
        if kind == "inf" and it == 2:
            assert math.isinf(norm) and math.isinf(want_norm) and coef == 0.0
        else:
            assert abs(norm - want_norm) <= 1e-13 * want_norm
            assert (coef == 1.0) == (kind == "below") and (kind == "below" or coef < 0.3)
        for i, (p, g) in enumerate(zip(tp, gs)):      # torch scaled the stored gradient by the same coefficient
            if g is not None and kind != "inf":
                assert torch.allclose(p.grad, g * coef, rtol=1e-13, atol=0)
    for i, (p, q) in enumerate(zip(tp, rp)):
        assert _close(p, q), i
        st = opt.state[p]
        assert int(st["step"]) == rt[i]
        assert _close(st["exp_avg"], rm[i]) and _close(st["exp_avg_sq"], rv[i]), i
    if kind == "inf":                             # torch's default: inf * 0 = NaN reaches the parameter that held the inf, and stays
        assert bool(torch.isnan(rp[3][-1])) and bool(torch.isfinite(rp[0]).all())


def test_coef_rules():
    assert ref.clip_coef(1.0, 2.0) == 1.0 and ref.clip_coef(4.0, 2.0) == 2.0 / (4.0 + 1e-6)
    assert ref.clip_coef(3.0, math.inf) == 1.0 and ref.clip_coef(0.0, 2.0) == 1.0
    assert ref.clip_coef(math.inf, 2.0) == 0.0 and math.isnan(ref.clip_coef(math.nan, 2.0)) and math.isnan(ref.clip_coef(math.inf, math.inf))
    t = torch.tensor(math.inf, dtype=torch.float64)
    assert math.isnan(float(torch.clamp(t / (t + 1e-6), max=1.0)))             # torch's own arithmetic for that corner


@pytest.mark.parametrize("bad", [0, 0.0, -1, -1.5, math.nan])
def test_fused_adam_refuses_a_non_positive_max_grad_norm(bad):
    ps = [torch.nn.Parameter(torch.randn(3))]
    with pytest.raises(ValueError):
        FusedAdam(ps, max_grad_norm=bad)
    opt = FusedAdam(ps, max_grad_norm=2.0)
    with pytest.raises(ValueError):
        opt.max_grad_norm = bad
    assert opt.max_grad_norm == 2.0
    with pytest.raises(ValueError):
        opt.step(max_grad_norm=bad)               # checked before any launch (there is no GPU here)


def test_attributes_are_settable_and_default_to_off():
    opt = FusedAdam([torch.nn.Parameter(torch.randn(3))])
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False
    opt.max_grad_norm, opt.skip_nonfinite = 2, True
    assert opt.max_grad_norm == 2.0 and isinstance(opt.max_grad_norm, float) and opt.skip_nonfinite is True
    opt.max_grad_norm = None
    assert opt.max_grad_norm is None
    assert "max_grad_norm" not in opt.defaults and "skip_nonfinite" not in opt.defaults
    assert set(opt.state_dict()) == {"state", "param_groups"}
    assert all("max_grad_norm" not in g and "skip_nonfinite" not in g for g in opt.state_dict()["param_groups"])


def test_attributes_survive_loading_a_reference_era_checkpoint():
    """The fixture dict of tests/test_host.py::test_fused_adam_loads_a_reference_era_checkpoint, restated: a torch < 1.12 Adam
    state dict knows nothing of the clipping attributes, and loading it (or pickling the optimizer) must not reset them."""
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7))]
    opt = FusedAdam(ps, lr=1e-3, max_grad_norm=2.0, skip_nonfinite=True)
    old = {"state": {0: {"step": 11, "exp_avg": torch.full((5, 3), 0.5), "exp_avg_sq": torch.full((5, 3), 0.25)},
                     1: {"step": 11, "exp_avg": torch.zeros(7), "exp_avg_sq": torch.ones(7)}},
           "param_groups": [{"lr": 1e-5, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "params": [0, 1]}]}
    opt.load_state_dict(copy.deepcopy(old))
    assert opt.max_grad_norm == 2.0 and opt.skip_nonfinite is True
    assert opt.param_groups[0]["lr"] == 1e-5 and opt.param_groups[0]["maximize"] is False and opt.state[ps[0]]["step"] == 11
    o2 = pickle.loads(pickle.dumps(opt))
    assert o2.max_grad_norm == 2.0 and o2.skip_nonfinite is True and o2.param_groups[0]["maximize"] is False
    plain = FusedAdam(ps, lr=1e-3)
    plain.load_state_dict(copy.deepcopy(old))
    assert plain.max_grad_norm is None and plain.skip_nonfinite is False
    tsd = torch.optim.Adam(ps, lr=1e-3).state_dict()                     # a torch.optim.Adam checkpoint of today
    opt.load_state_dict(tsd)
    assert opt.max_grad_norm == 2.0 and opt.skip_nonfinite is True


def test_train_refuses_skip_nonfinite_without_fused_adam_before_any_launch():
    from neuralrgbd_amd.train_step import TrainGraph, train
    model = torch.nn.Linear(2, 2)
    opt = torch.optim.Adam(model.parameters())
    with pytest.raises(ValueError, match="skip_nonfinite"):
        train(1, model, opt, 2, np.linspace(.1, 5, 8), [], [], None, None, [], skip_nonfinite=True)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        TrainGraph(model, opt, 2, np.linspace(.1, 5, 8), None, skip_nonfinite=True)
    for bad in (0, -2.0, math.nan):
        with pytest.raises(ValueError, match="max_grad_norm"):
            train(1, model, FusedAdam(model.parameters()), 2, np.linspace(.1, 5, 8), [], [], None, None, [], grad_clip_max=bad)
    assert all(p.grad is None for p in model.parameters())


def test_free_functions_refuse_cpu_tensors_and_other_norm_types():
    p = torch.nn.Parameter(torch.randn(9))
    p.grad = torch.randn(9)
    with pytest.raises(NrgbdError):
        clip_grad_norm_([p], 1.0)
    with pytest.raises(NrgbdError):
        clip_grad_norm_(p, 1.0)                   # a single tensor, as torch takes it
    with pytest.raises(NrgbdError):
        grad_norm([p])
    for nt in (1, math.inf, 3.0):
        with pytest.raises(NrgbdError):
            clip_grad_norm_([p], 1.0, norm_type=nt)
    with pytest.raises(ValueError):
        clip_grad_norm_([p], 0.0)
    assert torch.equal(p.grad, p.grad.clone()) and float(clip_grad_norm_([torch.nn.Parameter(torch.zeros(2))], 1.0)) == 0.0


def test_new_entries_are_declared_and_bound():
    import os
    from conftest import ROOT
    from neuralrgbd_amd import _lib
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    for name in ("nrgbd_grad_norm_workspace", "nrgbd_grad_norm", "nrgbd_scale_tensors", "nrgbd_adam_step_clipped"):
        assert name + "(" in header and name in _lib.SIGNATURES
    assert "train_KVNet.py:143-145,180-181" in header and "clip_grad_norm_" in header
    a, c = _lib.SIGNATURES["nrgbd_adam_step"][1], _lib.SIGNATURES["nrgbd_adam_step_clipped"][1]
    assert c[:len(a) - 1] == a[:-1] and len(c) == len(a) + 2 and c[-1] == a[-1]
    lib = _lib.load()                             # the refusals of the C side need no GPU: nothing is launched
    n = (_lib._L * 2)(2048, 2049)
    assert lib.nrgbd_grad_norm_workspace(n, 2) == 3 * 4 and lib.nrgbd_grad_norm_workspace(n, 0) == 0
    assert lib.nrgbd_grad_norm_workspace((_lib._L * 1)(0), 1) == -2 and lib.nrgbd_grad_norm_workspace(None, 1) == -1
