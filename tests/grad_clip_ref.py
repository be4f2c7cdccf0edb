"""Float64 comparator of global-norm gradient clipping followed by an Adam step — a restatement of
torch.nn.utils.clip_grad_norm_ (norm type 2: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1, gradients scaled by it) and of
torch.optim.adam._single_tensor_adam, on lists of float64 tensors.  tests/test_grad_clip_host.py holds it against torch itself on the
CPU; the GPU tests hold csrc/optim.hip against it."""
import math

import torch


def total_norm(grads):
    """sqrt of the sum of squares over every element of every tensor, in float64 (None entries: no gradient)."""
    s = torch.zeros((), dtype=torch.float64)
    for g in grads:
        if g is not None:
            s = s + (g.detach().double().cpu() ** 2).sum()
    return float(torch.sqrt(s))


def clip_coef(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)) with torch.clamp's NaN rule: a NaN stays a NaN."""
    q = float(max_norm) / (float(norm) + 1e-6) if not (math.isinf(max_norm) and math.isinf(norm)) else math.nan
    return q if (q < 1.0 or q != q) else 1.0


def clipped_adam_step(params, grads, exp_avg, exp_avg_sq, steps, max_norm, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                      maximize=False, coef=None):
    """One step, in place, on lists of float64 tensors (`steps`: list of Python ints, advanced).  grads[i] None: parameter i is left
    out of the norm and of the update, and its step count stays.  max_norm None: no clipping.  `coef`: the coefficient of a norm taken
    over more tensors than this call's (several parameter groups).  Returns (total_norm, coef)."""
    norm = total_norm(grads)
    if coef is None:
        coef = 1.0 if max_norm is None else clip_coef(norm, max_norm)
    b1, b2 = betas
    for i, g in enumerate(grads):
        if g is None:
            continue
        g = g.double()
        if max_norm is not None:
            g = g * coef
        if maximize:
            g = -g
        p, m, v = params[i], exp_avg[i], exp_avg_sq[i]
        if weight_decay != 0:
            g = g + weight_decay * p
        steps[i] += 1
        t = steps[i]
        m += (g - m) * (1 - b1)
        v.mul_(b2).add_((1 - b2) * g * g)
        step_size = lr / (1 - b1 ** t)
        denom = v.sqrt() / math.sqrt(1 - b2 ** t) + eps
        p -= step_size * (m / denom)
    return norm, coef
