"""Adam for the training loop on ONE hand-written multi-tensor kernel (csrc/optim.hip).

`FusedAdam` is a drop-in for the reference's `optim.Adam(model_KVnet.parameters(), lr=..., betas=(.9, .999))`
(train_KVNet.py:228-232; stepped at train_utils/train_KVNet.py:153): same constructor arguments (no amsgrad), same per-parameter
state names (`step`, `exp_avg`, `exp_avg_sq`) so checkpoints interchange with torch.optim.Adam, same arithmetic
(`torch.optim.adam._single_tensor_adam`, fp32).  What differs is the execution: the update of all 459 tensors is ~10 launches of
one kernel whose tensor pointers travel in the kernel arguments — no `_foreach_` slabs, no host synchronisation, capturable into a
hipGraph as it is (the step counters live on the device).  CUDA-device fp32 parameters only; anything else raises.

Global-norm gradient clipping (the reference's `--grad_clip --grad_clip_max 2.`: `torch.nn.utils.clip_grad_norm_` before the step,
train_utils/train_KVNet.py:143-145,180-181) runs on the same kernels' tensor-list idiom: `FusedAdam(max_grad_norm=M)` folds the
coefficient into the update's gradient read, `clip_grad_norm_` / `grad_norm` are the free functions for any other optimizer.  No
`_foreach_` launch, no host synchronisation, no allocation in the step, capturable, and the same bits in every run."""
import ctypes
import math

import torch

from . import _lib

_UNSET = object()


def _check_max_norm(m):
    if m is None:
        return None
    m = float(m)
    if not m > 0.0:                      # <= 0 and NaN
        raise ValueError("max_grad_norm must be > 0 (got %r)" % (m,))
    return m


def _ptr_table(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _norm_launch(lib, grads, max_norm, ws, clip, counter, dev):
    """nrgbd_grad_norm over the fp32 device tensors `grads` into the record `clip`; returns the host tables (pointers, counts)."""
    n = len(grads)
    tab = (_ptr_table([g.data_ptr() for g in grads]), (ctypes.c_long * n)(*[g.numel() for g in grads]), n)
    _norm_run(lib, tab, max_norm, ws, clip, counter, dev)
    return tab


def _norm_run(lib, tab, max_norm, ws, clip, counter, dev):
    with torch.cuda.device(dev):
        rc = lib.nrgbd_grad_norm(tab[0], tab[1], tab[2], float(max_norm), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4,
                                 ctypes.c_void_p(clip.data_ptr()), ctypes.c_void_p(counter.data_ptr()) if counter is not None else None,
                                 ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc, "nrgbd_grad_norm")


def _workspace_floats(lib, numels):
    n = len(numels)
    nb = lib.nrgbd_grad_norm_workspace((ctypes.c_long * n)(*numels), n) if n else 0
    if nb < 0:
        _lib.check(int(nb), "nrgbd_grad_norm_workspace")
    return max(1, nb // 4)


def _dense_grads(parameters, what):
    """The gradients torch.nn.utils.clip_grad_norm_ would take, checked for this path: fp32, dense, on ONE GPU, contiguous."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    ps = [p for p in parameters if p.grad is not None]
    for p in ps:
        g = p.grad
        if not (g.is_cuda and g.dtype == torch.float32 and not g.is_sparse):
            raise _lib.NrgbdError("%s: fp32 dense gradients on the GPU only (got %s %s)" % (what, g.device, g.dtype))
        if not g.is_contiguous():
            p.grad = g.contiguous()
    grads = [p.grad for p in ps if p.grad.numel() > 0]
    if len({g.device for g in grads}) > 1:
        raise _lib.NrgbdError("%s: gradients on more than one device" % what)
    return grads


def _free_norm(parameters, max_norm, what, scale):
    grads = _dense_grads(parameters, what)
    if not grads:
        return torch.zeros(())                    # torch's answer for an empty list
    lib = _lib.load()
    dev = grads[0].device
    ws = torch.empty(_workspace_floats(lib, [g.numel() for g in grads]), dtype=torch.float32, device=dev)
    clip = torch.empty(4, dtype=torch.float32, device=dev)
    tab = _norm_launch(lib, grads, max_norm, ws, clip, None, dev)
    if scale:
        with torch.cuda.device(dev):
            rc = lib.nrgbd_scale_tensors(tab[0], tab[1], tab[2], ctypes.c_void_p(clip.data_ptr()),
                                         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _lib.check(rc, "nrgbd_scale_tensors")
    return clip[0]


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """Drop-in for torch.nn.utils.clip_grad_norm_ (norm type 2) on csrc/optim.hip: the global norm of the gradients in a fixed
    summation order, then `g *= min(1, max_norm / (norm + 1e-6))` in place — two kernel types, no `_foreach_` launch, no host
    synchronisation, capturable into a hipGraph.  Returns the total norm as a 0-dim device tensor.  A non-finite norm goes through
    as in torch's default (coef 0 or NaN); `error_if_nonfinite=True` would need a host synchronisation and is refused.  For an
    optimizer other than FusedAdam (which folds the scale into its update: FusedAdam(max_grad_norm=...))."""
    if float(norm_type) != 2.0:
        raise _lib.NrgbdError("clip_grad_norm_: norm type 2 only (got %r)" % (norm_type,))
    if error_if_nonfinite:
        raise _lib.NrgbdError("clip_grad_norm_: error_if_nonfinite needs a host synchronisation; read the returned norm instead")
    m = _check_max_norm(max_norm)
    if m is None:
        raise ValueError("clip_grad_norm_: max_norm is required")
    return _free_norm(parameters, m, "clip_grad_norm_", True)


@torch.no_grad()
def grad_norm(parameters):
    """The global L2 norm of the gradients (0-dim device tensor): clip_grad_norm_'s kernels with nothing scaled."""
    return _free_norm(parameters, math.inf, "grad_norm", False)


class FusedAdam(torch.optim.Optimizer):
    """max_grad_norm = M (None: off): every step() first takes the global L2 norm over the gradients of ALL groups and updates with
    g * min(1, M / (norm + 1e-6)) — torch.nn.utils.clip_grad_norm_(params, M) followed by the step, bit for bit, without
    rewriting the gradients.  skip_nonfinite = True: a step whose norm is inf / NaN changes nothing (parameters, moments and step
    counts stay; `nonfinite_steps` counts it).  The default False is torch's behaviour: the coefficient is 0 or NaN and NaN reaches
    the parameters (and both moments, for good).  Both are attributes of the optimizer (the norm is global), settable at any time
    and not part of the state dict.  `last_grad_norm`, `last_clip_coef` and `nonfinite_steps` are 0-dim device views of the
    persistent record the kernels write: reading them launches nothing, `.item()` synchronises."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False, max_grad_norm=None,
                 skip_nonfinite=False):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FusedAdam: invalid hyper-parameters lr=%r betas=%r eps=%r weight_decay=%r" % (lr, betas, eps, weight_decay))
        max_grad_norm = _check_max_norm(max_grad_norm)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize))
        self._tables = {}
        self._max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self._clip_bufs = None

    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, m):
        self._max_grad_norm = _check_max_norm(m)

    def _clip_buffers(self):
        """(workspace, clip record [4], non-finite counter [1]) — persistent, so that a captured step() finds them where they were.
        The workspace is sized for every trainable parameter, whichever of them have a gradient in a given step."""
        b = self._clip_bufs
        count = sum(len(group["params"]) for group in self.param_groups)
        if b is not None and b[3] == count:
            return b[:3]
        ps = [p for group in self.param_groups for p in group["params"] if p.requires_grad and p.numel() > 0]
        devs = {p.device for p in ps}
        if len(devs) != 1 or next(iter(devs)).type != "cuda":
            raise _lib.NrgbdError("FusedAdam: gradient clipping needs the parameters on ONE GPU (got %s)" %
                                  sorted(str(d) for d in devs))
        dev = next(iter(devs))
        need = _workspace_floats(_lib.load(), [p.numel() for p in ps])
        if b is None:
            b = (torch.empty(need, dtype=torch.float32, device=dev), torch.tensor([0., 1., 0., 0.], dtype=torch.float32, device=dev),
                 torch.zeros(1, dtype=torch.float32, device=dev), count)
        else:                                     # add_param_group since: the record and the counter stay where they are
            b = (b[0] if b[0].numel() >= need else torch.empty(need, dtype=torch.float32, device=dev), b[1], b[2], count)
        self._clip_bufs = b
        return b[:3]

    @property
    def last_grad_norm(self):
        """Total norm of the last clipped step (0-dim device view; 0 before the first)."""
        return self._clip_buffers()[1][0]

    @property
    def last_clip_coef(self):
        """min(1, max_grad_norm / (norm + 1e-6)) of the last clipped step (0-dim device view; 1 before the first)."""
        return self._clip_buffers()[1][1]

    @property
    def nonfinite_steps(self):
        """Number of steps whose gradient norm was inf / NaN since construction (0-dim device float view)."""
        return self._clip_buffers()[2][0]

    def __getstate__(self):
        st = dict(super().__getstate__())
        st["_max_grad_norm"], st["skip_nonfinite"] = self._max_grad_norm, self.skip_nonfinite
        return st

    def _transient_defaults(self):
        d = self.__dict__
        d.setdefault("_max_grad_norm", None)
        d.setdefault("skip_nonfinite", False)
        d.setdefault("_clip_bufs", None)

    def _state_of(self, p):
        st = self.state[p]
        if not st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        elif not torch.is_tensor(st["step"]):       # a checkpoint of the reference's torch era (< 1.12): `step` is a Python int
            st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32, device=p.device)
        elif not (st["step"].is_cuda and st["step"].dtype == torch.float32):     # a torch.optim.Adam checkpoint: host-side counter
            st["step"] = st["step"].detach().to(device=p.device, dtype=torch.float32).reshape(())
        return st

    def load_state_dict(self, state_dict):
        """torch.optim.Adam checkpoints load as they are (train_KVNet.py:347 saves `optimizer.state_dict()`), except AMSGrad
        ones: this kernel keeps no running maximum of the second moment, and dropping it silently would change the training."""
        for group in state_dict.get("param_groups", ()):       # refuse BEFORE any state is replaced
            if group.get("amsgrad"):
                raise _lib.NrgbdError("FusedAdam: the loaded param_group has amsgrad=True; this optimizer has no AMSGrad form")
        super().load_state_dict(state_dict)
        # a checkpoint of the reference's torch era (< 1.12) carries only lr / betas / eps / weight_decay / amsgrad per group:
        # super() REPLACES the groups with the loaded ones, so the keys step() reads (`maximize`) are filled from the defaults
        for group in self.param_groups:
            for k, v in self.defaults.items():
                group.setdefault(k, v)
        self._tables = {}                                       # the moments are new tensors: the pointer tables are stale
        self._transient_defaults()                              # max_grad_norm / skip_nonfinite are no part of a state dict: kept

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            for k, v in self.defaults.items():
                group.setdefault(k, v)
        self._tables = {}
        self._transient_defaults()

    def mark_updated(self):
        """Advance the version counter of every parameter this optimizer owns.  The kernel writes through raw pointers, which
        autograd's version counters do not see; the inference-side caches (nets.py: packed weight streams, the clamped-FMA unit)
        are keyed on them.  step() calls this itself; a hipGraph REPLAY of a captured step() runs no Python, so whoever replays
        calls it (train_step.TrainGraph does)."""
        for group in self.param_groups:
            for p in group["params"]:
                if p.requires_grad:
                    torch._C._increment_version(p)

    def init_state(self):
        """Create the state of every parameter now (before a hipGraph capture: a state created inside a capture would become
        graph nodes that reset the moments at every replay)."""
        for group in self.param_groups:
            for p in group["params"]:
                if p.requires_grad:
                    self._state_of(p)
        if any(p.is_cuda for group in self.param_groups for p in group["params"]):
            self._clip_buffers()

    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=_UNSET, skip_nonfinite=_UNSET):
        """max_grad_norm / skip_nonfinite: override the attributes of the same name for this call (None / False: off)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        max_norm = self._max_grad_norm if max_grad_norm is _UNSET else _check_max_norm(max_grad_norm)
        skip = bool(self.skip_nonfinite if skip_nonfinite is _UNSET else skip_nonfinite)
        clipped = max_norm is not None or skip
        work = []
        for gi, group in enumerate(self.param_groups):
            ptrs, key = [], []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and not g.is_sparse):
                    raise _lib.NrgbdError("FusedAdam: fp32 dense parameters on the GPU only (got %s %s)" % (p.device, p.dtype))
                if not p.is_contiguous():
                    raise _lib.NrgbdError("FusedAdam: parameter of shape %s is not contiguous" % (tuple(p.shape),))
                if not g.is_contiguous():
                    g = p.grad = g.contiguous()
                st = self._state_of(p)
                ptrs.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(), p.numel()))
                key.append(ptrs[-1])
            if not ptrs:
                continue
            key = tuple(key)
            hit = self._tables.get(gi)
            if hit is None or hit[0] != key:        # the host-side pointer arrays, rebuilt only when a tensor moved
                n = len(ptrs)
                arrs = [(ctypes.c_void_p * n)(*[t[k] for t in ptrs]) for k in range(5)]
                arrs.append((ctypes.c_long * n)(*[t[5] for t in ptrs]))
                hit = (key, arrs, n)
                self._tables[gi] = hit
            work.append((group, hit, ptrs))
        clip = None
        if clipped and work:
            # ONE norm over the gradients of all groups (the tensors the update below reads), then every group's update scaled by it
            ws, clip, counter = self._clip_buffers()
            key = tuple((t[1], t[5]) for _, _, ptrs in work for t in ptrs)
            hit = self._tables.get("norm")
            if hit is None or hit[0] != key:
                hit = (key, (_ptr_table([k[0] for k in key]), (ctypes.c_long * len(key))(*[k[1] for k in key]), len(key)))
                self._tables["norm"] = hit
            _norm_run(lib, hit[1], math.inf if max_norm is None else max_norm, ws, clip, counter, clip.device)
        for group, (_, arrs, n), _ in work:
            dev = group["params"][0].device
            args = (arrs[0], arrs[1], arrs[2], arrs[3], arrs[4], arrs[5], n, float(group["lr"]),
                    float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                    float(group["weight_decay"]), int(bool(group["maximize"])))
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            with torch.cuda.device(dev):
                if clip is None:
                    rc = lib.nrgbd_adam_step(*args, stream)
                else:
                    rc = lib.nrgbd_adam_step_clipped(*args, ctypes.c_void_p(clip.data_ptr()), int(skip), stream)
            _lib.check(rc, "nrgbd_adam_step_clipped" if clip is not None else "nrgbd_adam_step")
            for p in group["params"]:
                if p.grad is not None:
                    torch._C._increment_version(p)      # like torch.optim.Adam's in-place ops (see mark_updated)
        return loss
