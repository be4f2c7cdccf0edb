"""Autograd bindings of the fused sampling kernels (training path, BASELINE config 4).

Inference never touches this module.  Under autograd the D-Net uses
    texels = PackNHWC(features, frames)        backward: channel slice + layout change (no gradient to the images)
    cost   = PlaneSweepCost(texels, ...)       backward: csrc/costvol_bwd.hip
the convolutions / BatchNorms of the three networks go through Conv2dCL / Conv3dCL / BatchNormActCL / UpsampleBilinearCL below
(hand-written kernels in all three directions); log-softmax, LeakyReLU and the NLL losses are ATen element-wise kernels.
"""
import torch

from . import _lib, ops


# Bit-reproducible training (opt-in).  The one order-dependent reduction of the training path is the scatter of the cost-volume
# backward (csrc/costvol_bwd.hip: float atomics); with the switch on, PlaneSweepCost takes csrc/costvol_bwd_det.hip instead.  A
# process-wide flag of this module, nothing else: neither torch's deterministic-algorithms setting nor the environment is consulted.
_DETERMINISTIC = False


def set_deterministic(flag):
    """Switch the bit-reproducible cost-volume backward on or off for the forwards that follow.  Returns the previous value."""
    global _DETERMINISTIC
    prev, _DETERMINISTIC = _DETERMINISTIC, bool(flag)
    return prev


def is_deterministic():
    return _DETERMINISTIC


class deterministic:
    """Context manager: the switch set to `flag` inside, the previous value restored on exit (also after an exception).
    flag = None leaves the switch alone (train(..., deterministic=None): follow the switch)."""

    def __init__(self, flag=True):
        self.flag = flag

    def __enter__(self):
        self.prev = _DETERMINISTIC
        if self.flag is not None:
            set_deterministic(self.flag)
        return self

    def __exit__(self, *exc):
        set_deterministic(self.prev)
        return False


class PackNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, rgb):
        ctx.cf = feat.shape[1]
        return ops.pack_nhwc(feat, rgb)

    @staticmethod
    def backward(ctx, g_tex):
        return g_tex[..., :ctx.cf].permute(0, 3, 1, 2).contiguous(), None


class PlaneSweepCost(torch.autograd.Function):
    """cost [D,h,w] of texels [V+1,h,w,Cp] (last = reference view)."""

    @staticmethod
    def forward(ctx, texels, KR, Kt, rays, d_candi, cx, cy, sigma, C, dist, align_corners):
        V = texels.shape[0] - 1
        cost, _ = ops.costvol(texels[V], texels[:V], KR, Kt, rays, d_candi, cx, cy, sigma, C, dist=dist,
                              align_corners=align_corners, want_cost=True, want_logp=False)
        ctx.save_for_backward(texels, KR, Kt, rays, d_candi)
        ctx.meta = (cx, cy, sigma, C, dist, align_corners)
        ctx.deterministic = _DETERMINISTIC     # the backward follows the forward it belongs to, wherever and whenever it runs
        return cost

    @staticmethod
    def backward(ctx, g_cost):
        texels, KR, Kt, rays, d_candi = ctx.saved_tensors
        cx, cy, sigma, C, dist, align = ctx.meta
        V = texels.shape[0] - 1
        g_ref, g_src = ops.costvol_bwd(texels[V], texels[:V], KR, Kt, rays, d_candi, cx, cy, sigma, C,
                                       g_cost.contiguous(), dist=dist, align_corners=align, deterministic=ctx.deterministic)
        return (torch.cat((g_src, g_ref.unsqueeze(0)), dim=0),) + (None,) * 10


class DepthWarp(torch.autograd.Function):
    """Warp of N source images through a per-pixel depth map (warping/homography.py:479-528), differentiable w.r.t. the
    rigid motions (R [N,3,3], t [N,3]) the local bundle adjustment refines (ICP/opt_pose_numerical.py:245-294):
    forward = nrgbd_warp_depth_fwd, backward = nrgbd_warp_depth_bwd.  No gradient is produced for the images or the depth
    map (the reference's caller never asks for one)."""

    @staticmethod
    def forward(ctx, src, dmap, K, R, t, rays):
        R, t = R.contiguous(), t.contiguous()
        ctx.save_for_backward(src, dmap, K, R, t, rays)
        return ops.warp_depth_fwd(src, dmap, K, R, t, rays)

    @staticmethod
    def backward(ctx, g_out):
        src, dmap, K, R, t, rays = ctx.saved_tensors
        g_R, g_t = ops.warp_depth_bwd(src, dmap, K, R, t, rays, g_out.contiguous())
        return None, None, None, g_R, g_t, None


# Packed weight streams of the training path, valid for ONE optimizer step.  train(..., accum_steps = A) and TrainGraph.step_windows run A
# windows on the same weights: inside `with pack_cache():` the first window packs every layer's streams (forward + data gradient) and the
# others read them (0.9 ms of packing launches per window at the training grid: VERDICT r5 item 6).  Keys are (id of the module's weight
# parameter, what was packed); the scope ends before the optimizer changes the weights.
_PACK_CACHE = None


class pack_cache:
    """Context manager: weight streams packed inside it are kept and reused until it exits.  `store`: an existing dict (TrainGraph
    keeps the streams its first-window graph writes so that the graph of the later windows reads the same buffers)."""

    def __init__(self, store=None):
        self.store = {} if store is None else store

    def __enter__(self):
        global _PACK_CACHE
        self.prev, _PACK_CACHE = _PACK_CACHE, self.store
        return self.store

    def __exit__(self, *exc):
        global _PACK_CACHE
        _PACK_CACHE = self.prev
        return False


def _cached(key, tag, fn):
    if _PACK_CACHE is None or key is None:
        return fn()
    hit = _PACK_CACHE.get((key, tag))
    if hit is None:
        hit = _PACK_CACHE[(key, tag)] = fn()
    return hit


class Conv3dCL(torch.autograd.Function):
    """3x3x3 convolution (stride 1, padding 1, no bias, 64 outputs) on channels-last activations, both directions on
    the fp32 matrix cores: forward = csrc/wino_dw.hip / wino_pc.hip (64 -> 64 layers, Winograd domain) / csrc/conv3d.hip; data gradient = the
    same kernel on the output gradient with transposed + flipped weights; weight gradient = csrc/conv3d_wgrad.hip.

    x [D,H,W,Cin] (Cin in {16, 32, 64}), w [64,C,3,3,3] -> y [D,H,W,64].  C < Cin (the K-Net's first layer at a window of 3 or 7
    frames: 10 -> 16, 22 -> 32): x carries zeros in channels C .. Cin-1, the weight streams are packed from w zero-padded to Cin, and
    the weight gradient of the padded rows is dropped — the parameter and its .grad keep the shape [64,C,3,3,3].
    """

    # Candidate kernels in order of preference (ops.conv3d_kernel holds the table and the reasons).  A/B: drop "dw4" from all three
    kernels = ("dw4", "dw", "pc", "direct")           # the 64 -> 64 layers, both directions
    kernels_first = ("dw4", "direct")                 # the 16 -> 64 first layer, forward
    kernels_first_dgrad = ("dw4", "dw", "direct")     # ... its data gradient: a 64 -> 64 (16 real) layer on the output gradient
    kernels_first32 = ("dw4", "dw", "pc")             # the first layer at 32 inputs (a 7-frame window), forward: conv3d.hip has no 32-input form

    @staticmethod
    def _conv(x, w, transposed=False, packed=None, key=None):
        """y = conv(x, w) (transposed: with w's data-gradient weights): choose the kernel, fetch its weight stream, launch.
        packed: (kind, stream) of this call if the caller already has it; key: pack_cache key of the layer."""
        cin = w.shape[1] if transposed else x.shape[-1]               # forward: the width of x (w zero-padded to it)
        kind = ops.conv3d_kernel(*x.shape, 64, Conv3dCL.kernels if cin == 64 else Conv3dCL.kernels_first_dgrad if transposed
                                 else Conv3dCL.kernels_first32 if cin == 32 else Conv3dCL.kernels_first)

        def stream():
            wf = w.contiguous()
            if not transposed and cin != w.shape[1]:
                wf = torch.cat((wf, wf.new_zeros(64, cin - w.shape[1], 3, 3, 3)), dim=1)
            if transposed:                                            # as a forward layer of THIS call
                wf = w.transpose(0, 1).flip(2, 3, 4)                  # [Cin, 64, 3,3,3]: correlation with the flipped kernel
                if cin < 64:                                          # the kernels produce 64 outputs: pad, then slice
                    wf = torch.cat((wf, wf.new_zeros(64 - cin, 64, 3, 3, 3)), dim=0)
                wf = wf.contiguous()
            return {"dw4": ops.conv_wino_dw4_pack, "dw": ops.conv_wino_dw_pack, "pc": ops.conv_wino_pack, "direct": ops.conv3d_pack_weights}[kind](wf)
        wp = packed[1] if packed is not None and packed[0] == kind else _cached(key, (kind, bool(transposed), cin), stream)
        if kind == "dw4":                                             # F(4,3) along depth (wino_dw4.hip)
            y = ops.conv_wino_dw4(x, wp, 64, want_stats=False)[0]
        elif kind == "dw":                                            # F(2,3) along depth (wino_dw.hip)
            y = ops.conv_wino_dw(x, wp, 64, want_stats=False)[0]
        elif kind == "pc":
            y = ops.conv_wino(x, wp, 64, 3, want_stats=False)[0]
        else:
            y = ops.conv3d(x, wp, want_stats=False)[0]
        return y[..., :cin].contiguous() if transposed and cin < 64 else y

    @staticmethod
    def forward(ctx, x, w, key=None, grad_channel=None):
        """grad_channel = c: only input channel c carries a gradient (the K-Net's first layer: 15 of its 16 input channels are warped
        images, KVNET.py:163-166) — the data gradient is then ONE output channel, a 27-tap stencil over gy on conv3d.hip's depth-marching
        kernel instead of a 64 -> 64 Winograd launch of which 63 output channels would be discarded."""
        x = x.contiguous()
        fwd = bwd = None
        ctx.grad_channel = grad_channel
        if w.shape[0] == 64 and w.shape[1] == 64 and ctx.needs_input_grad[0]:
            ctx.kind = ops.conv3d_kernel(*x.shape, 64, Conv3dCL.kernels)
            if ctx.kind != "direct":
                # both weight streams (forward + data gradient) in one launch: the weights changed since the last iteration anyway
                both = _cached(key, ("both3", ctx.kind), lambda: ops.conv_wino_pack_both(w, dw={"dw4": 4, "dw": 2, "pc": 0}[ctx.kind]))
                fwd, bwd = (ctx.kind, both[0]), both[1]
        y = Conv3dCL._conv(x, w, packed=fwd, key=key)
        ctx.save_for_backward(x, w, bwd)
        ctx.key = key
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, bwd = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[1]:
            gw = ops.conv3d_wgrad(x.contiguous(), gy)
            if gw.shape[1] != w.shape[1]:                             # x zero-padded: the padded rows are dropped, never stored
                gw = gw[:, :w.shape[1]].contiguous()
        if ctx.needs_input_grad[0]:
            c = ctx.grad_channel
            if c is not None and w.shape[0] == 64:
                # gx[v][c] = sum_co sum_tap gy[v - off(tap)][co] w[co][c][tap]: the 64 -> 1 kernel on gy with the taps mirrored
                w_tm = _cached(ctx.key, ("c1t", c), lambda: w.detach()[:, c].reshape(64, 27).flip(1).t().contiguous())
                gx = gy.new_zeros(gy.shape[:3] + (x.shape[-1],))
                gx[..., c] = ops.conv3d_cout1(gy, w_tm)
            else:
                gx = Conv3dCL._conv(gy, w, transposed=True, packed=None if bwd is None else (ctx.kind, bwd), key=ctx.key)
                if gx.shape[-1] != x.shape[-1]:                       # x zero-padded: the padding carries no gradient
                    gx = torch.cat((gx, gx.new_zeros(gx.shape[:3] + (x.shape[-1] - gx.shape[-1],))), dim=-1)
        return gx, gw, None, None


class Conv3dCout1CL(torch.autograd.Function):
    """The K-Net's last layer Conv3d(64, 1, 3, padding 1, no bias; models/basic.py:92-94) on a channels-last activation, all three
    directions as memory-bound 27-tap stencils: forward = csrc/conv3d.hip's depth-marching kernel, data and weight gradient =
    csrc/conv3d_c1_bwd.hip (until round 6: the layer zero-padded to 64 outputs on three 64 -> 64 matrix-core launches).

    x [D,H,W,64], w [1,64,3,3,3] -> y [D,H,W]."""

    @staticmethod
    def forward(ctx, x, w, key=None):
        x = x.contiguous()
        w_tm = _cached(key, ("c1", 0), lambda: w.detach()[0].reshape(64, 27).t().contiguous())    # [27, 64] tap-major
        ctx.save_for_backward(x, w_tm)
        return ops.conv3d_cout1(x, w_tm)

    @staticmethod
    def backward(ctx, gy):
        x, w_tm = ctx.saved_tensors
        gy = gy.contiguous()
        gx = ops.conv3d_cout1_dgrad(gy, w_tm) if ctx.needs_input_grad[0] else None
        gw = ops.conv3d_cout1_wgrad(x, gy) if ctx.needs_input_grad[1] else None
        return gx, gw, None


class BatchNormActCL(torch.autograd.Function):
    """y = act(batch_norm(x)) + residual on a channels-last tensor x [..., C] (batch statistics over every leading axis), forward
    and backward on csrc/bn_train.hip — nn.BatchNorm2d / nn.BatchNorm3d + ReLU + residual add of models/psm_submodule.py:10-16,31-50
    and models/basic.py:53-68,71-94 in training.  The running statistics (if any) are updated by the forward kernel."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, eps, relu, momentum, running_mean, running_var):
        C = x.shape[-1]
        x2 = x.contiguous().view(-1, C)
        r2 = None if residual is None else residual.contiguous().view(-1, C)
        y, coef = ops.bn_cl_fwd(x2, weight, bias, eps, relu, r2, momentum, running_mean, running_var)
        ctx.save_for_backward(x2, coef)
        ctx.relu = relu
        ctx.has_res = residual is not None
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        x2, coef = ctx.saved_tensors
        gy2 = gy.contiguous().view(x2.shape)
        gx, gg, gb = ops.bn_cl_bwd(x2, gy2, coef, ctx.relu)
        return gx.view(gy.shape), gg, gb, (gy if ctx.has_res else None), None, None, None, None, None


def batch_norm_act_cl(x_cl, bn, relu, residual=None):
    """nn.BatchNorm{2,3}d `bn` (+ ReLU, + residual) applied to the channels-last tensor x_cl [..., C] under autograd.
    Batch statistics (train mode, or a norm without running statistics: every norm of the reference as it is run):
    csrc/bn_train.hip in both directions.  Running statistics (a model the caller switched to eval()): the norm is the per-channel
    affine map x * s + t with s = gamma / sqrt(running_var + eps) — elementwise tensor arithmetic, differentiable as it is.
    On the GPU there is no other route: a channel count bn_train.hip has no form for raises NrgbdError (never F.batch_norm, i.e.
    MIOpen — ADVICE r5).  CPU tensors (host-side structure tests) go through torch.nn.functional."""
    import torch.nn.functional as F
    C = x_cl.shape[-1]
    from .nets import _bn_batch_args, _bn_eval_affine
    use_batch = bn.training or not bn.track_running_stats
    m, rm, rv, _ = _bn_batch_args(bn, host_counter=True)      # csrc/bn_train.hip takes no counter: bumped on the host
    on_gpu = x_cl.is_cuda and x_cl.dtype == torch.float32
    if on_gpu and use_batch:
        if not (bn.affine and ops.bn_cl_supported(x_cl.numel() // C, C)):
            from ._lib import NrgbdError
            raise NrgbdError("no hand-written kernel for a batch-statistics BatchNorm over %d channels (affine=%s): csrc/bn_train.hip "
                             "covers C %% 4 == 0 with C / 4 dividing 256" % (C, bn.affine))
        if x_cl.numel() // C <= 1:      # nn.BatchNorm's own refusal (torch/nn/functional.py::_verify_batch_size)
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x_cl.shape),))
        return BatchNormActCL.apply(x_cl, bn.weight, bn.bias, residual, bn.eps, relu, m, rm, rv)
    if on_gpu:                          # eval(): the affine map of the running statistics
        s_, t_ = _bn_eval_affine(bn, detach=False)
        y = x_cl * s_ + t_
    else:
        y = F.batch_norm(x_cl.reshape(-1, C), bn.running_mean if bn.track_running_stats else None,
                         bn.running_var if bn.track_running_stats else None, bn.weight, bn.bias, use_batch, m, bn.eps).view_as(x_cl)
    if relu:
        y = torch.relu(y)
    return y if residual is None else y + residual


class BiasLeakyReLUCL(torch.autograd.Function):
    """y = leaky_relu(x + bias[c], slope) for an NCHW tensor in channels_last memory (the R-Net's conv2d_leakyRelu /
    conv2dTranspose_leakyRelu tails, models/m_submodule.py:18-27,36-45; slope = 1: a plain bias), forward and backward in one
    pass each on csrc/bn_train.hip."""

    @staticmethod
    def forward(ctx, x, bias, slope):
        x_cl = x.permute(0, 2, 3, 1).contiguous()
        C = x_cl.shape[-1]
        y = ops.bias_lrelu_cl_fwd(x_cl.view(-1, C), bias, slope)
        ctx.save_for_backward(y)
        ctx.slope = slope
        ctx.shape = x_cl.shape
        return y.view(x_cl.shape).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        y, = ctx.saved_tensors
        C = y.shape[-1]
        gx, gb = ops.bias_lrelu_cl_bwd(y, gy.permute(0, 2, 3, 1).contiguous().view(-1, C), ctx.slope)
        return gx.view(ctx.shape).permute(0, 3, 1, 2), gb, None


def _bias_act(y, bias, slope):
    """+ bias, then LeakyReLU(slope) if slope is given: fused when there is a bias and the tensor is on the device."""
    if bias is not None and y.is_cuda and y.dtype == torch.float32 and y.shape[1] % 4 == 0 and y.shape[1] <= 1024:
        return BiasLeakyReLUCL.apply(y, bias, 1.0 if slope is None else float(slope))
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    return y if slope is None else torch.nn.functional.leaky_relu(y, slope)


class UpsampleBilinearCL(torch.autograd.Function):
    """F.upsample(bilinear, align_corners=True) of the tiny SPP maps (models/psm_submodule.py:153-158) under autograd, both
    directions on csrc/spp.hip.  x is an NCHW tensor (channels_last memory: the NHWC view is free); so is the result."""

    @staticmethod
    def forward(ctx, x, H, W):
        x_cl = x.permute(0, 2, 3, 1).contiguous()
        ctx.in_size = (x.shape[2], x.shape[3])
        return ops.upsample_bilinear_ac(x_cl, H, W).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        gy_cl = gy.permute(0, 2, 3, 1).contiguous()
        return ops.upsample_bilinear_ac(gy_cl, ctx.in_size[0], ctx.in_size[1], backward=True).permute(0, 3, 1, 2), None, None


class Conv2dCL(torch.autograd.Function):
    """3x3 convolution (stride 1, padding = dilation, no bias) of the feature CNN / R-Net under autograd, all three directions
    on the hand-written matrix-core kernels (models/psm_submodule.py:10-16, models/m_submodule.py:18-27 in training,
    train_utils/train_KVNet.py:103-153):
        forward        csrc/wino_pc.hip (Winograd domain; Cin % 32 == 0, Cout % 64 == 0) or csrc/conv2d.hip (direct)
        data gradient  the same kernels on the output gradient with the transposed + flipped weights
        weight grad.   csrc/conv2d_wgrad.hip
    x is an NCHW tensor, ideally in channels_last memory format (then the NHWC views the kernels work on are free); the result
    is an NCHW view of channels-last memory, so a trunk built from this op stays in that format.
    """

    DIRECT = {(32, 1), (64, 1), (96, 1), (128, 1), (128, 2)}    # (Cout, dilation) instantiated in conv2d.hip
    rnet_route = True    # False: the direct kernel for those widths (A/B, tools/)

    @staticmethod
    def _rnet_plan(cin, cout, dil, real_cout=None):
        """How wino_pc.hip's R-Net form (any stage count >= 2) covers a cin -> cout layer whose output width is not a multiple of 64 —
        the R-Net's 96-wide half-resolution and 67-wide (80 with padding) full-resolution layers, models/Refine.py:51-77 — instead of
        the direct kernel at 9 multiplies per output: (columns on whole 64-column groups, tail) with tail = ("half", n <= 32 columns on
        the kernel's 32-column form) | ("few", n <= 4 columns on csrc/conv_few.hip) | None; None if it does not apply.
        real_cout: output channels that are not zero padding (the padded columns are never computed: they stay zero)."""
        if not Conv2dCL.rnet_route:
            return None
        rc = cout if real_cout is None else min(real_cout, cout)
        full = (rc // 64) * 64
        extra = rc - full
        if dil != 1 or cin % 16 or cin < 32 or full == 0 or (cin % 32 == 0 and cout % 64 == 0):
            return None
        if extra == 0:
            return (full, None)
        if extra <= 4:
            return (full, ("few", extra))
        if extra <= 32 and cout >= full + extra:
            return (full, ("half", extra))
        return None

    @staticmethod
    def eligible(cin, cout, dil, need_dgrad=True, real=None):
        """Forward, data gradient (roles of Cin / Cout swapped; not needed when the input is an image) and weight gradient all
        have a kernel.  real = (cin, cout) before zero padding."""
        rci, rco = real if real is not None else (cin, cout)

        def fwd(ci, co, rc):
            return ((ci % 32 == 0 and co % 64 == 0 and dil in (1, 2)) or Conv2dCL._rnet_plan(ci, co, dil, rc) is not None
                    or (ci % 16 == 0 and (co, dil) in Conv2dCL.DIRECT))
        return fwd(cin, cout, rco) and (fwd(cout, cin, rci) or not need_dgrad) and cin % 16 == 0 and cout % 16 == 0

    @staticmethod
    def _conv(x_cl, w, dil, transposed=False, packed=None, key=None, real_out=None):
        cout, cin = (w.shape[1], w.shape[0]) if transposed else w.shape[:2]
        tr = bool(transposed)
        if cin % 32 == 0 and cout % 64 == 0:
            wp = packed if packed is not None else _cached(key, ("pc", tr), lambda: ops.conv_wino_pack(w, transposed))
            return ops.conv_wino(x_cl, wp, cout, 1, dil, want_stats=False)[0]
        if cout == 32 and cin % 32 == 0 and dil == 1 and ops.conv_wino_supported(x_cl.shape[0], x_cl.shape[1], x_cl.shape[2], cin, 32, 1):
            # the HALF form of wino_pc.hip (the trunk's 32 -> 32 layers): its stream is the 64-column one, upper half zero
            wp = _cached(key, ("half", tr), lambda: ops.conv_wino_pack(torch.cat((w, torch.zeros_like(w)), 1 if transposed else 0), transposed))
            return ops.conv_wino(x_cl, wp, 32, 1, 1, want_stats=False)[0]
        plan = Conv2dCL._rnet_plan(cin, cout, dil, real_out)
        if plan is not None:
            full, tail = plan

            def we():                                             # the weights as a forward layer [cout, cin, 3, 3] of THIS call
                return (w.detach().transpose(0, 1).flip(2, 3) if transposed else w.detach())
            done = full + (tail[1] if tail else 0)
            out = (x_cl.new_zeros if done < cout else x_cl.new_empty)(x_cl.shape[:3] + (cout,))     # padding columns: exactly zero
            ops.conv_wino_rnet(x_cl, _cached(key, ("rg", tr), lambda: ops.conv_wino_pack(we()[:full].contiguous())), full, None, False,
                               out=out, ycoff=0, cout_valid=full)
            if tail is not None and tail[0] == "few":
                n = tail[1]
                wf = _cached(key, ("rf", tr), lambda: we()[full:full + n].reshape(n, cin // 16, 16, 9).permute(1, 3, 0, 2).contiguous())
                ops.conv2d_few(x_cl, wf, None, False, out=out, ycoff=full)
            elif tail is not None:
                n = tail[1]
                th = _cached(key, ("rh", tr), lambda: ops.conv_wino_pack(torch.cat((we()[full:full + n], w.new_zeros(64 - n, cin, 3, 3)), 0).contiguous()))
                ops.conv_wino_rnet(x_cl, th, 32, None, False, out=out, ycoff=full, cout_valid=n)
            return out

        def direct():
            return ops.conv_pack_weights((w.transpose(0, 1).flip(2, 3) if transposed else w).contiguous())   # transposed: [Cin, Cout, 3, 3], flipped
        return ops.conv2d(x_cl, _cached(key, ("direct", tr), direct), cout, dil, want_stats=False)[0]

    @staticmethod
    def forward(ctx, x, w, dil, key=None, real=None):
        """real = (cin, cout) of the layer before the caller's zero padding (None: w's own widths)."""
        x_cl = x.permute(0, 2, 3, 1).contiguous()                 # free when x is channels_last
        cout, cin = w.shape[:2]
        fwd = bwd = None
        if cin % 64 == 0 and cout % 64 == 0 and ctx.needs_input_grad[0]:
            # both directions run on wino_pc.hip: one packing launch for the two streams
            fwd, bwd = _cached(key, ("both", 0), lambda: ops.conv_wino_pack_both(w))
        y = Conv2dCL._conv(x_cl, w, dil, packed=fwd, key=key, real_out=None if real is None else real[1])
        ctx.save_for_backward(x_cl, w, bwd)
        ctx.dil, ctx.key, ctx.real = dil, key, real
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        x_cl, w, bwd = ctx.saved_tensors
        gy_cl = gy.permute(0, 2, 3, 1).contiguous()
        gx = gw = None
        if ctx.needs_input_grad[1]:
            gw = ops.conv2d_wgrad(x_cl, gy_cl, ctx.dil)
        if ctx.needs_input_grad[0]:
            gx = Conv2dCL._conv(gy_cl, w, ctx.dil, transposed=True, packed=bwd, key=ctx.key,
                                real_out=None if ctx.real is None else ctx.real[0]).permute(0, 3, 1, 2)
        return gx, gw, None, None, None


def _padded_widths(cin, cout, dil, need_dgrad, real=None):
    """Smallest (cin_p, cout_p) >= (cin, cout), multiples of 16, for which Conv2dCL has every kernel it will need.
    real: the layer's own (cin, cout) when `cin` already counts padding channels of the incoming tensor."""
    real = (cin, cout) if real is None else real
    best = None
    for co in range(-(-cout // 16) * 16, cout + 129, 16):
        for ci in range(-(-cin // 16) * 16, cin + 129, 16):
            if Conv2dCL.eligible(ci, co, dil, need_dgrad, real) and (best is None or ci * co < best[0] * best[1]):
                best = (ci, co)
    return best


# stride-2 3x3 (padding 1) on the space-to-depth input: y[Y] = sum_ky w[ky] x[2Y + ky - 1]; with x2[Yp, py] = x[2Yp + py] the three
# taps are (Yp = Y - 1, py = 1), (Y, 0), (Y, 1): a 3x3 stride-1 kernel on x2 whose row r = dy + 1 and parity py select tap
# _S2_TAP[r][py] (-1: no such tap).  Same along x.
_S2_TAP = ((-1, 0), (1, 2), (-1, -1))
# ConvTranspose2d(k4, s2, p1): output row 2Y + a collects input rows Y + dy with kernel row ky = a + 1 - 2 dy:
# a = 0: (dy -1 -> 3), (0 -> 1);  a = 1: (0 -> 2), (+1 -> 0).  _T2_TAP[a][r = dy + 1]
_T2_TAP = ((3, 1, -1), (-1, 2, 0))
_index_cache = {}


def _tap_select(kind, device):
    """(flat source index, mask) that turn a flattened kernel into its embedded 3x3 form with ONE index_select (no GEMM: an
    einsum with the 0/1 selection tensors would run on rocBLAS)."""
    key = (kind, str(device))
    hit = _index_cache.get(key)
    if hit is None:
        if kind == "s2":        # target [py, px, r, c] <- source [ky, kx] (3x3)
            idx = torch.zeros(2, 2, 3, 3, dtype=torch.long)
            msk = torch.zeros(2, 2, 3, 3)
            for py in range(2):
                for px in range(2):
                    for r in range(3):
                        for c in range(3):
                            ky, kx = _S2_TAP[r][py], _S2_TAP[c][px]
                            if ky >= 0 and kx >= 0:
                                idx[py, px, r, c] = ky * 3 + kx
                                msk[py, px, r, c] = 1.0
        else:                   # "t2": target [a, b, r, c] <- source [ky, kx] (4x4)
            idx = torch.zeros(2, 2, 3, 3, dtype=torch.long)
            msk = torch.zeros(2, 2, 3, 3)
            for a_ in range(2):
                for b_ in range(2):
                    for r in range(3):
                        for c in range(3):
                            ky, kx = _T2_TAP[a_][r], _T2_TAP[b_][c]
                            if ky >= 0 and kx >= 0:
                                idx[a_, b_, r, c] = ky * 4 + kx
                                msk[a_, b_, r, c] = 1.0
        hit = (idx.reshape(-1).to(device), msk.reshape(-1).to(device))
        _index_cache[key] = hit
    return hit


def _conv3x3_cl(x, w, dil, bias, keep_width=False, act_slope=None, key=None):
    """3x3 stride-1 convolution through Conv2dCL, the channel counts zero-padded to widths the kernels have (67 -> 96 for the
    R-Net's full-resolution layers, 12 -> 16 for the space-to-depth image).  None if no width fits.
    x may already carry MORE channels than w reads (the padded output of the previous layer: its extra channels are zero).
    keep_width: return the padded output [N, cout_p, H, W] (extra channels exactly zero when the bias is added here: its
    padding is zero too) instead of a channel slice — the next layer then reads it as is."""
    F = torch.nn.functional
    cout, cin = w.shape[:2]
    have = x.shape[1]
    pw = _padded_widths(max(cin, have), cout, dil, x.requires_grad, real=(cin, cout))
    if pw is None:
        return None
    ci, co = pw
    if ci != have:
        x = F.pad(x, (0, 0, 0, 0, 0, ci - have))
    if ci != cin:
        w = F.pad(w, (0, 0, 0, 0, 0, ci - cin))
    if co != cout:
        w = F.pad(w, (0, 0, 0, 0, 0, 0, 0, co - cout))
    y = Conv2dCL.apply(x, w, dil, key, (cin, cout))
    # bias (+ LeakyReLU) on the full-width channels-last tensor (the padded channels stay exactly zero: zero weights, zero bias)
    y = _bias_act(y, None if bias is None else (bias if co == cout else F.pad(bias, (0, co - cout))), act_slope)
    if co != cout and not keep_width:
        y = y[:, :cout]
    return y


def conv2d_module(conv, x, _any_device=False, keep_width=False, act_slope=None):
    """nn.Conv2d forward for the module (autograd) paths, on the hand-written kernels in all three directions:
      * 3x3, stride 1, padding = dilation: Conv2dCL (channels zero-padded to a width the kernels have when needed: the R-Net's
        67-channel layers run as 96-wide ones);
      * 1x1 (stride 1 or 2, the trunk's shortcut / SPP / last layers, psm_submodule.py:90-139): the (strided) input through the
        same op with the weight as the centre tap of a 3x3 kernel;
      * 3x3, stride 2, padding 1 (firstconv, layer2: psm_submodule.py:90-99): space-to-depth (pixel_unshuffle) + the 3x3 kernel
        that holds the 2x2 window of the stride-2 taps (`_S2_TAP`).
    The weight embeddings are index / pad operations of torch, so autograd maps the weight gradient back by itself.
    (_any_device: the CPU test of the embeddings, tests/test_host.py, which substitutes F.conv2d for Conv2dCL.)
    Shapes none of this covers (other strides / kernel sizes, groups; none occurs in the path's networks) raise NrgbdError on the
    GPU — there is no vendor-library route; on the CPU (host-side structure tests, float64 reference graphs) they are the module's own forward."""
    F = torch.nn.functional
    k, st, pd, d = conv.kernel_size, conv.stride, conv.padding, conv.dilation

    def module_forward():
        if x.is_cuda and x.dtype == torch.float32:
            raise _lib.NrgbdError("no hand-written kernel for Conv2d(%d, %d, kernel %s, stride %s, padding %s, dilation %s, groups %d) on a %s input"
                                  % (conv.in_channels, conv.out_channels, k, st, pd, d, conv.groups, tuple(x.shape)))
        return _bias_act(conv(x[:, :conv.in_channels] if x.shape[1] != conv.in_channels else x), None, act_slope)
    if not ((x.is_cuda or _any_device) and x.dtype == torch.float32 and conv.groups == 1 and k[0] == k[1] and st[0] == st[1] and d[0] == d[1]
            and pd[0] == pd[1] and conv.padding_mode == "zeros"):
        return module_forward()
    w, y = conv.weight, None
    if k == (3, 3) and st == (1, 1) and pd == d:
        y = _conv3x3_cl(x, w, d[0], conv.bias, keep_width, act_slope, key=id(conv.weight))
    elif k == (1, 1) and pd == (0, 0) and st[0] in (1, 2):
        xs = x if st[0] == 1 else x[:, :, ::2, ::2]
        y = _conv3x3_cl(xs, F.pad(w, (1, 1, 1, 1)), 1, conv.bias, False, act_slope, key=id(conv.weight))
    elif k == (3, 3) and st == (2, 2) and pd == (1, 1) and d == (1, 1) and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0:
        idx, msk = _tap_select("s2", w.device)
        cout, cin = w.shape[:2]
        # pixel_unshuffle orders its channels c * 4 + py * 2 + px
        w2 = (w.reshape(cout, cin, 9).index_select(2, idx) * msk).reshape(cout, cin * 4, 3, 3)
        y = _conv3x3_cl(F.pixel_unshuffle(x, 2), w2, 1, conv.bias, False, act_slope, key=id(conv.weight))
    if y is None:
        return module_forward()
    return y


def conv_transpose2d_module(conv, x, _any_device=False, act_slope=None):
    """nn.ConvTranspose2d(kernel 4, stride 2, padding 1) of the R-Net (models/Refine.py:51-77, m_submodule.py:36-45) under autograd
    on the hand-written kernels: its four sub-pixel phases are 2x2-tap convolutions of the input (`_T2_TAP`); embedded in 3x3
    kernels and stacked along the output channels (4 Cout, ordered co * 4 + a * 2 + b) they are ONE Conv2dCL launch per direction,
    and pixel_shuffle interleaves the phases."""
    F = torch.nn.functional

    def module_forward():
        if x.is_cuda and x.dtype == torch.float32:
            raise _lib.NrgbdError("no hand-written kernel for this ConvTranspose2d (%d -> %d, kernel %s, stride %s) on a %s input"
                                  % (conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, tuple(x.shape)))
        return _bias_act(conv(x), None, act_slope)
    if not ((x.is_cuda or _any_device) and x.dtype == torch.float32 and conv.groups == 1 and conv.kernel_size == (4, 4) and conv.stride == (2, 2)
            and conv.padding == (1, 1) and conv.output_padding == (0, 0) and conv.dilation == (1, 1)):
        return module_forward()
    w = conv.weight                                  # [Cin, Cout, 4, 4]
    cin, cout = w.shape[:2]
    idx, msk = _tap_select("t2", w.device)
    w4 = (w.permute(1, 0, 2, 3).reshape(cout, cin, 16).index_select(2, idx) * msk)       # [Cout, Cin, (a, b, r, c)]
    w4 = w4.reshape(cout, cin, 4, 9).permute(2, 0, 1, 3).reshape(4 * cout, cin, 3, 3)   # rows (a * 2 + b) * Cout + co: phase-major
    # bias + LeakyReLU commute with the interleave: applied to the four phases at once BEFORE it, on the channels-last tensor
    # the convolution wrote
    b4 = None if conv.bias is None else conv.bias.repeat(4)
    y = _conv3x3_cl(x, w4, 1, b4, False, act_slope, key=id(conv.weight))
    if y is None:
        return module_forward()
    # sub-pixel interleave on the channels-last tensor: pixel (Y, X) holds its four output pixels as four runs of Cout channels,
    # so ONE copy of 4 Cout-float runs builds the channels-last result (F.pixel_shuffle would gather single floats into a planar
    # tensor that the next layer converts back)
    N, _, H, W = y.shape
    out = y.permute(0, 2, 3, 1).reshape(N, H, W, 2, 2, cout).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, cout)
    return out.permute(0, 3, 1, 2)


def padded_in_width(conv, need_dgrad=True):
    """Input width Conv2dCL runs a 3x3 stride-1 module at (its channel count zero-padded to a width the kernels have)."""
    pw = _padded_widths(conv.in_channels, conv.out_channels, conv.dilation[0], need_dgrad)
    return conv.in_channels if pw is None else pw[0]


def cat_cl(tensors, width=None):
    """torch.cat(tensors, dim=1) built in channels-last memory, optionally zero-padded to `width` channels: every operand is
    copied once, straight to its channel range of the [N, H, W, C] result (a planar cat of mixed layouts followed by F.pad and the
    convolution's own layout change were three full-resolution copies in front of the R-Net's 67-channel layer).  Returns the
    NCHW view."""
    parts = [t.permute(0, 2, 3, 1) for t in tensors]
    have = sum(t.shape[3] for t in parts)
    if width is not None and width > have and parts[0].is_cuda and parts[0].dtype == torch.float32:   # the padding serves Conv2dCL only
        parts.append(parts[0].new_zeros(parts[0].shape[:3] + (width - have,)))
    return torch.cat(parts, dim=3).permute(0, 3, 1, 2)


class LogSoftmaxD(torch.autograd.Function):
    """log_softmax over the depth axis of scale * a (+ b), planar volumes [..., D, h, w] with leading dimensions of size 1
    (models/basic.py:299-300: scale = -1; models/KVNET.py:172-173: a = K-Net gain, b = BV_predict), on softmax.hip in both directions."""

    @staticmethod
    def forward(ctx, a, b, scale):
        D = a.shape[-3]
        if a.numel() != D * a.shape[-2] * a.shape[-1]:
            raise ValueError("LogSoftmaxD: one volume per call, got %s" % (tuple(a.shape),))
        out = ops.logsoftmax_d(a.reshape(a.shape[-3:]), None if b is None else b.reshape(a.shape[-3:]), float(scale))
        ctx.save_for_backward(out)
        ctx.scale, ctx.shape = float(scale), a.shape
        return out.reshape(a.shape)

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        g = g.reshape(out.shape)
        ga = gb = None
        if ctx.needs_input_grad[0]:
            ga = ops.logsoftmax_d_bwd(out, g, ctx.scale).reshape(ctx.shape)
        if ctx.needs_input_grad[1]:
            gb = ga if (ga is not None and ctx.scale == 1.0) else ops.logsoftmax_d_bwd(out, g, 1.0).reshape(ctx.shape)
        return ga, gb, None


class LogSoftmaxCL(torch.autograd.Function):
    """F.log_softmax(x, dim=1) of an [N, C, H, W] tensor that lives in channels-last memory (the R-Net's last layer under autograd,
    models/Refine.py:104): rows kernel in both directions, the result stays an NCHW view of channels-last memory."""

    @staticmethod
    def supported(x):
        return x.dim() == 4 and x.shape[1] in (64, 128, 256) and x.is_cuda and x.dtype == torch.float32

    @staticmethod
    def forward(ctx, x):
        y = ops.logsoftmax_rows(x.permute(0, 2, 3, 1).contiguous(), inplace=False)
        ctx.save_for_backward(y)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return ops.logsoftmax_rows_bwd(y, g.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)


class NLLLossD(torch.autograd.Function):
    """F.nll_loss(logp [1, D, h, w], target [1, h, w], ignore_index) with mean reduction (train_utils/train_KVNet.py:103-120), in
    logp's own layout (planar, or the channels-last memory the R-Net writes): one gather + fixed-order reduction forward, one
    pass that writes the whole gradient backward."""

    @staticmethod
    def forward(ctx, logp, target, ignore_index):
        cl = logp.permute(0, 2, 3, 1).is_contiguous() and not logp.is_contiguous()
        vol = logp.permute(0, 2, 3, 1)[0] if cl else logp.contiguous()[0]
        stat = ops.nll_fwd(vol, target, ignore_index, cl)
        ctx.save_for_backward(target, stat)
        ctx.args = (int(ignore_index), tuple(vol.shape), cl)
        return stat[0].clone()

    @staticmethod
    def backward(ctx, g):
        target, stat = ctx.saved_tensors
        ignore_index, shape, cl = ctx.args
        gl = ops.nll_bwd(target, ignore_index, g.to(torch.float32), stat, shape, cl).unsqueeze(0)
        return (gl.permute(0, 3, 1, 2) if cl else gl), None, None


def nll_loss_d(logp, target, ignore_index=0):
    """F.nll_loss for one [1, D, h, w] log-probability volume on the hand-written kernels; anything else goes to ATen."""
    if logp.dim() == 4 and logp.shape[0] == 1 and logp.is_cuda and logp.dtype == torch.float32 and target.dtype == torch.int64:
        return NLLLossD.apply(logp, target, ignore_index)
    return torch.nn.functional.nll_loss(logp, target, ignore_index=ignore_index)
