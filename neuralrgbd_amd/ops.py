"""Typed torch-tensor wrappers over the C-ABI of libnrgbd_hip.so (include/nrgbd.h).

PyTorch is used here only for device memory and the current HIP stream; every function below
launches hand-written gfx950 kernels.  Inputs must be CUDA fp32 tensors — there is no CPU
path: a CPU tensor raises.
"""
import ctypes
import typing

import numpy as np
import torch

from . import _lib

DIST = {"L2": 0, "L1": 1}
GENERATION = {None: 0, "auto": 0, "gather": 1, "lds": 2, "quad": 3}   # kernel generations of nrgbd_costvol_fwd_gen


def _need(t, name, shape=None, strided=False):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise _lib.NrgbdError("%s is on %s: the plane-sweep path runs on the GPU only "
                              "(no CPU fallback)" % (name, t.device))
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t if (strided or t.is_contiguous()) else t.contiguous()


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def version():
    return _lib.load().nrgbd_version().decode()


def padded_channels(C):
    return (C + 3) // 4 * 4


def homography_terms(K, R, t):
    """K [3,3], R [V,3,3] (any strides with unit column stride), t [V,3] (any strides) -> (KR [V,3,3], Kt [V,3])
    in the reference's CPU summation order (nrgbd_homography_terms)."""
    K = _need(K, "K", (3, 3))
    R = _need(R, "R", strided=True)
    t = _need(t, "t", strided=True)
    V = R.shape[0]
    if tuple(R.shape) != (V, 3, 3) or tuple(t.shape) != (V, 3):
        raise ValueError("homography_terms: R %s / t %s, expected [V,3,3] / [V,3]" % (tuple(R.shape), tuple(t.shape)))
    if R.stride(2) != 1:
        R = R.contiguous()
    KR = torch.empty((V, 3, 3), dtype=torch.float32, device=K.device)
    Kt = torch.empty((V, 3), dtype=torch.float32, device=K.device)
    with torch.cuda.device(K.device):
        rc = _lib.load().nrgbd_homography_terms(_p(K), _p(R), R.stride(0), R.stride(1), _p(t), t.stride(0), t.stride(1),
                                                _p(KR), _p(Kt), V, _stream(K))
    _lib.check(rc, "nrgbd_homography_terms")
    return KR, Kt


def pose_inverse(T, singular_count=None):
    """T [...,4,4] fp32 on the GPU -> its inverse, same shape (nrgbd_pose_inverse: fp64 Gauss-Jordan in a fixed operation
    order, rounded to fp32; replaces `.inverse()` of test_utils/test_KVNet.py:50).  Capture-safe: no solver workspace,
    no host sync.  `singular_count`: optional int32 device scalar that counts singular inputs (their output is NaN)."""
    T = _need(T, "T")
    if T.dim() < 2 or tuple(T.shape[-2:]) != (4, 4):
        raise ValueError("pose_inverse: T %s, expected [...,4,4]" % (tuple(T.shape),))
    n = T.numel() // 16
    out = torch.empty_like(T)
    if singular_count is not None and (singular_count.dtype != torch.int32 or not singular_count.is_cuda):
        raise TypeError("singular_count must be an int32 CUDA tensor")
    with torch.cuda.device(T.device):
        rc = _lib.load().nrgbd_pose_inverse(_p(T), 16, _p(out), _p(singular_count), n, _stream(T))
    _lib.check(rc, "nrgbd_pose_inverse")
    return out


def pack_nhwc(feat, rgb=None, Cp=None, channels_last=False, want_rgb4=False):
    """feat [N,Cf,h,w] (or [N,h,w,Cf] if channels_last) (+ rgb [N,3,h*pool,w*pool]) -> texels [N,h,w,Cp] (nrgbd_pack_nhwc).
    want_rgb4: -> (texels, rgb4 [N,h,w,4]): the pooled-RGB word of every texel once more as a compact plane (the K-Net's warp)."""
    feat = _need(feat, "feat")
    if channels_last:
        N, h, w, Cf = feat.shape
    else:
        N, Cf, h, w = feat.shape
    pool = 1
    if rgb is not None:
        rgb = _need(rgb, "rgb")
        if rgb.shape[0] != N or rgb.shape[1] != 3 or rgb.shape[2] % h or rgb.shape[3] % w:
            raise ValueError("rgb %s does not pool onto feat %s" % (tuple(rgb.shape), tuple(feat.shape)))
        pool = rgb.shape[3] // w
        if rgb.shape[2] // h != pool:
            raise ValueError("anisotropic pooling is not supported")
    if Cp is None:
        Cp = padded_channels(Cf + (3 if rgb is not None else 0))
    out = torch.empty((N, h, w, Cp), dtype=torch.float32, device=feat.device)
    rgb4 = torch.empty((N, h, w, 4), dtype=torch.float32, device=feat.device) if want_rgb4 else None
    with torch.cuda.device(feat.device):
        rc = _lib.load().nrgbd_pack_nhwc(_p(feat), _p(rgb), _p(out), N, Cf, h, w, pool, Cp, int(bool(channels_last)),
                                          _p(rgb4), _stream(feat))
    _lib.check(rc, "nrgbd_pack_nhwc")
    return (out, rgb4) if want_rgb4 else out


def costvol(ref_nhwc, src_nhwc, KR, Kt, rays, d_candi, cx, cy, sigma, C, dist="L2",
            align_corners=False, want_cost=True, want_logp=False, generation=None):
    """Fused warp + cost volume (+ log-softmax).  Returns (cost [D,h,w] | None, logp [D,h,w] | None).
    `generation` (None = automatic | "gather" | "lds" | "quad") pins the kernel generation for tests / A-B timing
    (automatic = "quad" for the path's 64(+3)-channel texel; "quad4" = the same kernel with its per-view accumulators in LDS:
    bit-identical, every output written once, measured slower — profiles/r3_costvol_gen4.txt)."""
    src_nhwc = _need(src_nhwc, "src_nhwc")
    V, h, w, Cp = src_nhwc.shape
    ref_nhwc = _need(ref_nhwc, "ref_nhwc", (h, w, Cp))
    KR = _need(KR, "KR").reshape(V, 9)
    Kt = _need(Kt, "Kt", (V, 3))
    rays = _need(rays, "rays", (3, h * w))
    d_candi = _need(d_candi, "d_candi")
    D = d_candi.numel()
    dev = src_nhwc.device
    cost = torch.empty((D, h, w), dtype=torch.float32, device=dev) if want_cost else None
    logp = torch.empty((D, h, w), dtype=torch.float32, device=dev) if want_logp else None
    with torch.cuda.device(dev):
        rc = _lib.load().nrgbd_costvol_fwd_gen(_p(ref_nhwc), _p(src_nhwc), _p(KR), _p(Kt), _p(rays),
                                               _p(d_candi), float(cx), float(cy), float(sigma),
                                               DIST[dist], int(bool(align_corners)), _p(cost), _p(logp),
                                               V, int(C), Cp, D, h, w, GENERATION[generation], _stream(src_nhwc))
    _lib.check(rc, "nrgbd_costvol_fwd_gen")
    return cost, logp


def costvol_bwd(ref_nhwc, src_nhwc, KR, Kt, rays, d_candi, cx, cy, sigma, C, g_cost, dist="L2", align_corners=False,
                deterministic=False):
    """Gradient of the cost volume w.r.t. the packed features: (g_ref [h,w,Cp], g_src [V,h,w,Cp]).
    deterministic: csrc/costvol_bwd_det.hip (fixed-point scatter: the same bits on every run) instead of the atomic kernels of
    csrc/costvol_bwd.hip; both are within the same rounding bound of the exact gradient."""
    src_nhwc = _need(src_nhwc, "src_nhwc")
    V, h, w, Cp = src_nhwc.shape
    ref_nhwc = _need(ref_nhwc, "ref_nhwc", (h, w, Cp))
    d_candi = _need(d_candi, "d_candi")
    D = d_candi.numel()
    g_cost = _need(g_cost, "g_cost", (D, h, w))
    g_ref, g_src = torch.empty_like(ref_nhwc), torch.empty_like(src_nhwc)
    name = "nrgbd_costvol_bwd_det" if deterministic else "nrgbd_costvol_bwd"
    with torch.cuda.device(src_nhwc.device):
        nbytes = ctypes.c_size_t(0)
        _lib.check(getattr(_lib.load(), name + "_workspace")(V, Cp, D, h, w, ctypes.byref(nbytes)), name + "_workspace")
        work = torch.empty(nbytes.value, dtype=torch.uint8, device=src_nhwc.device) if nbytes.value else None
        rc = getattr(_lib.load(), name)(_p(ref_nhwc), _p(src_nhwc), _p(_need(KR, "KR").reshape(V, 9)), _p(_need(Kt, "Kt", (V, 3))),
                                        _p(_need(rays, "rays", (3, h * w))), _p(d_candi), float(cx), float(cy), float(sigma),
                                        DIST[dist], int(bool(align_corners)), _p(g_cost), _p(g_ref), _p(g_src),
                                        V, int(C), Cp, D, h, w, _p(work) if work is not None else None, nbytes.value,
                                        _stream(src_nhwc))
    _lib.check(rc, name)
    return g_ref, g_src


def warp_volume(src, src_strides, ref, ref_strides, KR, Kt, rays, d_candi, cx, cy, V, Cs, h, w,
                bv_cur=None, bv_pred=None, align_corners=False, channels_last=False, pad_channels=None):
    """Plane-sweep warp with samples kept (+ K-Net input assembly) -> [V*Cs (+Cs) (+1), D, h, w]
    (or [D, h, w, channels] with channels_last=True, the layout conv3d consumes).
    pad_channels = Cp (channels_last with ref and bv only): the voxel is Cp floats wide, zeros behind the assembly — the K-Net input
    of any temporal window at whole 16-channel blocks.  V = 4 at Cp = 16 is nrgbd_warp_volume's own fast form; every other
    window goes to nrgbd_warp_volume_cl.

    `src` / `ref` are any CUDA fp32 tensors; `src_strides` = (view, channel, y, x) and
    `ref_strides` = (channel, y, x) element strides from their data pointers.
    """
    src = _need(src, "src", strided=True)  # addressed through src_strides
    KR = _need(KR, "KR").reshape(V, 9)
    Kt = _need(Kt, "Kt", (V, 3))
    rays = _need(rays, "rays", (3, h * w))
    d_candi = _need(d_candi, "d_candi")
    D = d_candi.numel()
    n_ch = V * Cs
    if ref is not None:
        ref = _need(ref, "ref", strided=True)
        n_ch += Cs
    else:
        ref_strides = (0, 0, 0)
    if bv_cur is not None:
        bv_cur = _need(bv_cur, "bv_cur").reshape(D, h, w)
        bv_pred = _need(bv_pred, "bv_pred").reshape(D, h, w)
        n_ch += 1
    if pad_channels is not None and int(pad_channels) != n_ch:
        if not channels_last or ref is None or bv_cur is None or pad_channels < n_ch or pad_channels % 4:
            raise ValueError("warp_volume: pad_channels = %r needs channels_last, ref and bv_cur, a multiple of 4 >= %d" % (pad_channels, n_ch))
        out = torch.empty((D, h, w, int(pad_channels)), dtype=torch.float32, device=src.device)
        with torch.cuda.device(src.device):
            rc = _lib.load().nrgbd_warp_volume_cl(_p(src), *[int(s) for s in src_strides], _p(ref),
                                                  *[int(s) for s in ref_strides], _p(KR), _p(Kt), _p(rays),
                                                  _p(d_candi), float(cx), float(cy), int(bool(align_corners)),
                                                  _p(bv_cur), _p(bv_pred), _p(out), V, Cs, int(pad_channels), D, h, w, _stream(src))
        _lib.check(rc, "nrgbd_warp_volume_cl")
        return out
    shape = (D, h, w, n_ch) if channels_last else (n_ch, D, h, w)
    out = torch.empty(shape, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        rc = _lib.load().nrgbd_warp_volume(_p(src), *[int(s) for s in src_strides], _p(ref),
                                           *[int(s) for s in ref_strides], _p(KR), _p(Kt), _p(rays),
                                           _p(d_candi), float(cx), float(cy), int(bool(align_corners)),
                                           _p(bv_cur), _p(bv_pred), _p(out), V, Cs, D, h, w,
                                           int(bool(channels_last)), _stream(src))
    _lib.check(rc, "nrgbd_warp_volume")
    return out


def dpv_resample(dpv, T, rays, d_candi, tan_hh, tan_hv, z_half, z_radius, pad_value, clamp=(-1000.0, 0.0),
                 new_candi=False):
    """PREDICT: dpv [D,h,w], T [4,4] (device) -> resampled [len(d_candi),h,w].  `d_candi` = the depths of the OUTPUT planes
    (= the source's unless new_candi: resample_vol_cuda's d_candi_new form, nrgbd_dpv_resample_to)."""
    dpv = _need(dpv, "dpv")
    D, h, w = dpv.shape
    T = _need(T, "T").reshape(16)
    rays = _need(rays, "rays", (3, h * w))
    d_candi = _need(d_candi, "d_candi") if new_candi else _need(d_candi, "d_candi", (D,))
    if d_candi.dim() != 1:
        raise ValueError("d_candi must be 1-D")
    Do = d_candi.shape[0]
    out = torch.empty((Do, h, w), dtype=torch.float32, device=dpv.device)
    lo, hi = clamp if clamp is not None else (0.0, 0.0)
    with torch.cuda.device(dpv.device):
        rc = _lib.load().nrgbd_dpv_resample_to(_p(dpv), _p(T), _p(rays), _p(d_candi), float(tan_hh),
                                               float(tan_hv), float(z_half), float(z_radius),
                                               float(pad_value), int(clamp is not None), float(lo),
                                               float(hi), _p(out), D, Do, h, w, _stream(dpv))
    _lib.check(rc, "nrgbd_dpv_resample_to")
    return out


def dpv_keyframe_maps(dpv, T, rays, d_candi_out, d_candi_src, tan_hh, tan_hv, z_half, z_radius, pad_value,
                      clamp=(-1000.0, 0.0), want_ref=True, out=None):
    """dpv [D,h,w] log-DPV, T [4,4] (device) -> (dmap_ref, conf_ref, dmap_kf, conf_kf), each [h,w], in one launch
    (nrgbd_dpv_keyframe_maps): the keyframe pair is the expected depth and exp(max)^2 of the volume dpv_resample(...,
    new_candi=True) would return for d_candi_out, which is never written; the reference pair the same of dpv itself with
    d_candi_src [D].  want_ref=False: the reference pair is not computed (returned as None, or left untouched in `out`).
    `out`: the four maps of an earlier call to write into (a captured graph's static buffers)."""
    dpv = _need(dpv, "dpv")
    if dpv.dim() != 3:
        raise ValueError("dpv %s, expected [D,h,w]" % (tuple(dpv.shape),))
    D, h, w = dpv.shape
    T = _need(T, "T").reshape(16)
    rays = _need(rays, "rays", (3, h * w))
    d_candi_out = _need(d_candi_out, "d_candi_out")
    if d_candi_out.dim() != 1:
        raise ValueError("d_candi_out must be 1-D")
    d_candi_src = _need(d_candi_src, "d_candi_src", (D,)) if want_ref else None
    if out is None:
        new = lambda: torch.empty((h, w), dtype=torch.float32, device=dpv.device)
        out = (new() if want_ref else None, new() if want_ref else None, new(), new())
    dmap_ref, conf_ref, dmap_kf, conf_kf = out
    for name, t in (("dmap_kf", dmap_kf), ("conf_kf", conf_kf)) + ((("dmap_ref", dmap_ref), ("conf_ref", conf_ref)) if want_ref else ()):
        if _need(t, name, (h, w)) is not t:
            raise ValueError("%s must be contiguous" % name)
    lo, hi = clamp if clamp is not None else (0.0, 0.0)
    with torch.cuda.device(dpv.device):
        rc = _lib.load().nrgbd_dpv_keyframe_maps(_p(dpv), _p(T), _p(rays), _p(d_candi_out), _p(d_candi_src), float(tan_hh),
                                                 float(tan_hv), float(z_half), float(z_radius), float(pad_value),
                                                 int(clamp is not None), float(lo), float(hi), _p(dmap_kf), _p(conf_kf),
                                                 _p(dmap_ref if want_ref else None), _p(conf_ref if want_ref else None),
                                                 D, d_candi_out.shape[0], h, w, _stream(dpv))
    _lib.check(rc, "nrgbd_dpv_keyframe_maps")
    return dmap_ref, conf_ref, dmap_kf, conf_kf


def logsoftmax_d(a, b=None, scale=1.0):
    """log_softmax over dim 0 of scale*a (+ b); a, b [D, ...]."""
    a = _need(a, "a")
    D = a.shape[0]
    n = a.numel() // D
    if b is not None:
        b = _need(b, "b", a.shape)
    out = torch.empty_like(a)
    with torch.cuda.device(a.device):
        rc = _lib.load().nrgbd_logsoftmax_d(_p(a), _p(b), float(scale), _p(out), D, n, _stream(a))
    _lib.check(rc, "nrgbd_logsoftmax_d")
    return out


def is_channels_last_view(logp):
    """A [D, ...] volume that is a VIEW of contiguous channels-last memory [..., D] (what the R-Net's last layer hands out):
    the `channels_last=True` form of depth_regress / export_depth_u16 reads it where it lies."""
    return logp.dim() >= 2 and not logp.is_contiguous() and logp.movedim(0, -1).is_contiguous()


def _rows_volume(logp):
    """logp [D, ...] as a view of channels-last memory -> (that memory [..., D], D, pixels)."""
    logp = _need(logp, "logp", strided=True)
    rows = logp.movedim(0, -1)
    if not rows.is_contiguous():
        raise ValueError("channels_last=True: logp %s with strides %s is not a view of contiguous [..., D] memory"
                         % (tuple(logp.shape), tuple(logp.stride())))
    return rows, logp.shape[0], logp.numel() // logp.shape[0]


def depth_regress(logp, d_candi, want_conf=True, channels_last=False, out=None):
    """logp [D, ...] -> (expected depth [...], max log-prob [...]).  channels_last: logp is a [D, ...] view of contiguous
    channels-last memory [..., D] and is read as it lies (nrgbd_depth_regress_rows: the same bits, no transposing copy).
    out: a contiguous fp32 tensor of the depth map's shape to write it into (default: a fresh one)."""
    if channels_last:
        rows, D, n = _rows_volume(logp)
    else:
        logp = _need(logp, "logp")
        D = logp.shape[0]
        n = logp.numel() // D
    d_candi = _need(d_candi, "d_candi", (D,))
    depth = torch.empty(logp.shape[1:], dtype=torch.float32, device=logp.device) if out is None else out
    if (depth.shape != logp.shape[1:] or depth.dtype != torch.float32 or depth.device != logp.device or not depth.is_contiguous()):
        raise ValueError("depth_regress: out must be a contiguous float32 tensor %s on %s" % (tuple(logp.shape[1:]), logp.device))
    conf = torch.empty_like(depth) if want_conf else None
    with torch.cuda.device(logp.device):
        if channels_last:
            rc = _lib.load().nrgbd_depth_regress_rows(_p(rows), _p(d_candi), _p(depth), _p(conf), D, n, _stream(logp))
        else:
            rc = _lib.load().nrgbd_depth_regress(_p(logp), _p(d_candi), _p(depth), _p(conf), D, n, _stream(logp))
    _lib.check(rc, "nrgbd_depth_regress_rows" if channels_last else "nrgbd_depth_regress")
    return depth, conf


def export_depth_u16(logp, d_candi, depth_scale=1000.0, conf_scale=1000.0, channels_last=False):
    """logp [D, ...] -> (depth f32, conf f32 = exp(max logp), depth_u16, conf_u16 [as int16 storage viewed uint16]).
    channels_last: as depth_regress (nrgbd_export_depth_u16_rows)."""
    if channels_last:
        rows, D, n = _rows_volume(logp)
    else:
        logp = _need(logp, "logp")
        D = logp.shape[0]
        n = logp.numel() // D
    d_candi = _need(d_candi, "d_candi", (D,))
    shp = logp.shape[1:]
    depth = torch.empty(shp, dtype=torch.float32, device=logp.device)
    conf = torch.empty_like(depth)
    du = torch.empty(shp, dtype=torch.uint16, device=logp.device)
    cu = torch.empty(shp, dtype=torch.uint16, device=logp.device)
    entry = "nrgbd_export_depth_u16_rows" if channels_last else "nrgbd_export_depth_u16"
    with torch.cuda.device(logp.device):
        rc = getattr(_lib.load(), entry)(_p(rows if channels_last else logp), _p(d_candi), float(depth_scale), float(conf_scale),
                                         _p(depth), _p(conf), _p(du), _p(cu), D, n, _stream(logp))
    _lib.check(rc, entry)
    return depth, conf, du, cu


def warp_depth_fwd(src, dmap, K, R, t, rays):
    """src [N,C,H,W], dmap [H,W], K [3,3], R [N,3,3], t [N,3], rays [3,HW] -> warped [N,C,H,W] (nrgbd_warp_depth_fwd)."""
    src = _need(src, "src")
    N, C, H, W = src.shape
    dmap = _need(dmap, "dmap").reshape(H, W)
    K = _need(K, "K", (3, 3)); R = _need(R, "R", (N, 3, 3)); t = _need(t, "t", (N, 3)); rays = _need(rays, "rays", (3, H * W))
    out = torch.empty_like(src)
    with torch.cuda.device(src.device):
        rc = _lib.load().nrgbd_warp_depth_fwd(_p(src), _p(dmap), _p(K), _p(R), _p(t), _p(rays), _p(out), N, C, H, W, _stream(src))
    _lib.check(rc, "nrgbd_warp_depth_fwd")
    return out


def warp_depth_bwd(src, dmap, K, R, t, rays, g_out):
    """Gradient of sum(warp_depth_fwd(...) * g_out) w.r.t. (R [N,3,3], t [N,3])."""
    src = _need(src, "src")
    N, C, H, W = src.shape
    dmap = _need(dmap, "dmap").reshape(H, W)
    K = _need(K, "K", (3, 3)); R = _need(R, "R", (N, 3, 3)); t = _need(t, "t", (N, 3)); rays = _need(rays, "rays", (3, H * W))
    g_out = _need(g_out, "g_out", src.shape)
    nwg = int(_lib.load().nrgbd_warp_depth_bwd_workgroups(H, W))
    partial = torch.empty((N, nwg, 12), dtype=torch.float32, device=src.device)
    g_R = torch.empty((N, 3, 3), dtype=torch.float32, device=src.device)
    g_t = torch.empty((N, 3), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        rc = _lib.load().nrgbd_warp_depth_bwd(_p(src), _p(dmap), _p(K), _p(R), _p(t), _p(rays), _p(g_out), _p(partial),
                                               _p(g_R), _p(g_t), N, C, H, W, _stream(src))
    _lib.check(rc, "nrgbd_warp_depth_bwd")
    return g_R, g_t


# ----------------------------------------------------------------------------- local bundle adjustment (opt_pose.py)
LBA_STATE = 32          # NRGBD_LBA_STATE: floats per view of the optimiser state (uq, t, R, Adam moments)
LBA_MAX_LEVELS = 8      # NRGBD_LBA_MAX_LEVELS
MAX_V = 16              # NRGBD_MAX_V
LBA_MAX_PLANES = 5 + 3 * MAX_V     # lba.hip kLbaMaxPlanes: ref (3) + sources (3 N) + depth + confidence


def lba_pyramid(planes, ks):
    """Every level F.avg_pool2d(plane, k) (floor sizes, each from the full-resolution plane) of the [H,W] planes in one launch
    (nrgbd_lba_pyramid) -> list over levels of [nplanes, H//k, W//k] views into one buffer."""
    P = len(planes)
    if not 1 <= P <= LBA_MAX_PLANES:                  # checked before anything touches the device
        raise ValueError("lba_pyramid: %d planes, 1 to %d" % (P, LBA_MAX_PLANES))
    H, W = planes[0].shape
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= LBA_MAX_LEVELS or min(ks) < 1 or H // max(ks) == 0 or W // max(ks) == 0:
        raise ValueError("lba_pyramid: kernel sizes %s invalid for %dx%d" % (ks, H, W))
    planes = [_need(x, "plane %d" % i) for i, x in enumerate(planes)]
    for x in planes:
        if tuple(x.shape) != (H, W) or x.device != planes[0].device:
            raise ValueError("lba_pyramid: every plane must be [%d,%d] on %s" % (H, W, planes[0].device))
    sizes = [(H // k, W // k) for k in ks]
    out = torch.empty(P * sum(h * w for h, w in sizes), dtype=torch.float32, device=planes[0].device)
    ptrs = (ctypes.c_void_p * P)(*[x.data_ptr() for x in planes])
    karr = (ctypes.c_int * len(ks))(*ks)
    with torch.cuda.device(out.device):
        rc = _lib.load().nrgbd_lba_pyramid(ptrs, P, H, W, karr, len(ks), _p(out), _stream(out))
    _lib.check(rc, "nrgbd_lba_pyramid")
    levels, off = [], 0
    for h, w in sizes:
        levels.append(out[off:off + P * h * w].view(P, h, w))
        off += P * h * w
    return levels


def lba_workgroups(H, W):
    return int(_lib.load().nrgbd_lba_workgroups(H, W))


def lba_grad(ref, src, dmap, conf, K, rays, state, partial):
    """One fused loss + gradient pass at the poses held in state [N, LBA_STATE] (nrgbd_lba_grad): ref [3,H,W], src [N,3,H,W],
    dmap / conf [H,W], K [3,3], rays [3,HW] -> partial [N, lba_workgroups(H, W), 13] (a flat buffer at least that large)."""
    src = _need(src, "src")
    N, C, H, W = src.shape
    if C != 3 or not 1 <= N <= MAX_V:
        raise ValueError("lba_grad: src must be [N<=%d,3,H,W], got %s" % (MAX_V, tuple(src.shape)))
    ref = _need(ref, "ref", (3, H, W)); dmap = _need(dmap, "dmap", (H, W)); conf = _need(conf, "conf", (H, W))
    K = _need(K, "K", (3, 3)); rays = _need(rays, "rays", (3, H * W)); state = _need(state, "state", (N, LBA_STATE))
    partial = _need(partial, "partial")
    if partial.numel() < N * lba_workgroups(H, W) * 13:
        raise ValueError("lba_grad: partial holds %d floats, %d needed" % (partial.numel(), N * lba_workgroups(H, W) * 13))
    with torch.cuda.device(src.device):
        rc = _lib.load().nrgbd_lba_grad(_p(ref), _p(src), _p(dmap), _p(conf), _p(K), _p(rays), _p(state), _p(partial),
                                        N, H, W, _stream(src))
    _lib.check(rc, "nrgbd_lba_grad")
    return partial


def lba_init(init, state):
    """state[n] <- (uq, t) = init [N,6], Adam moments 0, R from uq (nrgbd_lba_update, step 0)."""
    state = _need(state, "state")
    N = state.shape[0]
    init = _need(init, "init", (N, 6))
    if tuple(state.shape) != (N, LBA_STATE) or not 1 <= N <= MAX_V:
        raise ValueError("lba_init: state must be [N<=%d,%d]" % (MAX_V, LBA_STATE))
    with torch.cuda.device(state.device):
        rc = _lib.load().nrgbd_lba_update(None, 1, _p(init), _p(state), None, 1, 0, N, 1, 1, 1, 0, 0.0, 0, 0, _stream(state))
    _lib.check(rc, "nrgbd_lba_update")
    return state


def lba_update(partial, state, loss_log, log_slot, H, W, joint, step, lr, opt_R, opt_t):
    """Adam step number `step` (>= 1) from the partials of lba_grad at an H x W level (nrgbd_lba_update); the loss goes to
    loss_log[0, log_slot] (joint) or loss_log[n, log_slot]."""
    state = _need(state, "state")
    N = state.shape[0]
    if tuple(state.shape) != (N, LBA_STATE) or not 1 <= N <= MAX_V:
        raise ValueError("lba_update: state must be [N<=%d,%d]" % (MAX_V, LBA_STATE))
    partial = _need(partial, "partial")
    loss_log = _need(loss_log, "loss_log")
    if loss_log.dim() != 2 or loss_log.shape[0] != (1 if joint else N) or not 0 <= log_slot < loss_log.shape[1]:
        raise ValueError("lba_update: loss_log %s / slot %d" % (tuple(loss_log.shape), log_slot))
    if step < 1:
        raise ValueError("lba_update: step counts from 1 (lba_init is step 0)")
    with torch.cuda.device(state.device):
        rc = _lib.load().nrgbd_lba_update(_p(partial), lba_workgroups(H, W), None, _p(state), _p(loss_log),
                                          int(loss_log.shape[1]), int(log_slot), N, H, W, int(bool(joint)), int(step),
                                          float(lr), int(bool(opt_R)), int(bool(opt_t)), _stream(state))
    _lib.check(rc, "nrgbd_lba_update")
    return state


class LbaLevel:
    """The two launches of one LBA iteration at one pyramid level with their arguments checked once (lba_grad / lba_update's
    checks) and kept as ctypes values: the optimiser calls them scales x iterations times."""

    def __init__(self, ref, src, dmap, conf, K, rays, state, partial, loss_log, joint, opt_R, opt_t):
        lba_grad(ref, src, dmap, conf, K, rays, state, partial)            # validates (and runs) the first pass
        self._keep = (ref, src, dmap, conf, K, rays, state, partial, loss_log)
        N, _, H, W = src.shape
        self.H, self.W = H, W
        self._lib = _lib.load()
        self._g = (_p(ref), _p(src), _p(dmap), _p(conf), _p(K), _p(rays), _p(state), _p(partial), N, H, W, _stream(src))
        self._u = (_p(partial), lba_workgroups(H, W), None, _p(state), _p(loss_log), int(loss_log.shape[1]))
        self._u2 = (N, H, W, int(bool(joint)))
        self._u3 = (int(bool(opt_R)), int(bool(opt_t)), _stream(src))
        self._args = (state, loss_log, joint, opt_R, opt_t)
        self._first = True

    def grad(self):
        if self._first:            # the constructor ran this iteration's pass
            self._first = False
            return
        _lib.check(self._lib.nrgbd_lba_grad(*self._g), "nrgbd_lba_grad")

    def update(self, log_slot, step, lr):
        state, loss_log, joint, opt_R, opt_t = self._args
        if not 0 <= log_slot < loss_log.shape[1] or step < 1:
            raise ValueError("LbaLevel.update: slot %d / step %d" % (log_slot, step))
        _lib.check(self._lib.nrgbd_lba_update(*self._u, int(log_slot), *self._u2, int(step), float(lr), *self._u3),
                   "nrgbd_lba_update")


# ----------------------------------------------------------------------------- K-Net convolutions
def conv3d_workgroups(D, H, W):
    return int(_lib.load().nrgbd_conv3d_workgroups(D, H, W))


def conv3d_pack_weights(w):
    """w [64, Cin, 3, 3, 3] -> packed B-operand stream for conv3d (one 1 KB line per wave load)."""
    w = _need(w, "w")
    cout, cin = w.shape[:2]
    if cout != 64 or tuple(w.shape[2:]) != (3, 3, 3):
        raise ValueError("conv3d_pack_weights expects [64, Cin, 3, 3, 3], got %s" % (tuple(w.shape),))
    wp = torch.empty(27 * cin * 64, dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        rc = _lib.load().nrgbd_conv3d_pack_weights(_p(w), _p(wp), cin, _stream(w))
    _lib.check(rc, "nrgbd_conv3d_pack_weights")
    return wp


def conv3d(x, w_packed, x_ss=None, x_relu=False, res=None, res_ss=None, res_relu=False,
           materialize=False, want_stats=True, out=None, mat_out=None):
    """Channels-last 3x3x3 convolution on the fp32 matrix cores.

    x [D,H,W,Cin]; input = act(x*s+t) (+ act(res*s'+t')).  Returns (y [D,H,W,64], stats | None, materialized | None).
    """
    x = _need(x, "x")
    D, H, W, Cin = x.shape
    y = out if out is not None else torch.empty((D, H, W, 64), dtype=torch.float32, device=x.device)
    nwg = conv3d_workgroups(D, H, W)
    stats = torch.empty((nwg, 128), dtype=torch.float32, device=x.device) if want_stats else None
    mat = None
    if materialize:
        mat = mat_out if mat_out is not None else torch.empty_like(x)
    if res is not None:
        res = _need(res, "res", x.shape)
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_conv3d_3x3x3_f32(_p(x), _p(x_ss), int(x_relu), _p(res), _p(res_ss), int(res_relu),
                                                 _p(mat), _p(w_packed), _p(y), _p(stats), D, H, W, Cin, 64, _stream(x))
    _lib.check(rc, "nrgbd_conv3d_3x3x3_f32")
    return y, stats, mat


def _wino_pack(w, transposed, name, points):
    """Shared body of the three Winograd weight packers.  points: transform points along depth of the stream (4: wino_dw.hip,
    6: wino_dw4.hip), None: one 2-D stream per depth tap (wino_pc.hip: kd = 3, or kd = 1 for a [Cout, Cin, 3, 3] weight).
    transposed: False = the forward stream, True = the data-gradient stream (w is the FORWARD weight [Cin', Cout', ...]: channel axes
    swapped, taps flipped), 2 = both in one launch: a buffer of twice the size, forward half first (ops.conv_wino_pack_both)."""
    w = _need(w, "w")
    if points is None and w.dim() == 4:
        w = w[:, :, None]
    if w.dim() != 5 or tuple(w.shape[3:]) != (3, 3) or w.shape[2] not in ((1, 3) if points is None else (3,)):
        raise ValueError("%s expects [Cout, Cin, %s3, 3, 3], got %s" % (name, "(3,) " if points is None else "", tuple(w.shape)))
    Cout, Cin = (w.shape[1], w.shape[0]) if transposed is True or transposed == 1 else w.shape[:2]
    if Cout % 64 or Cin % 16 or (transposed == 2 and Cin % 64):
        raise ValueError("%s: Cout %% 64 and Cin %% 16 required, got Cout=%d Cin=%d" % (name, Cout, Cin))
    kd = [int(w.shape[2])] if points is None else []          # nrgbd_conv_wino_pack alone takes the tap count
    wp = torch.empty(Cout * Cin * (points or kd[0]) * 16 * (2 if transposed == 2 else 1), dtype=torch.float32, device=w.device)
    wc = w.detach().contiguous()
    with torch.cuda.device(w.device):
        rc = getattr(_lib.load(), "nrgbd_" + name)(_p(wc), _p(wp), Cin, Cout, *kd, int(transposed), _stream(w))
    _lib.check(rc, "nrgbd_" + name)
    return wp


def conv_wino_pack(w, transposed=False):
    """w [Cout, Cin, 3, 3, 3] (kd = 3) or [Cout, Cin, 3, 3] (kd = 1) -> Winograd-domain B-operand stream of nrgbd_conv_wino_f32:
    U = G g G^T over (ky, kx) in float64, rounded once to fp32, laid out [cg][stage = cb*kd + depth tap][xi = 4*xi_y + xi_x]
    [wave][lane = kq*16 + j][e] with ci = cb*16 + 4*kq + e and co = cg*64 + 16*wave + j.  transposed: see _wino_pack."""
    return _wino_pack(w, transposed, "conv_wino_pack", None)


def conv_wino_pack_both(w, dw=False):
    """(forward stream, data-gradient stream) of a layer's weight in ONE launch (training re-packs both every iteration).
    dw: the streams of wino_dw.hip (Winograd along depth too; dw = 4: wino_dw4.hip, F(4,3) along depth) instead of wino_pc.hip's."""
    both = (conv_wino_dw4_pack if dw == 4 else conv_wino_dw_pack if dw else conv_wino_pack)(w, transposed=2)
    n = both.numel() // 2
    return both[:n], both[n:]


def conv_wino_pack_reference(w):
    """The same stream through torch (einsum in float64): what the device packer is tested against."""
    if w.dim() == 4:
        w = w[:, :, None]
    Cout, Cin, KD = w.shape[:3]
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64, device=w.device)
    U = torch.einsum("ay,ockyx,bx->ockab", G, w.detach().double(), G).reshape(Cout, Cin, KD, 16)   # [co, ci, kd, xi]
    U = U.reshape(Cout // 64, 4, 16, Cin // 16, 4, 4, KD, 16)   # co -> (cg, wave, j); ci -> (cb, kq, e)
    U = U.permute(0, 3, 6, 7, 1, 4, 2, 5).contiguous()          # [cg, cb, kd, xi, wave, kq, j, e]
    return U.to(torch.float32).reshape(-1)


def conv_wino_supported(N, H, W, Cin, Cout, kd):
    """Shapes nrgbd_conv_wino_f32 accepts (the callers fall back to the direct kernels otherwise): channel multiples, at least
    two stages, an even stage count except for the 16-channel 3-D first layer, 32-bit byte offsets in the loader."""
    stages = (Cin // 16) * kd
    span = (1 if kd == 3 else N) * H * W * Cin
    if Cout == 32:      # the HALF form of wino_pc.hip: 2-D, dilation 1 (the caller's business), weights packed by conv_wino_pack32
        return kd == 1 and Cin % 16 == 0 and stages >= 2 and stages % 2 == 0 and span < (1 << 30)
    return Cin % 16 == 0 and Cout % 64 == 0 and stages >= 2 and (stages % 2 == 0 or (kd == 3 and Cin == 16)) and span < (1 << 30)


def conv_wino_pack32(w):
    """Weight stream of a 32-output-channel 3x3 layer for the HALF form of nrgbd_conv_wino_f32 (Cout = 32): the 64-column stream
    with the upper 32 columns zero (the kernel's waves read the two 16-column lines that exist)."""
    w = _need(w, "w")
    if w.dim() != 4 or w.shape[0] != 32 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError("conv_wino_pack32 expects [32, Cin, 3, 3], got %s" % (tuple(w.shape),))
    return conv_wino_pack(torch.cat((w.detach(), torch.zeros_like(w)), 0))


def conv_wino_tiles(N, H, W, dilation=1):
    return int(_lib.load().nrgbd_conv_wino_tiles(N, H, W, dilation))


def conv_wino(x, w_wino, Cout, kd, dilation=1, x_ss=None, x_relu=False, res=None, res_ss=None, res_relu=False,
              materialize=False, want_stats=True):
    """Channels-last 3x3(x3) stride-1 convolution in the Winograd domain on the producer/consumer kernel (wino_pc.hip):
    x [N,H,W,Cin] -> (y [N,H,W,Cout], stats [2*Cout, tiles] (column-major partials for bn_finalize_cm) | None,
    materialized | None); kd = 3 convolves over N as depth."""
    x = _need(x, "x")
    N, H, W, Cin = x.shape
    y = torch.empty((N, H, W, Cout), dtype=torch.float32, device=x.device)
    half = Cout == 32     # HALF form: one statistics row per (tile, row block); the weight stream is the zero-padded 64-column one
    if half and (kd != 1 or dilation != 1):
        raise ValueError("conv_wino: Cout = 32 is the 2-D, dilation-1 form only")
    stats = torch.empty((2 * Cout, (2 if half else 1) * conv_wino_tiles(N, H, W, dilation)), dtype=torch.float32, device=x.device) if want_stats else None
    mat = torch.empty_like(x) if materialize else None
    if res is not None:
        res = _need(res, "res", x.shape)
    if w_wino.numel() != max(1, Cout // 64) * (Cin // 16) * kd * 16 * 1024:
        raise ValueError("conv_wino: packed weights do not match Cin=%d Cout=%d kd=%d" % (Cin, Cout, kd))
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_conv_wino_f32(_p(x), _p(x_ss), int(x_relu), _p(res), _p(res_ss), int(res_relu), _p(mat),
                                              _p(w_wino), _p(y), _p(stats), N, H, W, Cin, Cout, kd, dilation, _stream(x))
    _lib.check(rc, "nrgbd_conv_wino_f32")
    return y, stats, mat


def conv_wino_dw_pack(w, transposed=False):
    """w [Cout, Cin, 3, 3, 3] -> weight stream of nrgbd_conv_wino_dw_f32 (Winograd in depth too): U_t = sum_kd G[t][kd] (G g_kd G^T)
    in float64, rounded once, laid out [cg][stage = t*(Cin/16) + cb][xi][wave][lane = kq*16 + j][e].  transposed: see _wino_pack."""
    return _wino_pack(w, transposed, "conv_wino_dw_pack", 4)


def conv_wino_dw_pack_reference(w):
    """The same stream through torch (einsum in float64): what the device packer is tested against."""
    Cout, Cin = w.shape[:2]
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64, device=w.device)
    U = torch.einsum("tz,ay,oczyx,bx->octab", G, G, w.detach().double(), G).reshape(Cout, Cin, 4, 16)   # [co, ci, t, xi]
    U = U.reshape(Cout // 64, 4, 16, Cin // 16, 4, 4, 4, 16)    # co -> (cg, wave, j); ci -> (cb, kq, e); t; xi
    U = U.permute(0, 6, 3, 7, 1, 4, 2, 5).contiguous()          # [cg, t, cb, xi, wave, kq, j, e]
    return U.to(torch.float32).reshape(-1)


def conv_wino_dw_supported(N, H, W, Cin, Cout):
    """Shapes nrgbd_conv_wino_dw_f32 accepts: pairs of depth slices, whole 8x16 tiles, 32-bit in-plane byte offsets."""
    return N % 2 == 0 and N >= 2 and H % 8 == 0 and W % 16 == 0 and Cin % 16 == 0 and Cout % 64 == 0 and H * W * Cin < (1 << 30)


def relu_unit(gamma, beta, n):
    """2^-k with 2^k > |gamma_c| sqrt(n) + |beta_c| for every channel: a bound on |BatchNorm(y)_c| under batch statistics over n
    values that holds for ANY data (|y - mean| <= sqrt(n var)), i.e. the x_unit of the clamped-FMA convolution forms.  Reads the
    affine parameters once (host synchronisation: callers cache it with the packed weights)."""
    import math
    bound = float(gamma.detach().abs().max()) * math.sqrt(float(n)) + float(beta.detach().abs().max())
    # One extra power of two of headroom (free: a power-of-two unit changes no bit below saturation).  The bound is exact for exact
    # statistics; the kernels finalise the variance as E[y^2] - mean^2 from fp32 per-tile sums (in float64), which can UNDER-estimate
    # it when |mean| >> std (a tile's partial of y^2 is good to ~1.5e-5 relative) and so over-scale the normalised values.  The
    # finalisers guard the other side (csrc/common.hpp bn_finalize_channel): a channel whose computed variance falls below
    # 1e-5 mean^2 gets a NaN scale (loud: the frame's outputs are NaN, valid_dpv trips) — whenever the scale is finite the computed
    # variance is at least 1 / 2.5 of the true one, inside the factor 4 that the doubled bound covers.  The clamp can therefore not
    # saturate silently (tests/test_gpu_knet.py constructs the collapsing channel)
    return 2.0 ** -max(0, math.floor(math.log2(max(2.0 * bound, 1e-30))) + 1)


def conv_wino_dw(x, w_wino, Cout, x_ss=None, x_relu=False, res=None, res_ss=None, res_relu=False, materialize=False,
                 want_stats=True, x_unit=0.0):
    """Channels-last 3x3x3 stride-1 convolution over x [D,H,W,Cin] with Winograd in all three dimensions (wino_dw.hip):
    -> (y [D,H,W,Cout], stats [2*Cout, tiles] (column-major partials for bn_finalize_cm) | None, materialized | None).
    x_unit = 2^-k > 0: the clamped-FMA form (nrgbd_conv_wino_dw_unit_f32) — x_ss and x_relu required, no residual / materialise,
    and w_wino packed from 2^k * w."""
    x = _need(x, "x")
    N, H, W, Cin = x.shape
    y = torch.empty((N, H, W, Cout), dtype=torch.float32, device=x.device)
    stats = torch.empty((2 * Cout, conv_wino_tiles(N, H, W, 1)), dtype=torch.float32, device=x.device) if want_stats else None
    mat = torch.empty_like(x) if materialize else None
    if res is not None:
        res = _need(res, "res", x.shape)
    if w_wino.numel() != (Cout // 64) * (Cin // 16) * 4 * 16 * 1024:
        raise ValueError("conv_wino_dw: packed weights do not match Cin=%d Cout=%d" % (Cin, Cout))
    with torch.cuda.device(x.device):
        if x_unit:
            if x_ss is None or not x_relu or res is not None or materialize:
                raise ValueError("conv_wino_dw: x_unit is the plain BatchNorm + ReLU form only")
            rc = _lib.load().nrgbd_conv_wino_dw_unit_f32(_p(x), _p(x_ss), float(x_unit), _p(w_wino), _p(y), _p(stats), N, H, W, Cin,
                                                          Cout, _stream(x))
        else:
            rc = _lib.load().nrgbd_conv_wino_dw_f32(_p(x), _p(x_ss), int(x_relu), _p(res), _p(res_ss), int(res_relu), _p(mat),
                                                     _p(w_wino), _p(y), _p(stats), N, H, W, Cin, Cout, _stream(x))
    _lib.check(rc, "nrgbd_conv_wino_dw_f32")
    return y, stats, mat


def conv_wino_dw4_supported(N, H, W, Cin, Cout):
    """Shapes nrgbd_conv_wino_dw4_f32 accepts: quadruples of depth slices, whole 8x16 tiles, 32-bit in-plane byte offsets."""
    return N % 4 == 0 and N >= 4 and H % 8 == 0 and W % 16 == 0 and Cin % 16 == 0 and Cout % 64 == 0 and H * W * Cin < (1 << 30)


def conv3d_kernel(D, H, W, Cin, Cout, candidates):
    """Which kernel runs a channels-last 3x3x3 layer on a [D, H, W, Cin] input: the first of `candidates`, in order, that takes the
    shape.  "dw4" = wino_dw4.hip (6 multiplies per output voxel; D % 4 == 0), "dw" = wino_dw.hip (8; D even) — both whole 8x16 tiles
    —, "pc" = wino_pc.hip (12; any grid), each for 16, 32 or 64 inputs and 64 outputs; "direct" = conv3d.hip (27) takes every grid at 16
    or 64 inputs and ends every search.  Cin = 32 (the first layer of a 7-frame window: 22 channels zero-padded) has no direct form:
    its tuples leave "direct" out, which is also what admits the width — a list that names "direct" is a list for 16 or 64 inputs and
    answers "direct" for any other width, as it always did —, and a grid none of the three takes (2^30 bytes of input per depth
    slice) is an NrgbdError.  Pure host code: this is the one place the choice is written down.  Who passes what:

      caller                                      Cin  candidates             why not the full list
      K-Net inference (KalmanGainNet.kernels)     any  dw4, dw, pc, direct    -
        ... generation="wino_pc" (tests)          any  pc, direct             compares the kernels on the whole stack
        ... generation="direct" (tests)           any  direct
        ... a layer with a fused residual         64   dw, pc, direct         wino_dw4.hip has no residual form (only with
                                                                              _split_residual off: an A/B)
      autograd 64 -> 64, both directions          64   dw4, dw, pc, direct    (Conv3dCL.kernels)
      autograd 16 -> 64 forward                   16   dw4, direct            (Conv3dCL.kernels_first) its 16-input forms of wino_dw /
                                                                              wino_pc were never timed against the direct kernel
                                                                              at the training grids: inference takes them, training
                                                                              does not
      autograd 16 -> 64 data gradient             64   dw4, dw, direct        (Conv3dCL.kernels_first_dgrad) the layer zero-padded to
                                                                              64 -> 64 on dL/dy; wino_pc.hip was never timed here
      first layer at 32 inputs, both paths        32   dw4, dw, pc            (KalmanGainNet.kernels32, Conv3dCL.kernels_first32)
                                                                              conv3d.hip is instantiated for 16 and 64 inputs
    The A/B switches are edits of those tuples (tools/knet_ab.py drops "dw4")."""
    takes = {"dw4": conv_wino_dw4_supported, "dw": conv_wino_dw_supported, "pc": lambda *shape: conv_wino_supported(*shape, 3)}
    widths = (16, 64) if "direct" in candidates or not candidates else (16, 32, 64)
    for kind in candidates:
        if kind != "direct" and Cout == 64 and Cin in widths and takes[kind](D, H, W, Cin, Cout):
            return kind
        if kind == "direct":
            break
    if Cin == 32 and candidates and "direct" not in candidates:
        raise _lib.NrgbdError("no hand-written kernel for a 3x3x3 layer with 32 inputs on a %d x %d x %d grid (candidates %s)"
                              % (D, H, W, ", ".join(candidates)))
    return "direct"


def conv_wino_dw4_pack(w, transposed=False):
    """w [Cout, Cin, 3, 3, 3] -> weight stream of nrgbd_conv_wino_dw4_f32 (F(2x2,3x3) in the plane x F(4,3) along depth, points
    0, +-1/2, +-3/2, inf): U_t = sum_kd Gd[t][kd] (G g_kd G^T) in float64, rounded once, phases in execution order t = 1,2,3,4,0,5.
    transposed: see _wino_pack."""
    return _wino_pack(w, transposed, "conv_wino_dw4_pack", 6)


def conv_wino_dw4(x, w_wino, Cout, x_ss=None, x_relu=False, want_stats=True, x_unit=0.0):
    """Channels-last 3x3x3 stride-1 convolution over x [D,H,W,Cin] with F(4,3) along depth on top of the in-plane F(2x2,3x3)
    (wino_dw4.hip; D % 4 == 0): -> (y [D,H,W,Cout], stats [2*Cout, tiles] | None).  Input forms: x as it is (x_ss None, x_relu False),
    act(x * s + t), or — x_unit = 2^-k > 0 — relu(x * s + t) as the clamped FMA with w_wino packed from 2^k * w."""
    x = _need(x, "x")
    N, H, W, Cin = x.shape
    if w_wino.numel() != (Cout // 64) * (Cin // 16) * 6 * 16 * 1024:
        raise ValueError("conv_wino_dw4: packed weights do not match Cin=%d Cout=%d" % (Cin, Cout))
    y = torch.empty((N, H, W, Cout), dtype=torch.float32, device=x.device)
    stats = torch.empty((2 * Cout, conv_wino_tiles(N, H, W, 1)), dtype=torch.float32, device=x.device) if want_stats else None
    lib = _lib.load()
    with torch.cuda.device(x.device):
        nbytes = ctypes.c_size_t(0)
        _lib.check(lib.nrgbd_conv_wino_dw4_workspace(N, H, W, Cout, ctypes.byref(nbytes)), "nrgbd_conv_wino_dw4_workspace")
        # per-launch scratch from the caching allocator (stream-aware: concurrent launches on other streams get other blocks; inside a
        # hipGraph capture it lives in the graph's pool): 32 KB per workgroup, no kernel is launched for it
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=x.device)
        rc = lib.nrgbd_conv_wino_dw4_f32(_p(x), _p(x_ss), int(x_relu), float(x_unit), _p(w_wino), _p(y), _p(stats), _p(ws),
                                         ctypes.c_size_t(ws.numel()), N, H, W, Cin, Cout, _stream(x))
    _lib.check(rc, "nrgbd_conv_wino_dw4_f32")
    return y, stats


def conv3d_wgrad(x, gy):
    """Weight gradient of the channels-last 3x3x3 convolution: x [D,H,W,Cin] (Cin 16, 32 or 64), gy [D,H,W,64] -> dW [64,Cin,3,3,3]."""
    x = _need(x, "x")
    D, H, W, Cin = x.shape
    gy = _need(gy, "gy", (D, H, W, 64))
    nwg = int(_lib.load().nrgbd_conv3d_wgrad_workgroups())
    partial = torch.empty(nwg * 27 * 64 * Cin, dtype=torch.float32, device=x.device)
    dw = torch.empty((64, Cin, 3, 3, 3), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_conv3d_wgrad_f32(_p(x), _p(gy), _p(partial), _p(dw), D, H, W, Cin, _stream(x))
    _lib.check(rc, "nrgbd_conv3d_wgrad_f32")
    return dw


def conv3d_cout1(x, w_tap_major, x_ss=None, x_relu=False, res=None, res_ss=None, res_relu=False):
    """Last K-Net layer: x [D,H,W,64] -> y [D,H,W]; w_tap_major [27,64]."""
    x = _need(x, "x")
    D, H, W, Cin = x.shape
    w_tap_major = _need(w_tap_major, "w_tap_major", (27, Cin))
    y = torch.empty((D, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_conv3d_3x3x3_cout1_f32(_p(x), _p(x_ss), int(x_relu), _p(res), _p(res_ss), int(res_relu),
                                                       _p(w_tap_major), _p(y), D, H, W, Cin, _stream(x))
    _lib.check(rc, "nrgbd_conv3d_3x3x3_cout1_f32")
    return y


def conv3d_cout1_dgrad(gy, w_tap_major):
    """Data gradient of the K-Net's last layer Conv3d(64, 1): gy [D,H,W], w_tap_major [27,64] -> gx [D,H,W,64] (conv3d_c1_bwd.hip)."""
    gy = _need(gy, "gy")
    D, H, W = gy.shape
    w_tap_major = _need(w_tap_major, "w_tap_major", (27, 64))
    gx = torch.empty((D, H, W, 64), dtype=torch.float32, device=gy.device)
    with torch.cuda.device(gy.device):
        rc = _lib.load().nrgbd_conv3d_cout1_dgrad_f32(_p(gy), _p(w_tap_major), _p(gx), D, H, W, _stream(gy))
    _lib.check(rc, "nrgbd_conv3d_cout1_dgrad_f32")
    return gx


def conv3d_cout1_wgrad(x, gy):
    """Weight gradient of the K-Net's last layer Conv3d(64, 1): x [D,H,W,64], gy [D,H,W] -> dW [1,64,3,3,3] (conv3d_c1_bwd.hip)."""
    x = _need(x, "x")
    D, H, W, Cin = x.shape
    if Cin != 64:
        raise ValueError("conv3d_cout1_wgrad: 64 input channels, got %d" % Cin)
    gy = _need(gy, "gy", (D, H, W))
    lib = _lib.load()
    dw = torch.empty((1, 64, 3, 3, 3), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        nbytes = ctypes.c_size_t(0)
        _lib.check(lib.nrgbd_conv3d_cout1_wgrad_workspace(D, H, W, ctypes.byref(nbytes)), "nrgbd_conv3d_cout1_wgrad_workspace")
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=x.device)
        rc = lib.nrgbd_conv3d_cout1_wgrad_f32(_p(x), _p(gy), _p(dw), _p(ws), ctypes.c_size_t(ws.numel()), D, H, W, _stream(x))
    _lib.check(rc, "nrgbd_conv3d_cout1_wgrad_f32")
    return dw


def _status_ptr(status, like):
    if status is None:
        return ctypes.c_void_p(0)
    if not (isinstance(status, torch.Tensor) and status.is_cuda and status.dtype == torch.int32 and status.numel() >= 1 and status.device == like.device):
        raise TypeError("status must be an int32 tensor on the device of the statistics")
    return ctypes.c_void_p(status.data_ptr())


def _nbt_ptr(nbt, like):
    if nbt is None:
        return ctypes.c_void_p(0)
    if not (isinstance(nbt, torch.Tensor) and nbt.is_cuda and nbt.dtype == torch.int64 and nbt.numel() == 1 and nbt.device == like.device):
        raise TypeError("batches_tracked must be an int64 scalar tensor on the device of the statistics")
    return ctypes.c_void_p(nbt.data_ptr())


def bn3d_finalize(stats, count, gamma, beta, eps, momentum, running_mean=None, running_var=None, status=None, batches_tracked=None):
    """Per-workgroup partials -> scale_shift [64,2]; updates the running statistics in place (train mode).
    status: int32 device word that counts variance-collapsed channels (include/nrgbd.h; nets.check_status raises on it)."""
    stats = _need(stats, "stats")
    ss = torch.empty((64, 2), dtype=torch.float32, device=stats.device)
    with torch.cuda.device(stats.device):
        rc = _lib.load().nrgbd_bn3d_finalize(_p(stats), stats.shape[0], int(count), _p(gamma), _p(beta), float(eps),
                                             float(momentum), _p(running_mean), _p(running_var), _p(ss), _status_ptr(status, stats), _nbt_ptr(batches_tracked, stats),
                                             _stream(stats))
    _lib.check(rc, "nrgbd_bn3d_finalize")
    return ss


# ----------------------------------------------------------------------------- 2-D feature CNN helpers
def conv2d_workgroups(N, H, W):
    return int(_lib.load().nrgbd_conv2d_workgroups(N, H, W))


def conv_pack_weights(w):
    """w [Cout, Cin, 3, 3] (or [Cout, Cin, 3, 3, 3]) -> packed B-operand stream of the matrix-core conv kernels."""
    w = _need(w, "w")
    cout, cin = w.shape[:2]
    taps = 1
    for k in w.shape[2:]:
        taps *= int(k)
    wp = torch.empty(taps * cin * cout, dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        rc = _lib.load().nrgbd_conv_pack_weights(_p(w), _p(wp), cin, cout, taps, _stream(w))
    _lib.check(rc, "nrgbd_conv_pack_weights")
    return wp


def conv2d(x, w_packed, cout, dilation=1, x_ss=None, x_relu=False, res=None, res_ss=None, res_relu=False,
           materialize=False, bias=None, out_lrelu=False, want_stats=True):
    """Channels-last 3x3 convolution (stride 1, pad = dilation) on the fp32 matrix cores.

    x [N,H,W,Cin]; input = act(x*s+t) (+ act(res*s'+t')).  Returns (y [N,H,W,cout], stats | None, materialized | None).
    """
    x = _need(x, "x")
    N, H, W, Cin = x.shape
    y = torch.empty((N, H, W, cout), dtype=torch.float32, device=x.device)
    stats = torch.empty((conv2d_workgroups(N, H, W), 2 * cout), dtype=torch.float32, device=x.device) if want_stats else None
    mat = torch.empty_like(x) if materialize else None
    if res is not None:
        res = _need(res, "res", x.shape)
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_conv2d_3x3_f32(_p(x), _p(x_ss), int(x_relu), _p(res), _p(res_ss), int(res_relu), _p(mat),
                                               _p(w_packed), _p(bias), int(out_lrelu), _p(y), _p(stats), N, H, W, Cin,
                                               int(cout), int(dilation), _stream(x))
    _lib.check(rc, "nrgbd_conv2d_3x3_f32")
    return y, stats, mat


def conv_s2_pack(w, cp=None):
    """Weights of a stride-2, pad-1 3x3 convolution [Cout, C, 3, 3] -> packed stream of the equivalent 2x2-tap convolution on the
    space-to-depth input (nrgbd_conv2d_taps_f32, taps = 4): w2[co, (py*2+px)*C + c, ty, tx] with (ty, py) -> ky: (0,1) -> 0,
    (1,0) -> 1, (1,1) -> 2 and the same for x; (0,0) does not occur (zero).  cp = padded channel count (multiple of 16)."""
    w = _need(w, "w")
    return conv_pack_weights(conv_s2_weights(w, cp))


def conv_s2_weights(w, cp=None):
    """The re-indexing itself (any device): w [Cout, C, 3, 3] of a stride-2, pad-1 convolution -> w2 [Cout, cp, 2, 2] of the
    2x2-window convolution (window rows {y-1, y}, columns {x-1, x}) on the space-to-depth input."""
    cout, c = w.shape[:2]
    cp = cp or -(-4 * c // 16) * 16
    w2 = torch.zeros((cout, cp, 2, 2), dtype=w.dtype, device=w.device)
    kmap = {(0, 1): 0, (1, 0): 1, (1, 1): 2}
    for (ty, py), ky in kmap.items():
        for (tx, px), kx in kmap.items():
            ph = py * 2 + px
            w2[:, ph * c:(ph + 1) * c, ty, tx] = w[:, :, ky, kx]
    return w2


def space_to_depth2(x, nchw=False, cp=None):
    """[N,C,H,W] (nchw) or [N,H,W,C] -> [N,H/2,W/2,cp] with channel (py*2+px)*C + c = x[2y+py, 2x+px, c], zero-padded to cp."""
    x = _need(x, "x")
    if nchw:
        N, C, H, W = x.shape
    else:
        N, H, W, C = x.shape
    cp = cp or -(-4 * C // 16) * 16
    y = torch.empty((N, H // 2, W // 2, cp), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_space_to_depth2(_p(x), int(nchw), _p(y), N, C, H, W, cp, _stream(x))
    _lib.check(rc, "nrgbd_space_to_depth2")
    return y


def conv2d_taps(x, w_packed, cout, taps, x_ss=None, x_relu=False, want_stats=True, stride=1):
    """1x1 convolution (taps = 1) or the 2x2-window form of a stride-2 3x3 convolution on a space-to-depth input (taps = 4) on
    the matrix-core kernel, with the trunk's prologue and statistics epilogue: x [N,H,W,Cin] -> (y [N,H,W,cout], stats | None).
    stride > 1 (taps = 1 only): the 1x1 convolution's own stride — x [N,H*s,W*s,Cin] is read at every s-th pixel."""
    x = _need(x, "x")
    N, H, W, Cin = x.shape
    if stride != 1:
        if taps != 1 or H % stride or W % stride:
            raise ValueError("conv2d_taps: a stride needs taps = 1 and sides that are multiples of it")
        H, W = H // stride, W // stride
    y = torch.empty((N, H, W, cout), dtype=torch.float32, device=x.device)
    stats = torch.empty((conv2d_workgroups(N, H, W), 2 * cout), dtype=torch.float32, device=x.device) if want_stats else None
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_conv2d_taps_f32(_p(x), _p(x_ss), int(x_relu), _p(w_packed), _p(y), _p(stats), N, H, W, Cin,
                                                int(cout), int(taps), int(stride), _stream(x))
    _lib.check(rc, "nrgbd_conv2d_taps_f32")
    return y, stats


def conv2d_wgrad(x, gy, dilation=1):
    """Weight gradient of the channels-last 3x3 stride-1 convolution: x [N,H,W,Cin], gy [N,H,W,Cout] -> dW [Cout,Cin,3,3]."""
    x = _need(x, "x")
    N, H, W, Cin = x.shape
    gy = _need(gy, "gy")
    Cout = gy.shape[-1]
    if tuple(gy.shape[:3]) != (N, H, W):
        raise ValueError("conv2d_wgrad: gy %s does not match x %s" % (tuple(gy.shape), tuple(x.shape)))
    lib = _lib.load()
    nwg = int(lib.nrgbd_conv2d_wgrad_workgroups(N, H, W, Cin, Cout))
    _lib.check(min(nwg, 0), "nrgbd_conv2d_wgrad_workgroups")
    blocks = -(-Cout // 64) * -(-Cin // 64)
    partial = torch.empty(blocks * nwg * 9 * 64 * 64, dtype=torch.float32, device=x.device)
    dw = torch.empty((Cout, Cin, 3, 3), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.nrgbd_conv2d_wgrad_f32(_p(x), _p(gy), _p(partial), _p(dw), N, H, W, Cin, Cout, int(dilation), _stream(x))
    _lib.check(rc, "nrgbd_conv2d_wgrad_f32")
    return dw


def conv2d_rnet(x, w_packed, cout, bias=None, lrelu=True, out=None, ldy=None, ycoff=0, cout_valid=None, mode=0, pa=0, pb=0):
    """R-Net layer on the matrix cores (nrgbd_conv2d_rnet_f32).  x [N,H,W,Cin] channels-last.
    mode 0: 3x3 conv -> out[..., ycoff:ycoff+cout_valid] of a [N,H,W,ldy] buffer (allocated [N,H,W,cout_valid] if None);
    mode 1: sub-pixel phase (pa, pb) of ConvTranspose2d(k4,s2,p1) -> the same inside a [N,2H,2W,ldy] buffer (required);
    mode 2: conv + bias + log_softmax over the channels -> planar [N,cout,H,W];
    mode 3: all four phases of the transposed conv in one launch (w_packed = the phases' packed weights concatenated)."""
    x = _need(x, "x")
    N, H, W, Cin = x.shape
    cv = cout if cout_valid is None else cout_valid
    if mode == 2:
        out = torch.empty((N, cout, H, W), dtype=torch.float32, device=x.device)
        ldy = cout
    elif out is None:
        if mode in (1, 3):
            raise ValueError("conv2d_rnet: a transposed conv writes into a caller-provided [N,2H,2W,ldy] buffer")
        out = torch.empty((N, H, W, cv), dtype=torch.float32, device=x.device)
        ldy = cv
    elif ldy is None:
        ldy = out.shape[-1]
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_conv2d_rnet_f32(_p(x), _p(w_packed), _p(bias), int(bool(lrelu)), _p(out), int(ldy), int(ycoff),
                                                int(cv), int(mode), int(pa), int(pb), N, H, W, Cin, int(cout), _stream(x))
    _lib.check(rc, "nrgbd_conv2d_rnet_f32")
    return out


def rnet_pack(dpv_log, feat, feat_planar, out=None):
    """dpv_log [D,h,w] (log-prob), feat [h,w,Cf] (or [Cf,h,w] if feat_planar) -> [1,h,w,D+Cf] = cat(exp(dpv), feat)."""
    dpv_log = _need(dpv_log, "dpv_log")
    feat = _need(feat, "feat")
    D, h, w = dpv_log.shape
    Cf = feat.shape[0] if feat_planar else feat.shape[-1]
    if out is None:
        out = torch.empty((1, h, w, D + Cf), dtype=torch.float32, device=dpv_log.device)
    elif tuple(out.shape) != (1, h, w, D + Cf) or not out.is_contiguous():
        raise ValueError("rnet_pack: out must be a contiguous [1,h,w,D+Cf] tensor")
    with torch.cuda.device(dpv_log.device):
        rc = _lib.load().nrgbd_rnet_pack(_p(dpv_log), _p(feat), int(bool(feat_planar)), _p(out), D, Cf, h * w, _stream(dpv_log))
    _lib.check(rc, "nrgbd_rnet_pack")
    return out


def bn_finalize(stats, count, gamma, beta, eps, momentum, running_mean=None, running_var=None, status=None, batches_tracked=None):
    """Per-workgroup partials [nwg, 2C] -> scale_shift [C,2]; updates the running statistics in place (train mode)."""
    stats = _need(stats, "stats")
    C = stats.shape[1] // 2
    ss = torch.empty((C, 2), dtype=torch.float32, device=stats.device)
    with torch.cuda.device(stats.device):
        rc = _lib.load().nrgbd_bn_finalize(_p(stats), stats.shape[0], C, int(count), _p(gamma), _p(beta), float(eps),
                                           float(momentum), _p(running_mean), _p(running_var), _p(ss), _status_ptr(status, stats), _nbt_ptr(batches_tracked, stats),
                                           _stream(stats))
    _lib.check(rc, "nrgbd_bn_finalize")
    return ss


def bn_small_stats(xs, gammas, betas, eps, momentum, running_means=None, running_vars=None, batches_tracked=None):
    """Pivot-shifted float64 batch statistics of 1..4 small channels-last maps xs[i] [..., C] in one launch (nrgbd_bn_small_stats: the
    SPP branches) -> [scale_shift [C,2] per map]; updates the running statistics (unbiased variance) and batches_tracked in
    place where given.  eps, momentum: one value for all maps or one per map.  No collapse guard: nothing to report."""
    n = len(xs)
    if not 1 <= n <= 4 or len(gammas) != n or len(betas) != n:
        raise ValueError("bn_small_stats: 1 to 4 maps with one gamma and beta each, got %d / %d / %d" % (n, len(gammas), len(betas)))
    xs = [_need(x, "x") for x in xs]
    C = xs[0].shape[-1]
    if any(x.shape[-1] != C for x in xs):
        raise ValueError("bn_small_stats: the maps must share one channel count, got %s" % [tuple(x.shape) for x in xs])
    per = lambda v: [float(u) for u in v] if isinstance(v, (list, tuple)) else [float(v)] * n
    eps, momentum = per(eps), per(momentum)
    rms = list(running_means) if running_means is not None else [None] * n
    rvs = list(running_vars) if running_vars is not None else [None] * n
    nbts = list(batches_tracked) if batches_tracked is not None else [None] * n
    if len(eps) != n or len(momentum) != n or len(rms) != n or len(rvs) != n or len(nbts) != n:
        raise ValueError("bn_small_stats: one eps / momentum / running statistic per map")
    dev = xs[0].device
    ss = [torch.empty((C, 2), dtype=torch.float32, device=dev) for _ in range(n)]
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[0 if t is None else t.data_ptr() for t in ts])
    gammas = [_need(g, "gamma", (C,)) for g in gammas]
    betas = [_need(b, "beta", (C,)) for b in betas]
    for i in range(n):
        if (rms[i] is None) != (rvs[i] is None):
            raise ValueError("bn_small_stats: running_mean and running_var come together")
        for t, name in ((rms[i], "running_mean"), (rvs[i], "running_var")):
            if t is not None and _need(t, name, (C,)) is not t:
                raise ValueError("bn_small_stats: %s must be contiguous (it is updated in place)" % name)
        _nbt_ptr(nbts[i], xs[i])
    keep = (ptrs(xs), (ctypes.c_long * n)(*[x.numel() // C for x in xs]), ptrs(gammas), ptrs(betas), (ctypes.c_float * n)(*eps),
            (ctypes.c_float * n)(*momentum), ptrs(rms), ptrs(rvs), ptrs(nbts), ptrs(ss))
    with torch.cuda.device(dev):
        rc = _lib.load().nrgbd_bn_small_stats(n, *[ctypes.cast(a, ctypes.c_void_p) for a in keep[:2]], int(C),
                                          *[ctypes.cast(a, ctypes.c_void_p) for a in keep[2:]], _stream(xs[0]))
    _lib.check(rc, "nrgbd_bn_small_stats")
    return ss


def conv_wino_rnet(x, w_wino, cout, bias=None, lrelu=True, out=None, ycoff=0, cout_valid=None):
    """R-Net conv2d_leakyRelu block in the Winograd domain: x [N,H,W,Cin] -> leaky_relu(conv3x3(x) + bias).
    `cout` = columns of the packed weights (% 64, or 32: the HALF form, whose stream is the 64-column one with the upper half zero);
    `out` [N,H,W,ldy] may be wider than the layer (a concat buffer): output
    column c < cout_valid of a pixel lands at out[..., ycoff + c], the rest of the pixel is left alone."""
    x = _need(x, "x")
    N, H, W, Cin = x.shape
    valid = int(cout if cout_valid is None else cout_valid)
    if out is None:
        out = torch.empty((N, H, W, valid), dtype=torch.float32, device=x.device)
    elif tuple(out.shape[:3]) != (N, H, W) or not out.is_contiguous() or out.shape[3] < ycoff + valid:
        raise ValueError("conv_wino_rnet: out must be a contiguous [N,H,W,>= ycoff + cout_valid] tensor")
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_conv_wino_rnet_ex_f32(_p(x), _p(w_wino), _p(bias), int(bool(lrelu)), _p(out), N, H, W, Cin, int(cout),
                                                      int(out.shape[3]), int(ycoff), valid, _stream(x))
    _lib.check(rc, "nrgbd_conv_wino_rnet_ex_f32")
    return out


def deconv_phase_weights(w):
    """ConvTranspose2d(k4, s2, p1) weight [Cin, Cout, 4, 4] -> the four sub-pixel phases as 3x3 kernels (non-zero in a 2x2 corner)
    stacked phase-major along the output channels, [4 Cout, Cin, 3, 3], rows (2a + b) * Cout + co: the embedding of
    autograd.conv_transpose2d_module."""
    from .autograd import _tap_select
    cin, cout = w.shape[:2]
    idx, msk = _tap_select("t2", w.device)
    w4 = w.detach().permute(1, 0, 2, 3).reshape(cout, cin, 16).index_select(2, idx) * msk
    return w4.reshape(cout, cin, 4, 9).permute(2, 0, 1, 3).reshape(4 * cout, cin, 3, 3).contiguous()


def deconv_live_points(phase):
    """The 9 transform points xi = 4 xi_y + xi_x of F(2x2, 3x3) at which phase 2a + b of deconv_phase_weights is non-zero."""
    a, b = phase >> 1, phase & 1
    return [4 * (r + a) + c + b for r in range(3) for c in range(3)]


def conv_wino_rnet_deconv_pack(w_wino, Cin):
    """The 256-column stream conv_wino_pack makes of deconv_phase_weights (ONE 64-column slice: [256, Cin, 3, 3]) -> the masked
    stream of conv_wino_rnet_deconv, [4 phases][Cin/16 stages][9 live points][1024] floats (the dropped lines are exact zeros)."""
    w_wino = _need(w_wino, "w_wino")
    if w_wino.numel() != 256 * Cin * 16:
        raise ValueError("conv_wino_rnet_deconv_pack: a 256-column stream of %d input channels expected" % Cin)
    wm = torch.empty(4 * (Cin // 16) * 9 * 1024, dtype=torch.float32, device=w_wino.device)
    with torch.cuda.device(w_wino.device):
        rc = _lib.load().nrgbd_conv_wino_rnet_deconv_pack(_p(w_wino), _p(wm), int(Cin), _stream(w_wino))
    _lib.check(rc, "nrgbd_conv_wino_rnet_deconv_pack")
    return wm


def conv_wino_rnet_deconv_supported(N, H, W, Cin, ldy):
    """Shapes nrgbd_conv_wino_rnet_deconv_f32 accepts (per 64-column slice; the caller takes the direct kernel otherwise)."""
    return Cin >= 32 and Cin % 32 == 0 and N * H * W * Cin < (1 << 30) and 4 * N * H * W * ldy < (1 << 31)


def conv_wino_rnet_deconv(x, w_masked, out, bias=None, lrelu=True, ycoff=0, cout_valid=64):
    """ConvTranspose2d(k4, s2, p1) + bias + LeakyReLU(0.01) of one 64-column slice in the Winograd domain, dead transform points
    skipped: x [N,H,W,Cin] -> out[..., ycoff:ycoff+cout_valid] of a contiguous [N,2H,2W,ldy] buffer; the rest of a pixel is left alone."""
    x = _need(x, "x")
    N, H, W, Cin = x.shape
    if tuple(out.shape[:3]) != (N, 2 * H, 2 * W) or not out.is_contiguous() or out.shape[3] < ycoff + cout_valid:
        raise ValueError("conv_wino_rnet_deconv: out must be a contiguous [N,2H,2W,>= ycoff + cout_valid] tensor")
    if w_masked.numel() != 4 * (Cin // 16) * 9 * 1024:
        raise ValueError("conv_wino_rnet_deconv: the masked stream does not belong to %d input channels" % Cin)
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_conv_wino_rnet_deconv_f32(_p(x), _p(w_masked), _p(bias), int(bool(lrelu)), _p(out), N, H, W, Cin, 64,
                                                          int(out.shape[3]), int(ycoff), int(cout_valid), _stream(x))
    _lib.check(rc, "nrgbd_conv_wino_rnet_deconv_f32")
    return out


def conv2d_few(x, w_few, bias=None, lrelu=True, out=None, ycoff=0):
    """3x3 convolution with 1-4 output channels on the vector ALUs (nrgbd_conv2d_few_f32): x [N,H,W,ldx] channels-last, w_few
    [Cin/16, 9, Cout, 16] (= w [Cout, Cin, 3, 3] with ci -> (block, lane) and (ky, kx) -> tap; Cin % 16 == 0 <= ldx) ->
    out[..., ycoff:ycoff+Cout] of a contiguous [N,H,W,ldy] buffer (allocated [N,H,W,Cout] if None)."""
    x = _need(x, "x")
    w_few = _need(w_few, "w_few")
    N, H, W, ldx = x.shape
    nblk, taps, cout, lanes = w_few.shape
    if taps != 9 or lanes != 16 or not 1 <= cout <= 4 or nblk * 16 > ldx:
        raise ValueError("conv2d_few: w_few %s for an input of %d channels" % (tuple(w_few.shape), ldx))
    if out is None:
        out = torch.empty((N, H, W, cout), dtype=torch.float32, device=x.device)
    elif tuple(out.shape[:3]) != (N, H, W) or not out.is_contiguous() or out.shape[3] < ycoff + cout:
        raise ValueError("conv2d_few: out must be a contiguous [N,H,W,>= ycoff + Cout] tensor")
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_conv2d_few_f32(_p(x), int(ldx), _p(w_few), _p(bias), int(bool(lrelu)), _p(out), int(out.shape[3]), int(ycoff),
                                               N, H, W, nblk * 16, cout, _stream(x))
    _lib.check(rc, "nrgbd_conv2d_few_f32")
    return out


def bn_cl_supported(rows, C):
    """Shapes of the channels-last train-mode BatchNorm kernels (bn_train.hip): 16-byte channel quads that tile a 256-lane workgroup."""
    return rows > 0 and 4 <= C <= 1024 and C % 4 == 0 and 256 % (C // 4) == 0


def bn_cl_fwd(x, gamma, beta, eps, relu, residual=None, momentum=0.0, running_mean=None, running_var=None):
    """y = act(batchnorm(x)) + residual with batch statistics over the rows of x [rows, C] (contiguous, channels last).
    Returns (y, coef [4,C] = scale, shift, mean, invstd); updates the running statistics in place when given."""
    x = _need(x, "x")
    rows, C = x.shape
    if residual is not None:
        residual = _need(residual, "residual", (rows, C))
    y = torch.empty_like(x)
    coef = torch.empty((4, C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        lib = _lib.load()
        G = lib.nrgbd_bn_cl_workgroups(rows, C)
        _lib.check(min(G, 0), "nrgbd_bn_cl_workgroups")
        partial = torch.empty((G, 2 * C), dtype=torch.float32, device=x.device)
        rc = lib.nrgbd_bn_cl_fwd(_p(x), _p(residual), _p(_need(gamma, "gamma", (C,))), _p(_need(beta, "beta", (C,))), float(eps),
                                 float(momentum), _p(running_mean), _p(running_var), int(bool(relu)), _p(y), _p(coef), _p(partial),
                                 rows, C, _stream(x))
    _lib.check(rc, "nrgbd_bn_cl_fwd")
    return y, coef


def bn_cl_bwd(x, gy, coef, relu):
    """Backward of bn_cl_fwd w.r.t. (x, gamma, beta): gx [rows, C], g_gamma [C], g_beta [C] (the residual's gradient is gy)."""
    x = _need(x, "x")
    rows, C = x.shape
    gy = _need(gy, "gy", (rows, C))
    coef = _need(coef, "coef", (4, C))
    gx = torch.empty_like(x)
    gg = torch.empty((2, C), dtype=torch.float32, device=x.device)
    coef2 = torch.empty((2, C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        lib = _lib.load()
        G = lib.nrgbd_bn_cl_workgroups(rows, C)
        _lib.check(min(G, 0), "nrgbd_bn_cl_workgroups")
        partial = torch.empty((G, 2 * C), dtype=torch.float32, device=x.device)
        rc = lib.nrgbd_bn_cl_bwd(_p(x), _p(gy), _p(coef), int(bool(relu)), _p(gx), _p(gg[0]), _p(gg[1]), _p(coef2), _p(partial),
                                 rows, C, _stream(x))
    _lib.check(rc, "nrgbd_bn_cl_bwd")
    return gx, gg[0], gg[1]


def bn_finalize_cm(stats, count, gamma, beta, eps, momentum, running_mean=None, running_var=None, status=None, batches_tracked=None):
    """Column-major per-tile partials [2C, rows] (conv_wino) -> scale_shift [C,2]; updates the running statistics in place."""
    stats = _need(stats, "stats")
    C = stats.shape[0] // 2
    ss = torch.empty((C, 2), dtype=torch.float32, device=stats.device)
    with torch.cuda.device(stats.device):
        rc = _lib.load().nrgbd_bn_finalize_cm(_p(stats), stats.shape[1], C, int(count), _p(gamma), _p(beta), float(eps),
                                              float(momentum), _p(running_mean), _p(running_var), _p(ss), _status_ptr(status, stats), _nbt_ptr(batches_tracked, stats),
                                              _stream(stats))
    _lib.check(rc, "nrgbd_bn_finalize_cm")
    return ss


def logsoftmax_rows(x, inplace=True):
    """log_softmax over the last (channel) axis of a contiguous channels-last tensor [..., C], C in {64, 128, 256} (nrgbd_logsoftmax_rows)."""
    x = _need(x, "x")
    C = x.shape[-1]
    y = x if inplace else torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_logsoftmax_rows(_p(x), _p(y), x.numel() // C, int(C), _stream(x))
    _lib.check(rc, "nrgbd_logsoftmax_rows")
    return y


def logsoftmax_d_bwd(logp, g, scale=1.0):
    """Backward of logsoftmax_d: scale * (g - exp(logp) * sum_k g) on planar [D, ...] volumes (nrgbd_logsoftmax_d_bwd)."""
    logp = _need(logp, "logp")
    g = _need(g, "g", logp.shape)
    D = logp.shape[0]
    gz = torch.empty_like(logp)
    with torch.cuda.device(logp.device):
        rc = _lib.load().nrgbd_logsoftmax_d_bwd(_p(logp), _p(g), float(scale), _p(gz), D, logp.numel() // D, _stream(logp))
    _lib.check(rc, "nrgbd_logsoftmax_d_bwd")
    return gz


def logsoftmax_rows_bwd(y, g):
    """Backward of logsoftmax_rows on contiguous channels-last tensors [..., C], C in {64, 128, 256} (nrgbd_logsoftmax_rows_bwd)."""
    y = _need(y, "y")
    g = _need(g, "g", y.shape)
    C = y.shape[-1]
    gx = torch.empty_like(y)
    with torch.cuda.device(y.device):
        rc = _lib.load().nrgbd_logsoftmax_rows_bwd(_p(y), _p(g), _p(gx), y.numel() // C, int(C), _stream(y))
    _lib.check(rc, "nrgbd_logsoftmax_rows_bwd")
    return gx


def _nll_target(target, n):
    if not (isinstance(target, torch.Tensor) and target.is_cuda and target.dtype == torch.int64):
        raise TypeError("target must be an int64 tensor on the GPU")
    if target.numel() != n:
        raise ValueError("target has %d elements, the volume %d pixels" % (target.numel(), n))
    return target if target.is_contiguous() else target.contiguous()


def nll_fwd(logp, target, ignore_index, channels_last):
    """Mean NLL of a [D, n] (planar) or [n, D] (channels_last) log-probability volume -> stat [2] = (loss, counted pixels)
    (nrgbd_nll_fwd; a device tensor: no host synchronisation)."""
    logp = _need(logp, "logp")
    D = logp.shape[-1] if channels_last else logp.shape[0]
    n = logp.numel() // D
    target = _nll_target(target, n)
    lib = _lib.load()
    partial = torch.empty((lib.nrgbd_nll_workgroups(n), 2), dtype=torch.float32, device=logp.device)
    stat = torch.empty(2, dtype=torch.float32, device=logp.device)
    with torch.cuda.device(logp.device):
        rc = lib.nrgbd_nll_fwd(_p(logp), ctypes.c_void_p(target.data_ptr()), int(ignore_index), int(D), n, int(bool(channels_last)),
                               _p(partial), _p(stat), _stream(logp))
    _lib.check(rc, "nrgbd_nll_fwd")
    return stat


def nll_bwd(target, ignore_index, g_out, stat, shape, channels_last):
    """Gradient of nll_fwd w.r.t. logp, in logp's layout `shape` ([D, ...] or [..., D]) (nrgbd_nll_bwd)."""
    g_out = _need(g_out, "g_out").reshape(1)
    stat = _need(stat, "stat", (2,))
    D = shape[-1] if channels_last else shape[0]
    g = torch.empty(tuple(shape), dtype=torch.float32, device=stat.device)
    n = g.numel() // D
    target = _nll_target(target, n)
    with torch.cuda.device(stat.device):
        rc = _lib.load().nrgbd_nll_bwd(ctypes.c_void_p(target.data_ptr()), int(ignore_index), _p(g_out), _p(stat), _p(g), int(D), n,
                                       int(bool(channels_last)), _stream(stat))
    _lib.check(rc, "nrgbd_nll_bwd")
    return g


def bias_lrelu_cl_fwd(x, bias, slope):
    """y = leaky_relu(x + bias, slope) on channels-last rows x [rows, C] (nrgbd_bias_lrelu_cl_fwd)."""
    x = _need(x, "x")
    rows, C = x.shape
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_bias_lrelu_cl_fwd(_p(x), _p(_need(bias, "bias", (C,))), float(slope), _p(y), rows, C, _stream(x))
    _lib.check(rc, "nrgbd_bias_lrelu_cl_fwd")
    return y


def bias_lrelu_cl_bwd(y, gy, slope):
    """Backward of bias_lrelu_cl_fwd from its OUTPUT y: (gx [rows, C], g_bias [C])."""
    y = _need(y, "y")
    rows, C = y.shape
    gy = _need(gy, "gy", (rows, C))
    gx = torch.empty_like(y)
    gb = torch.empty((C,), dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        lib = _lib.load()
        G = lib.nrgbd_bias_lrelu_cl_workgroups(rows, C)
        _lib.check(min(G, 0), "nrgbd_bias_lrelu_cl_workgroups")
        partial = torch.empty((G, C), dtype=torch.float32, device=y.device)
        rc = lib.nrgbd_bias_lrelu_cl_bwd(_p(y), _p(gy), float(slope), _p(gx), _p(gb), _p(partial), rows, C, _stream(y))
    _lib.check(rc, "nrgbd_bias_lrelu_cl_bwd")
    return gx, gb


def upsample_bilinear_ac(x, H, W, backward=False):
    """Bilinear up-sampling (align_corners=True) of a channels-last map x [N,bh,bw,C] -> [N,H,W,C] (nrgbd_upsample_bilinear_ac);
    backward=True: x is the gradient of the output [N,H2,W2,C] and (H, W) the INPUT size -> gradient of the input [N,H,W,C]."""
    x = _need(x, "x")
    N, a, b, C = x.shape
    y = torch.empty((N, H, W, C), dtype=torch.float32, device=x.device)
    bh, bw, Ho, Wo = (H, W, a, b) if backward else (a, b, H, W)
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_upsample_bilinear_ac(_p(x), _p(y), N, bh, bw, Ho, Wo, C, int(backward), _stream(x))
    _lib.check(rc, "nrgbd_upsample_bilinear_ac")
    return y


def spp_concat(quarter, deep, branches):
    """[quarter | deep | up(relu(bn(z_0))) | ... | up(relu(bn(z_3)))] -> [N,h,w,Cq+Cd+4*Cb] in one pass (nrgbd_spp_concat).
    quarter [N,h,w,Cq], deep [N,h,w,Cd] channels-last; branches: four (z [N,bh,bw,Cb] raw 1x1-conv output, ss [Cb,2]) in the
    concat's order; up = bilinear, align_corners=True (psm_submodule.py:149-161)."""
    quarter, deep = _need(quarter, "quarter"), _need(deep, "deep")
    N, h, w, Cq = quarter.shape
    Cd = deep.shape[3]
    if tuple(deep.shape[:3]) != (N, h, w) or len(branches) != 4:
        raise ValueError("spp_concat: quarter %s / deep %s / %d branches" % (tuple(quarter.shape), tuple(deep.shape), len(branches)))
    Cb = branches[0][0].shape[3]
    args = []
    for z, ss in branches:
        z, ss = _need(z, "branch"), _need(ss, "branch scale/shift", (Cb, 2))
        if z.shape[0] != N or z.shape[3] != Cb:
            raise ValueError("spp_concat: branch %s" % (tuple(z.shape),))
        args += [_p(z), _p(ss), int(z.shape[1]), int(z.shape[2])]
    out = torch.empty((N, h, w, Cq + Cd + 4 * Cb), dtype=torch.float32, device=quarter.device)
    with torch.cuda.device(quarter.device):
        rc = _lib.load().nrgbd_spp_concat(_p(quarter), Cq, _p(deep), Cd, *args, Cb, _p(out), N, h, w, _stream(quarter))
    _lib.check(rc, "nrgbd_spp_concat")
    return out


def nhwc_stats(x):
    """Per-workgroup (sum, sum of squares) partials of a channels-last tensor [..., C] -> [nwg, 2C]."""
    x = _need(x, "x")
    C = x.shape[-1]
    P = x.numel() // C
    nwg = int(_lib.load().nrgbd_nhwc_stats_workgroups(P))
    stats = torch.empty((nwg, 2 * C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_nhwc_stats(_p(x), P, C, _p(stats), _stream(x))
    _lib.check(rc, "nrgbd_nhwc_stats")
    return stats


def nhwc_act(x, x_ss=None, x_relu=False, res=None, res_ss=None, res_relu=False, out=None, ldy=None):
    """y = act(x*s+t) (+ act(res*s'+t')) on channels-last [..., C]; `out` may be a wider buffer (pixel stride ldy)."""
    x = _need(x, "x")
    C = x.shape[-1]
    P = x.numel() // C
    if res is not None:
        res = _need(res, "res", x.shape)
    if out is None:
        out, ldy = torch.empty_like(x), C
    elif ldy is None:
        raise ValueError("nhwc_act: out needs its pixel stride ldy")
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_nhwc_act(_p(x), _p(x_ss), int(x_relu), _p(res), _p(res_ss), int(res_relu), _p(out), P, C,
                                         int(ldy), _stream(x))
    _lib.check(rc, "nrgbd_nhwc_act")
    return out


def nhwc_act_lean(x, x_ss=None, x_relu=False, res=None, res_ss=None, res_relu=False, out=None, ldy=None, wg_per_cu=1):
    """nhwc_act with the same bits from the co-resident form of the kernel: wg_per_cu workgroups of four waves per CU (1 = meant
    to share the CUs with a convolution of another stream; up to 8 when it runs alone).  C a power of two."""
    x = _need(x, "x")
    C = x.shape[-1]
    P = x.numel() // C
    if res is not None:
        res = _need(res, "res", x.shape)
    if out is None:
        out, ldy = torch.empty_like(x), C
    elif ldy is None:
        raise ValueError("nhwc_act_lean: out needs its pixel stride ldy")
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_nhwc_act_lean(_p(x), _p(x_ss), int(x_relu), _p(res), _p(res_ss), int(res_relu), _p(out), P, C,
                                              int(ldy), int(wg_per_cu), _stream(x))
    _lib.check(rc, "nrgbd_nhwc_act_lean")
    return out


def bn2d_train_act(x, gamma, beta, eps, relu=False, residual=None, inplace=True, want_mean_var=False):
    """Train-mode BatchNorm2d + activation (+ residual) in two HBM passes.  x [N,C,H,W] -> (y, mean_var | None)."""
    x = _need(x, "x")
    N, C, H, W = x.shape
    if residual is not None:
        residual = _need(residual, "residual", x.shape)
    y = x if inplace else torch.empty_like(x)
    partial = torch.empty(int(_lib.load().nrgbd_bn2d_partial_floats(C)), dtype=torch.float32, device=x.device)
    mv = torch.empty((C, 2), dtype=torch.float32, device=x.device) if want_mean_var else None
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_bn2d_train_act(_p(x), _p(gamma), _p(beta), float(eps), int(bool(relu)), _p(residual),
                                               _p(y), _p(partial), _p(mv), N, C, H * W, _stream(x))
    _lib.check(rc, "nrgbd_bn2d_train_act")
    return y, mv


def avgpool8(x):
    """8x8 / stride-8 average pooling of [N,C,H,W]."""
    x = _need(x, "x")
    N, C, H, W = x.shape
    y = torch.empty((N, C, H // 8, W // 8), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_avgpool8(_p(x), _p(y), N * C, H, W, _stream(x))
    _lib.check(rc, "nrgbd_avgpool8")
    return y


def avgpool_cl(x, k):
    """k x k / stride-k average pooling of a channels-last map x [N,H,W,C] -> [N,H//k,W//k,C] (nrgbd_avgpool_cl; floor like avg_pool2d)."""
    x = _need(x, "x")
    N, H, W, C = x.shape
    y = torch.empty((N, H // k, W // k, C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_avgpool_cl(_p(x), _p(y), N, H, W, C, int(k), _stream(x))
    _lib.check(rc, "nrgbd_avgpool_cl")
    return y


def scatter_channels(src, dst, coff):
    """dst[r, y, x, coff + c] = src[c, y, x] for every image r of the channels-last buffer dst [R,H,W,ldy]; src is any strided
    [C,H,W] view (NCHW planes or a permuted channels-last tensor) (nrgbd_scatter_channels)."""
    src = _need(src, "src", strided=True)
    dst = _need(dst, "dst", strided=True)
    C, H, W = src.shape
    if dst.dim() != 4 or tuple(dst.shape[1:3]) != (H, W) or not dst.is_contiguous() or dst.shape[3] < coff + C:
        raise ValueError("scatter_channels: dst must be a contiguous [R,%d,%d,>= %d] tensor" % (H, W, coff + C))
    with torch.cuda.device(src.device):
        rc = _lib.load().nrgbd_scatter_channels(_p(src), src.stride(0), src.stride(1), src.stride(2), C, H, W, _p(dst),
                                                 int(dst.shape[3]), int(coff), int(dst.shape[0]), int(dst.stride(0)), _stream(src))
    _lib.check(rc, "nrgbd_scatter_channels")
    return dst


def bias_act_(x, bias, slope):
    """In place x = leaky_relu(x + bias[c], slope) on a contiguous [N,C,H,W] tensor (slope 1 = bias add only)."""
    x = _need(x, "x", strided=True)
    if not x.is_contiguous():
        raise ValueError("bias_act_ needs a contiguous NCHW tensor")
    N, C, H, W = x.shape
    bias = _need(bias, "bias", (C,))
    with torch.cuda.device(x.device):
        rc = _lib.load().nrgbd_bias_act_nchw(_p(x), _p(bias), float(slope), N, C, H * W, _stream(x))
    _lib.check(rc, "nrgbd_bias_act_nchw")
    return x


# ---- the video stream's frame ingest and window assembly (ingest.hip; neuralrgbd_amd/video.py) -------------------------------

LAYOUT = {"hwc": 0, "chw": 1}        # layout flag of nrgbd_frame_ingest_u8


def frame_ingest(frame, dst, mean, std, layout="hwc"):
    """One uint8 CUDA frame ([Hin,Win,3] for layout "hwc", [3,Hin,Win] for "chw"; rows may be padded: any row stride) -> dst, a
    contiguous 16-byte aligned fp32 [3,Hout,Wout] view (a slot of a frame ring), as ((u / 255 - mean_c) / std_c) with a nearest
    resize when the sizes differ (nrgbd_frame_ingest_u8: ToTensor + Normalize + PIL NEAREST of the loaders, bit for bit).
    Returns dst."""
    if layout not in LAYOUT:
        raise ValueError("frame_ingest: layout %r, expected 'hwc' or 'chw'" % (layout,))
    if not isinstance(frame, torch.Tensor):
        raise TypeError("frame must be a torch.Tensor")
    if not frame.is_cuda:
        raise _lib.NrgbdError("frame is on %s: the frame ingest runs on the GPU only (no CPU fallback)" % (frame.device,))
    if frame.dtype != torch.uint8:
        raise TypeError("frame must be uint8, got %s" % frame.dtype)
    hwc = layout == "hwc"
    if frame.dim() != 3 or frame.shape[2 if hwc else 0] != 3:
        raise ValueError("frame_ingest: frame %s is not %s" % (tuple(frame.shape), "[H,W,3]" if hwc else "[3,H,W]"))
    Hin, Win = (frame.shape[0], frame.shape[1]) if hwc else (frame.shape[1], frame.shape[2])
    # rows of any pitch are read in place; anything else (a permuted or sliced view) is made contiguous first
    if hwc:
        ok = frame.stride(2) == 1 and frame.stride(1) == 3 and (frame.stride(0) >= 3 * Win or Hin == 1)
        pitch = frame.stride(0) if Hin > 1 else 3 * Win
    else:
        ok = frame.stride(2) == 1 and (frame.stride(1) >= Win or Hin == 1) and frame.stride(0) == Hin * frame.stride(1)
        pitch = frame.stride(1) if Hin > 1 else Win
    if not ok:
        frame = frame.contiguous()
        pitch = 3 * Win if hwc else Win
    dst = _need(dst, "dst", strided=True)
    if dst.dim() != 3 or dst.shape[0] != 3 or not dst.is_contiguous() or dst.device != frame.device:
        raise ValueError("frame_ingest: dst must be a contiguous [3,Hout,Wout] tensor on the frame's device, got %s" % (tuple(dst.shape),))
    mean, std = [float(m) for m in mean], [float(s) for s in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("frame_ingest: mean and std take three values each")
    with torch.cuda.device(dst.device):
        rc = _lib.load().nrgbd_frame_ingest_u8(_p(frame), int(Hin), int(Win), int(pitch), LAYOUT[layout], mean[0], mean[1], mean[2],
                                               std[0], std[1], std[2], _p(dst), int(dst.shape[1]), int(dst.shape[2]), _stream(dst))
    _lib.check(rc, "nrgbd_frame_ingest_u8")
    return dst


def window_gather(ring, slots, src=None, ref=None):
    """ring [R,3,H,W] (images contiguous, any slot stride), slots = the V ring slots of the sources in window order followed by the
    slot of the reference -> (src [V,3,H,W], ref [3,H,W]) in one launch (nrgbd_window_gather; bit-equal to torch.stack of the
    slots).  src / ref: optional contiguous output buffers."""
    ring = _need(ring, "ring", strided=True)
    if ring.dim() != 4 or ring.shape[1] != 3 or not ring[0].is_contiguous():
        raise ValueError("window_gather: ring %s must be [R,3,H,W] with contiguous images" % (tuple(ring.shape),))
    R, _, H, W = ring.shape
    slots = [int(s) for s in slots]
    V = len(slots) - 1
    if V < 1 or V > _lib.GATHER_MAX_V:
        raise ValueError("window_gather: %d source slots, expected 1 .. %d" % (V, _lib.GATHER_MAX_V))
    if min(slots) < 0 or max(slots) >= R:
        raise ValueError("window_gather: slots %s outside the ring of %d" % (slots, R))
    if src is None:
        src = torch.empty((V, 3, H, W), dtype=torch.float32, device=ring.device)
    if ref is None:
        ref = torch.empty((3, H, W), dtype=torch.float32, device=ring.device)
    src, ref = _need(src, "src", strided=True), _need(ref, "ref", strided=True)
    if src.numel() != V * 3 * H * W or ref.numel() != 3 * H * W or not src.is_contiguous() or not ref.is_contiguous():
        raise ValueError("window_gather: src %s / ref %s must be contiguous buffers of %s / %s"
                         % (tuple(src.shape), tuple(ref.shape), (V, 3, H, W), (3, H, W)))
    st = _lib.WindowSlots()
    for i, s in enumerate(slots):
        st.idx[i] = s
    with torch.cuda.device(ring.device):
        rc = _lib.load().nrgbd_window_gather(_p(ring), int(R), int(ring.stride(0)) if R > 1 else 3 * H * W, st, V, _p(src), _p(ref),
                                             int(H), int(W), _stream(ring))
    _lib.check(rc, "nrgbd_window_gather")
    return src, ref


# ---- the training stream's depth-label ingest (depth_ingest.hip; neuralrgbd_amd/train_video.py) ------------------------------

def _i32_table(t, name, n, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != dev or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise ValueError("depth_ingest: %s must be a contiguous int32 tensor of %d entries on %s" % (name, n, dev))
    return t


def depth_ingest(depth, tables, depth_scale, thr_q, thr_full, labels_q=None, labels_full=None, dmap_raw=None, dmap_imgsize=None):
    """One uint16 CUDA depth frame [Hin,Win] (torch.uint16, or the same bits as int16; rows may be padded: any row stride) -> the
    given outputs, in one launch (nrgbd_depth_ingest_u16: the loaders' depth preparation, mdataloader/scanNet.py:372-422, bit for bit).
    tables: the six int32 device tables (rows_full [H], cols_full [W], rows_q [h], cols_q [w], mask_rows_q [h], mask_cols_q [w]);
    thr_q / thr_full: host int32 thresholds (train_video.label_thresholds).  labels_q [h,w] / labels_full [H,W] int64 and dmap_raw [h,w]
    / dmap_imgsize [H,W] fp32: contiguous CUDA tensors (a leading 1 is accepted) or None = not computed; at least one is given.
    Returns (labels_q, labels_full, dmap_raw, dmap_imgsize)."""
    if not isinstance(depth, torch.Tensor):
        raise TypeError("depth must be a torch.Tensor")
    if not depth.is_cuda:
        raise _lib.NrgbdError("depth is on %s: the depth ingest runs on the GPU only (no CPU fallback)" % (depth.device,))
    if depth.dtype not in (torch.uint16, torch.int16):
        raise TypeError("depth must be uint16 (or its bits as int16), got %s" % depth.dtype)
    if depth.dim() != 2:
        raise ValueError("depth_ingest: depth %s is not [Hin,Win]" % (tuple(depth.shape),))
    Hin, Win = depth.shape
    if depth.stride(1) != 1 or (Hin > 1 and depth.stride(0) < Win):
        depth = depth.contiguous()
    pitch = depth.stride(0) if Hin > 1 else Win
    dev = depth.device
    if len(tables) != 6:
        raise ValueError("depth_ingest: six index tables, got %d" % len(tables))
    H, W, h, w = (int(tables[i].numel()) if isinstance(tables[i], torch.Tensor) else -1 for i in (0, 1, 2, 3))
    names = ("rows_full", "cols_full", "rows_q", "cols_q", "mask_rows_q", "mask_cols_q")
    tables = [_i32_table(t, nm, n, dev) for t, nm, n in zip(tables, names, (H, W, h, w, h, w))]
    outs = []
    for t, nm, dt, shape in ((labels_q, "labels_q", torch.int64, (h, w)), (labels_full, "labels_full", torch.int64, (H, W)),
                             (dmap_raw, "dmap_raw", torch.float32, (h, w)), (dmap_imgsize, "dmap_imgsize", torch.float32, (H, W))):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != dev or not t.is_contiguous()
                              or tuple(t.shape) not in (shape, (1,) + shape)):
            raise ValueError("depth_ingest: %s must be a contiguous %s tensor %s on %s" % (nm, dt, shape, dev))
        outs.append(t)
    if all(t is None for t in outs):
        raise ValueError("depth_ingest: no output given")
    thr = []
    for t, nm in ((thr_q, "thr_q"), (thr_full, "thr_full")):
        a = np.ascontiguousarray(t, dtype=np.int32)
        if a.ndim != 1 or not 1 <= a.size <= _lib.DEPTH_MAX_THRESHOLDS:
            raise ValueError("depth_ingest: %s holds %s thresholds, expected 1 .. %d" % (nm, a.shape, _lib.DEPTH_MAX_THRESHOLDS))
        thr.append(a)
    with torch.cuda.device(dev):
        rc = _lib.load().nrgbd_depth_ingest_u16(
            _p(depth), int(Hin), int(Win), int(pitch), *(_p(t) for t in tables), float(depth_scale),
            ctypes.c_void_p(thr[0].ctypes.data), int(thr[0].size), ctypes.c_void_p(thr[1].ctypes.data), int(thr[1].size),
            *(_p(t) for t in outs), H, W, h, w, _stream(depth))
    _lib.check(rc, "nrgbd_depth_ingest_u16")
    return tuple(outs)


# ---- on-device depth evaluation (depth_eval.hip; neuralrgbd_amd/evaluate.py) ----------------------------------------------------

def depth_eval_workgroups(n):
    """Partial records nrgbd_depth_eval writes for n pixels (needs no GPU)."""
    rc = _lib.load().nrgbd_depth_eval_workgroups(int(n))
    if rc < 0:
        _lib.check(rc, "nrgbd_depth_eval_workgroups")
    return rc


def depth_eval_workspace(n, J):
    """Bytes of workspace nrgbd_depth_eval needs for n pixels and J confidence sets (needs no GPU)."""
    rc = _lib.load().nrgbd_depth_eval_workspace(int(n), int(J))
    if rc < 0:
        _lib.check(rc, "nrgbd_depth_eval_workspace")
    return rc


def _eval_record(t, name, dtype, shape, dev):
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != dev or not t.is_contiguous() or tuple(t.shape) != shape):
        raise ValueError("depth_eval: %s must be a contiguous %s tensor %s on %s" % (name, dtype, shape, dev))
    return t


def depth_eval(depth, logconf, gt, log_thr, gt_range, workspace, frame, total=None, err_map=None):
    """One depth map against its ground truth (nrgbd_depth_eval: replaces the host evaluation of test_utils/export_res.py:108-116).
    depth / logconf / gt: contiguous CUDA fp32 tensors of one shape (the two maps of depth_regress, metres with 0 = a hole);
    log_thr: host fp32 [J], ascending from -inf; gt_range = (gt_min, gt_max); workspace: a CUDA tensor of at least
    depth_eval_workspace(n, J) bytes; frame / total: (sums float64 [J,6], counts int64 [J,4], header int64 [4]) — frame is written,
    total (or None) is added to; err_map: fp32 of the maps' shape or None.  Two launches, nothing allocated, nothing synchronised."""
    depth = _need(depth, "depth", strided=True)
    dev, shape = depth.device, tuple(depth.shape)
    for t, nm in ((depth, "depth"), (logconf, "logconf"), (gt, "gt")) + (((err_map, "err_map"),) if err_map is not None else ()):
        t = _need(t, nm, shape, strided=True)
        if t.device != dev or not t.is_contiguous():
            raise ValueError("depth_eval: %s must be contiguous and on %s" % (nm, dev))
    thr = np.ascontiguousarray(log_thr, dtype=np.float32)
    if thr.ndim != 1 or not 1 <= thr.size <= _lib.DEPTH_EVAL_MAX_SETS:
        raise ValueError("depth_eval: log_thr holds %s thresholds, expected 1 .. %d" % (thr.shape, _lib.DEPTH_EVAL_MAX_SETS))
    J = int(thr.size)
    if not isinstance(workspace, torch.Tensor) or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("depth_eval: workspace must be a contiguous tensor on %s" % (dev,))
    recs = []
    for rec, nm in ((frame, "frame"), (total, "total")):
        if rec is None and nm == "total":
            recs += [None, None, None]
            continue
        if rec is None or len(rec) != 3:
            raise ValueError("depth_eval: %s is (sums, counts, header)" % nm)
        recs += [_eval_record(rec[0], nm + " sums", torch.float64, (J, 6), dev), _eval_record(rec[1], nm + " counts", torch.int64, (J, 4), dev),
                 _eval_record(rec[2], nm + " header", torch.int64, (4,), dev)]
    with torch.cuda.device(dev):
        rc = _lib.load().nrgbd_depth_eval(_p(depth), _p(logconf), _p(gt), depth.numel(), float(gt_range[0]), float(gt_range[1]),
                                          ctypes.c_void_p(thr.ctypes.data), J, _p(workspace), workspace.numel() * workspace.element_size(),
                                          *(_p(t) for t in recs), _p(err_map), _stream(depth))
    _lib.check(rc, "nrgbd_depth_eval")


# ---- the guided-filter refinement net (dgf.hip; neuralrgbd_amd/nets.py: DGFRefineNet) -------------------------------------------

DGF_TILE = _lib.DGF_TILE        # (rows, columns) of the image tile a workgroup of nrgbd_dgf_refine_f32 owns


def dgf_refine(depth_lr, img, w1, b1, w2, b2, eps=1e-8, out=None):
    """The DGF refinement of n in {1, 2} low-resolution depth maps under one guide image, one launch (nrgbd_dgf_refine_f32: replaces
    Refine.py:620-641, GF/guided_filter.py:54-97 and GF/box_filter.py).
    depth_lr [n,h,w] or [n,1,h,w]; img [3,H,W] or [1,3,H,W] with H = s h, W = s w, s >= 2; w1 / b1 / w2 / b2: the parameters of
    Conv2d(3, 64, 1) and Conv2d(64, 1, 1) in any shape of 192 / 64 / 64 / 1 contiguous elements (read in place).
    Returns [n,1,H,W]; `out`: a contiguous fp32 tensor of n H W elements to write into instead (any alignment)."""
    depth_lr, img = _need(depth_lr, "depth_lr"), _need(img, "img")
    if depth_lr.dim() == 4 and depth_lr.shape[1] == 1:
        depth_lr = depth_lr[:, 0]
    if img.dim() == 4 and img.shape[0] == 1:
        img = img[0]
    if depth_lr.dim() != 3 or img.dim() != 3 or img.shape[0] != 3:
        raise ValueError("dgf_refine: depth_lr [n,h,w] and img [3,H,W], got %s and %s" % (tuple(depth_lr.shape), tuple(img.shape)))
    n, h, w = depth_lr.shape
    H, W = img.shape[1:]
    params = []
    for t, nm, numel in ((w1, "w1", 192), (b1, "b1", 64), (w2, "w2", 64), (b2, "b2", 1)):
        t = _need(t, nm)
        if t.numel() != numel or t.device != img.device:
            raise ValueError("dgf_refine: %s holds %d elements on %s, expected %d on %s" % (nm, t.numel(), t.device, numel, img.device))
        params.append(t)
    if depth_lr.device != img.device:
        raise ValueError("dgf_refine: depth_lr on %s, img on %s" % (depth_lr.device, img.device))
    if out is None:
        out = torch.empty((n, 1, H, W), dtype=torch.float32, device=img.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != img.device or not out.is_contiguous()
          or out.numel() != n * H * W):
        raise ValueError("dgf_refine: out must be a contiguous float32 tensor of %d elements on %s" % (n * H * W, img.device))
    with torch.cuda.device(img.device):
        rc = _lib.load().nrgbd_dgf_refine_f32(_p(depth_lr), n, h, w, _p(img), H, W, *(_p(t) for t in params), float(eps), _p(out),
                                              _stream(img))
    _lib.check(rc, "nrgbd_dgf_refine_f32")
    return out.view(n, 1, H, W)


# ---- TSDF fusion (tsdf.hip; neuralrgbd_amd/fusion.py) ---------------------------------------------------------------------------

def _tsdf_volume(tsdf, weight, who):
    tsdf = _need(tsdf, "tsdf", strided=True)
    if tsdf.dim() != 3 or not tsdf.is_contiguous():
        raise ValueError("%s: tsdf must be a contiguous [Z,Y,X] tensor, got %s" % (who, tuple(tsdf.shape)))
    weight = _need(weight, "weight", tuple(tsdf.shape), strided=True)
    if weight.device != tsdf.device or not weight.is_contiguous():
        raise ValueError("%s: weight must be contiguous and on %s" % (who, tsdf.device))
    return tsdf, weight


def _vec3(v, name):
    v = tuple(float(x) for x in v)
    if len(v) != 3:
        raise ValueError("%s takes three values, got %d" % (name, len(v)))
    return v


def _tsdf_pose(who, pose):
    """A host [3,4] or [4,4] world -> camera matrix as the float32 [3,4] the C entries read."""
    if isinstance(pose, torch.Tensor):
        if pose.is_cuda:
            raise ValueError("%s: pose is a host matrix (it is read at the call)" % who)
        pose = pose.detach().numpy()
    pose = np.asarray(pose)
    if pose.shape not in ((3, 4), (4, 4)):
        raise ValueError("%s: pose is [3,4] or [4,4] world -> camera, got %s" % (who, pose.shape))
    return np.ascontiguousarray(pose[:3, :4], dtype=np.float32)


def _tsdf_frame(who, tsdf, weight, origin, depth, gate, wmap, pose, intrinsics, box):
    """What the two integrations check and prepare alike: -> (tsdf, weight, [depth, gate, wmap], float32 pose [3,4], (fx, fy, cx, cy),
    origin, the box as a C array or None)."""
    tsdf, weight = _tsdf_volume(tsdf, weight, who)
    dev = tsdf.device
    depth = _need(depth, "depth", strided=True)
    if depth.dim() != 2:
        raise ValueError("%s: depth must be [H,W], got %s" % (who, tuple(depth.shape)))
    maps = []
    for t, nm in ((depth, "depth"), (gate, "gate"), (wmap, "wmap")):
        if t is not None:
            t = _need(t, nm, tuple(depth.shape), strided=True)
            if t.device != dev or not t.is_contiguous():
                raise ValueError("%s: %s must be contiguous and on %s" % (who, nm, dev))
        maps.append(t)
    pose = _tsdf_pose(who, pose)
    k = tuple(float(x) for x in intrinsics)
    if len(k) != 4:
        raise ValueError("%s: intrinsics = (fx, fy, cx, cy)" % who)
    o = _vec3(origin, "%s: origin" % who)
    cbox = None
    if box is not None:
        b = tuple(int(x) for x in box)
        if len(b) != 6:
            raise ValueError("%s: box = (x0, y0, z0, x1, y1, z1)" % who)
        cbox = (ctypes.c_int * 6)(*b)
    return tsdf, weight, maps, pose, k, o, cbox


def tsdf_integrate(tsdf, weight, origin, voxel_size, depth, pose, intrinsics, trunc, depth_range=(0.0, float("inf")), w_max=64.0,
                   gate=None, gate_thr=0.0, wmap=None, box=None):
    """One depth frame into a TSDF volume, in place, one launch (nrgbd_tsdf_integrate_f32; the per-voxel operation sequence is
    written out in include/nrgbd.h).
    tsdf / weight: contiguous CUDA fp32 [Z,Y,X]; origin: world position of lattice point (0,0,0); depth (and gate, wmap, or None):
    contiguous CUDA fp32 [H,W] on the same device; pose: host [3,4] or [4,4] world -> camera, cast to float32; intrinsics =
    (fx, fy, cx, cy) at the depth map's size; depth_range = (d_near, d_far]; box: a half-open voxel box (x0, y0, z0, x1, y1, z1) or
    None for the whole grid.  Nothing is allocated, nothing synchronised."""
    _tsdf_integration("tsdf_integrate", tsdf, weight, origin, voxel_size, depth, pose, intrinsics, trunc, depth_range, w_max, gate, gate_thr,
                      wmap, box)


def _tsdf_color(color, tsdf, who):
    """The colour planes [3,Z,Y,X] of a volume: fp32, contiguous, on the volume's device."""
    color = _need(color, "color", (3,) + tuple(tsdf.shape), strided=True)
    if color.device != tsdf.device or not color.is_contiguous():
        raise ValueError("%s: color must be a contiguous [3,Z,Y,X] tensor on %s" % (who, tsdf.device))
    return color


def _tsdf_image(who, image, color_intrinsics, color_affine, dev):
    """What the coloured integrations check and prepare alike: -> (image, (fxc, fyc, cxc, cyc), the affine as float32 [6])."""
    image = _need(image, "image", strided=True)
    if image.dim() != 3 or image.shape[0] != 3 or image.shape[1] < 1 or image.shape[2] < 1:
        raise ValueError("%s: image must be [3,Hc,Wc], got %s" % (who, tuple(image.shape),))
    if image.device != dev or not image.is_contiguous():
        raise ValueError("%s: image must be contiguous and on %s" % (who, dev,))
    kc = tuple(float(x) for x in color_intrinsics)
    if len(kc) != 4:
        raise ValueError("%s: color_intrinsics = (fx, fy, cx, cy)" % who)
    if color_affine is None:
        color_affine = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    affine = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float32).reshape(-1) for v in color_affine]))
    if affine.shape != (6,):
        raise ValueError("%s: color_affine = (a [3], b [3])" % who)
    return image, kc, affine


def _tsdf_integration(who, tsdf, weight, origin, voxel_size, depth, pose, intrinsics, trunc, depth_range, w_max, gate, gate_thr, wmap, box,
                      colour=None, remove=None):
    """The four integration wrappers' checks and call (nrgbd_<who>_f32).  colour = (color, image, color_intrinsics, color_affine): the
    coloured entries; remove = (pose_add or None, w_floor): the reintegrate family, `pose` being pose_remove."""
    tsdf, weight, maps, pose, k, o, cbox = _tsdf_frame(who, tsdf, weight, origin, depth, gate, wmap, pose, intrinsics, box)
    add = None if remove is None or remove[0] is None else _tsdf_pose(who, remove[0])
    if colour is not None:
        color = _tsdf_color(colour[0], tsdf, who)
        image, kc, affine = _tsdf_image(who, colour[1], colour[2], colour[3], tsdf.device)
    host = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    Z, Y, X = tsdf.shape
    H, W = maps[0].shape
    d, g, wm = (_p(t) for t in maps)
    args = [_p(tsdf), _p(weight)] + ([] if colour is None else [_p(color)]) + [X, Y, Z, o[0], o[1], o[2], float(voxel_size)]
    camera = [k[0], k[1], k[2], k[3], float(trunc), float(depth_range[0]), float(depth_range[1]), float(w_max)]
    if remove is None:      # (..., depth, gate, gate_thr, wmap, H, W, pose, fx .. w_max, box, ...)
        args += [d, g, float(gate_thr), wm, H, W, host(pose)] + camera + [cbox]
    else:                   # (..., depth, gate, wmap, pose_remove, pose_add, H, W, fx .. w_max, w_floor, gate_thr, box, ...)
        args += [d, g, wm, host(pose), host(add), H, W] + camera + [float(remove[1]), float(gate_thr), cbox]
    if colour is not None:
        args += [_p(image), image.shape[1], image.shape[2], kc[0], kc[1], kc[2], kc[3], host(affine)]
    with torch.cuda.device(tsdf.device):
        rc = getattr(_lib.load(), "nrgbd_%s_f32" % who)(*args, _stream(tsdf))
    _lib.check(rc, "nrgbd_%s_f32" % who)


def tsdf_integrate_color(tsdf, weight, color, origin, voxel_size, depth, pose, intrinsics, trunc, image, color_intrinsics,
                         color_affine=None, depth_range=(0.0, float("inf")), w_max=64.0, gate=None, gate_thr=0.0, wmap=None, box=None):
    """tsdf_integrate with the frame's colour averaged into the volume's colour planes, one launch (nrgbd_tsdf_integrate_color_f32;
    the operation sequence is written out in include/nrgbd.h): tsdf and weight get the bits tsdf_integrate gives them, and every
    voxel that is updated averages the pixel of `image` it projects to — clamped into the image — into `color` with the same weight.
    color: contiguous CUDA fp32 [3,Z,Y,X]; image: contiguous CUDA fp32 [3,Hc,Wc] on the same device, at a size of its own;
    color_intrinsics = (fx, fy, cx, cy) at that size; color_affine = (a [3], b [3]): the colour of a pixel is image * a + b per
    channel (None: a = 1, b = 0).  Everything else as tsdf_integrate.  Nothing is allocated, nothing synchronised."""
    _tsdf_integration("tsdf_integrate_color", tsdf, weight, origin, voxel_size, depth, pose, intrinsics, trunc, depth_range, w_max, gate,
                      gate_thr, wmap, box, colour=(color, image, color_intrinsics, color_affine))


def tsdf_reintegrate(tsdf, weight, origin, voxel_size, depth, pose_remove, intrinsics, trunc, pose_add=None, w_floor=1e-3,
                     depth_range=(0.0, float("inf")), w_max=64.0, gate=None, gate_thr=0.0, wmap=None, box=None):
    """A depth frame that tsdf_integrate fused at pose_remove taken out of the volume again and, when pose_add is given, put back at
    that pose, in place, one launch (nrgbd_tsdf_reintegrate_f32; the operation sequence is written out in include/nrgbd.h).  The
    arguments are tsdf_integrate's — pass the maps the frame was integrated with —, and w_floor >= 0: a voxel whose weight does not
    stay above it after the removal is fresh again (0, 0).  With pose_add the result is bit for bit that of the removal followed by
    tsdf_integrate at pose_add, with every plane read and written once.  The removal inverts the integration on voxels whose
    weight never reached w_max.  Nothing is allocated, nothing synchronised."""
    _tsdf_integration("tsdf_reintegrate", tsdf, weight, origin, voxel_size, depth, pose_remove, intrinsics, trunc, depth_range, w_max, gate,
                      gate_thr, wmap, box, remove=(pose_add, w_floor))


def tsdf_reintegrate_color(tsdf, weight, color, origin, voxel_size, depth, pose_remove, intrinsics, trunc, image, color_intrinsics,
                           color_affine=None, pose_add=None, w_floor=1e-3, depth_range=(0.0, float("inf")), w_max=64.0, gate=None,
                           gate_thr=0.0, wmap=None, box=None):
    """tsdf_reintegrate on a colour volume (nrgbd_tsdf_reintegrate_color_f32): the frame's colour leaves the colour planes with its
    distance — pass the picture, intrinsics and affine it was integrated with — and enters them again at pose_add; an emptied voxel's
    colour is 0.  The arguments are tsdf_integrate_color's and tsdf_reintegrate's.  Nothing is allocated, nothing synchronised."""
    _tsdf_integration("tsdf_reintegrate_color", tsdf, weight, origin, voxel_size, depth, pose_remove, intrinsics, trunc, depth_range, w_max,
                      gate, gate_thr, wmap, box, colour=(color, image, color_intrinsics, color_affine), remove=(pose_add, w_floor))


def tsdf_shift(src, dst, shift, spill=False):
    """A TSDF volume moved by shift = (sx, sy, sz) whole voxels, one launch (nrgbd_tsdf_shift_f32; the semantics are written out in
    include/nrgbd.h): dst[p][i] = src[p][i + shift] where i + shift lies in the grid, bit for bit, and +0.0 elsewhere — the contents
    of a volume whose origin moved by voxel_size * shift.  src / dst: contiguous CUDA fp32 [2,Z,Y,X] (tsdf, weight) or [5,Z,Y,X]
    (with r, g, b: TSDFVolume's buffer), the same shape and device, distinct storage (their bytes must not overlap).  spill=True:
    the same launch turns src into the spill volume — the retained voxels' tsdf and weight set to 0 except on the one-voxel rim that
    faces the motion, so that src's mesh cells are exactly the old volume's cells with a corner that left.  spill=False: src is only
    read.  Nothing is allocated, nothing synchronised."""
    who = "tsdf_shift"
    src = _need(src, "src", strided=True)
    if src.dim() != 4 or src.shape[0] not in (2, 5) or not src.is_contiguous():
        raise ValueError("%s: src must be a contiguous [2|5,Z,Y,X] tensor, got %s" % (who, tuple(src.shape)))
    dst = _need(dst, "dst", tuple(src.shape), strided=True)
    if dst.device != src.device or not dst.is_contiguous():
        raise ValueError("%s: dst must be contiguous and on %s" % (who, src.device))
    nbytes = src.numel() * 4
    if src.data_ptr() < dst.data_ptr() + nbytes and dst.data_ptr() < src.data_ptr() + nbytes:
        raise ValueError("%s: src and dst need distinct storage (their bytes overlap)" % who)
    s = tuple(int(v) for v in shift)
    if len(s) != 3 or any(int(v) != v for v in shift):
        raise ValueError("%s: shift = (sx, sy, sz) whole voxels, got %r" % (who, shift))
    lim = 2 ** 31 - 1
    s = tuple(max(-lim, min(lim, v)) for v in s)                # beyond the grid either way: nothing is retained
    planes, Z, Y, X = src.shape
    with torch.cuda.device(src.device):
        rc = _lib.load().nrgbd_tsdf_shift_f32(_p(src), _p(dst), planes, X, Y, Z, s[0], s[1], s[2], 1 if spill else 0, _stream(src))
    _lib.check(rc, "nrgbd_tsdf_shift_f32")


TSDF_BLOCK = 8                                                      # NRGBD_TSDF_BLOCK: voxels along a paged block's edge
TSDF_MAX_BLOCKS = 1 << 20                                           # NRGBD_TSDF_MAX_BLOCKS: blocks in one call


class BlockOrigins(typing.NamedTuple):
    """Block origins on both sides: what tsdf_block_origins returns and the two block wrappers take in a host array's place."""
    host: np.ndarray                                                # int32 [n,3]
    dev: torch.Tensor                                               # the same on the device


def tsdf_block_origins(origins, device):
    """origins: a host int array [n,3] of (ox, oy, oz) in grid voxels, |o| <= 2^30 -> BlockOrigins(the int32 array, its copy on
    `device`).  The upload the block wrappers do per call, done once: for a caller that uses the same blocks again, or that captures
    the launches into a graph (an upload from pageable host memory is not a graph node)."""
    if isinstance(origins, BlockOrigins):
        return origins
    if isinstance(origins, torch.Tensor):
        raise TypeError("tsdf_block_origins: origins is a host int array [n,3], not a tensor")
    a = np.asarray(origins)
    if a.size == 0:
        a = np.zeros((0, 3), np.int32)
    if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in "iu":
        raise ValueError("tsdf_block_origins: origins is an int array [n,3], got %s %s" % (a.dtype, a.shape))
    if len(a) > TSDF_MAX_BLOCKS:
        raise ValueError("tsdf_block_origins: %d blocks, at most %d in one call" % (len(a), TSDF_MAX_BLOCKS))
    if len(a) and int(np.abs(a.astype(np.int64)).max()) > 2 ** 30:
        raise ValueError("tsdf_block_origins: an origin beyond 2^30 voxels")
    host = np.ascontiguousarray(a, dtype=np.int32)
    return BlockOrigins(host, torch.from_numpy(host).to(device))


def _tsdf_blocks(who, buf, origins, blocks):
    """What the two block wrappers check alike: -> (buf, BlockOrigins, n, blocks or None)."""
    buf = _need(buf, "buf", strided=True)
    if buf.dim() != 4 or buf.shape[0] not in (2, 5) or not buf.is_contiguous():
        raise ValueError("%s: buf must be a contiguous [2|5,Z,Y,X] tensor, got %s" % (who, tuple(buf.shape)))
    o = tsdf_block_origins(origins, buf.device)
    if o.dev.device != buf.device:
        raise ValueError("%s: the origins are on %s, buf on %s" % (who, o.dev.device, buf.device))
    n = len(o.host)
    if blocks is not None:
        blocks = _need(blocks, "blocks", strided=True)
        if (blocks.dim() != 5 or tuple(blocks.shape[1:]) != (buf.shape[0],) + (TSDF_BLOCK,) * 3 or blocks.shape[0] < n
                or not blocks.is_contiguous() or blocks.device != buf.device or blocks.data_ptr() % 16):
            raise ValueError("%s: blocks must be a contiguous 16-byte aligned [>= %d,%d,8,8,8] tensor on %s, got %s"
                             % (who, n, buf.shape[0], buf.device, tuple(blocks.shape)))
    return buf, o, n, blocks


def tsdf_blocks_gather(buf, origins, out=None, nonempty=None):
    """n blocks of 8^3 voxels read out of a TSDF volume, one launch (nrgbd_tsdf_blocks_gather_f32; the semantics are written out in
    include/nrgbd.h): blocks[b][p][k][j][i] = buf[p][oz + k][oy + j][ox + i] bit for bit where that voxel lies in the grid and +0.0
    where it does not.  buf: contiguous CUDA fp32 [2,Z,Y,X] or [5,Z,Y,X] (TSDFVolume's buffer); origins: a host int array [n,3] of
    (ox, oy, oz) in grid voxels, uploaded here — any integers up to 2^30 either way, aligned to nothing —, or tsdf_block_origins'
    result; out: contiguous CUDA fp32 [>= n,planes,8,8,8] to write the first n blocks of (allocated when None); nonempty: CUDA int32
    [>= n] to write the flags into (allocated when None): 1 where some in-grid word of the block has a non-zero bit pattern (-0.0 and
    NaN count).  Returns (blocks [n,planes,8,8,8], nonempty [n]).  Synchronises nothing."""
    who = "tsdf_blocks_gather"
    buf, o, n, out = _tsdf_blocks(who, buf, origins, out)
    if out is None:
        out = torch.empty((n, buf.shape[0]) + (TSDF_BLOCK,) * 3, dtype=torch.float32, device=buf.device)
    if nonempty is None:
        nonempty = torch.empty(n, dtype=torch.int32, device=buf.device)
    elif (not isinstance(nonempty, torch.Tensor) or nonempty.dtype != torch.int32 or nonempty.dim() != 1 or nonempty.shape[0] < n
          or not nonempty.is_contiguous() or nonempty.device != buf.device):
        raise ValueError("%s: nonempty must be a contiguous int32 tensor [>= %d] on %s" % (who, n, buf.device))
    planes, Z, Y, X = buf.shape
    with torch.cuda.device(buf.device):
        rc = _lib.load().nrgbd_tsdf_blocks_gather_f32(_p(buf), planes, X, Y, Z, _p(o.dev), n, _p(out), _p(nonempty), _stream(buf))
    _lib.check(rc, "nrgbd_tsdf_blocks_gather_f32")
    return out[:n], nonempty[:n]


def tsdf_blocks_scatter(buf, origins, blocks):
    """The inverse of tsdf_blocks_gather, one launch (nrgbd_tsdf_blocks_scatter_f32): every voxel of block b that lies in the grid
    gets blocks[b]'s word, the part of a block outside the grid is ignored, and every voxel outside all the blocks keeps its bits.
    buf, origins: as tsdf_blocks_gather's; blocks: contiguous CUDA fp32 [>= n,planes,8,8,8], the first n are used.  Two blocks of one
    call must not overlap inside the grid — the launch has no order between them —: origins closer than 8 along all three axes whose
    common part reaches into the grid raise ValueError, checked on the host before anything is launched.  Synchronises nothing."""
    who = "tsdf_blocks_scatter"
    buf, o, n, blocks = _tsdf_blocks(who, buf, origins, blocks)
    if blocks is None:
        raise TypeError("%s: blocks must be a torch.Tensor" % who)
    planes, Z, Y, X = buf.shape
    pair = tsdf_blocks_overlap(o.host, (X, Y, Z))
    if pair is not None:
        raise ValueError("%s: blocks %d and %d (origins %s and %s) overlap inside the grid" % ((who,) + pair + tuple(
            tuple(int(v) for v in o.host[k]) for k in pair)))
    with torch.cuda.device(buf.device):
        rc = _lib.load().nrgbd_tsdf_blocks_scatter_f32(_p(buf), planes, X, Y, Z, _p(o.dev), n, _p(blocks), _stream(buf))
    _lib.check(rc, "nrgbd_tsdf_blocks_scatter_f32")


def tsdf_blocks_overlap(origins, dims):
    """The first pair (a, b) of rows of the int array origins [n,3] whose 8^3 blocks share a voxel of the dims = (X, Y, Z) grid, or
    None.  Host only.  Blocks on one 8-voxel lattice — what a paged shift moves — overlap only where two are the same: one sort.
    Otherwise the blocks that touch the grid are sorted into the cells of an 8-voxel lattice; two blocks can share a voxel only from
    the same or a neighbouring cell, so the work grows with n, not n^2."""
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 3)
    dims = np.asarray(dims, dtype=np.int64)
    touching = np.flatnonzero(((o + TSDF_BLOCK > 0) & (o < dims)).all(axis=1))
    if len(touching) < 2:
        return None
    if not ((o[touching] - o[touching[0]]) % TSDF_BLOCK).any():
        rows, first, count = np.unique(o[touching], axis=0, return_index=True, return_counts=True)
        if count.max() == 1:
            return None
        twice = touching[(o[touching] == rows[np.flatnonzero(count > 1)[first[count > 1].argmin()]]).all(axis=1)]
        return (int(twice[0]), int(twice[1]))
    cells = {}
    for b in touching:
        cells.setdefault(tuple(o[b] // TSDF_BLOCK), []).append(int(b))
    for b in touching:
        c = o[b] // TSDF_BLOCK
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    for a in cells.get((int(c[0]) + dx, int(c[1]) + dy, int(c[2]) + dz), ()):
                        if a >= b or (np.abs(o[a] - o[b]) >= TSDF_BLOCK).any():
                            continue
                        lo, hi = np.maximum(np.maximum(o[a], o[b]), 0), np.minimum(np.minimum(o[a], o[b]) + TSDF_BLOCK, dims)
                        if (lo < hi).all():
                            return (a, int(b))
    return None


def tsdf_extract_workspace(X, Y, Z):
    """Bytes of workspace nrgbd_tsdf_extract_points needs for an X x Y x Z grid (needs no GPU)."""
    rc = _lib.load().nrgbd_tsdf_extract_workspace(int(X), int(Y), int(Z))
    if rc < 0:
        _lib.check(rc, "nrgbd_tsdf_extract_workspace")
    return rc


def _tsdf_colors(colors, rows, color, dev, who):
    """The [capacity,3] colour rows that go with a coloured extraction's points (None with None)."""
    if color is None:
        if colors is not None:
            raise ValueError("%s: colors needs the volume's color planes" % who)
        return None
    if rows is None:
        if colors is not None:
            raise ValueError("%s: colors without the rows they belong to" % who)
        return None
    colors = _need(colors, "colors", tuple(rows.shape), strided=True)
    if not colors.is_contiguous() or colors.device != dev:
        raise ValueError("%s: colors must be a contiguous [capacity,3] tensor on %s" % (who, dev))
    return colors


def tsdf_extract_points(tsdf, weight, origin, voxel_size, w_min, workspace, points, counts, color=None, colors=None):
    """The zero crossings of a TSDF volume as points (nrgbd_tsdf_extract_points: three launches, no atomics, ascending (linear voxel
    index, axis) order).  workspace: a contiguous CUDA tensor of at least tsdf_extract_workspace(X, Y, Z) bytes; points: contiguous
    CUDA fp32 [capacity,3] — the first min(found, capacity) rows are written — or None for a count alone; counts: CUDA int64 [2],
    written (crossings found, points written).  color: the volume's colour planes [3,Z,Y,X] and colors: contiguous CUDA fp32
    [capacity,3] — row p gets the colour of point p (nrgbd_tsdf_extract_points_color: the same launches, the same points); without
    them the colourless entry runs.  Nothing is allocated, nothing synchronised."""
    tsdf, weight = _tsdf_volume(tsdf, weight, "tsdf_extract_points")
    dev = tsdf.device
    if color is not None:
        color = _tsdf_color(color, tsdf, "tsdf_extract_points")
    if not isinstance(workspace, torch.Tensor) or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("tsdf_extract_points: workspace must be a contiguous tensor on %s" % (dev,))
    if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or counts.device != dev or not counts.is_contiguous()
            or tuple(counts.shape) != (2,)):
        raise ValueError("tsdf_extract_points: counts must be a contiguous int64 tensor [2] on %s" % (dev,))
    capacity = 0
    if points is not None:
        points = _need(points, "points", strided=True)
        if points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous() or points.device != dev:
            raise ValueError("tsdf_extract_points: points must be a contiguous [capacity,3] tensor on %s" % (dev,))
        capacity = points.shape[0]
    colors = _tsdf_colors(colors, points, color, dev, "tsdf_extract_points")
    o = _vec3(origin, "tsdf_extract_points: origin")
    Z, Y, X = tsdf.shape
    coloured = color is not None                                    # the coloured entry: `color` after weight, `colors` after points
    name = "nrgbd_tsdf_extract_points_color" if coloured else "nrgbd_tsdf_extract_points"
    args = ([_p(tsdf), _p(weight)] + [_p(color)] * coloured
            + [X, Y, Z, o[0], o[1], o[2], float(voxel_size), float(w_min), _p(workspace), workspace.numel() * workspace.element_size(),
               _p(points if capacity else None)] + [_p(colors if capacity else None)] * coloured + [capacity, _p(counts), _stream(tsdf)])
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), name)(*args)
    _lib.check(rc, name)


def tsdf_mesh_workspace(X, Y, Z):
    """Bytes of workspace nrgbd_tsdf_extract_mesh needs for an X x Y x Z grid (needs no GPU)."""
    rc = _lib.load().nrgbd_tsdf_mesh_workspace(int(X), int(Y), int(Z))
    if rc < 0:
        _lib.check(rc, "nrgbd_tsdf_mesh_workspace")
    return rc


def tsdf_extract_mesh(tsdf, weight, origin, voxel_size, w_min, workspace, vertices, faces, counts, color=None, colors=None):
    """The surface of a TSDF volume as an indexed triangle mesh (nrgbd_tsdf_extract_mesh: four launches, no atomics).  The vertices are
    the points of tsdf_extract_points, bit for bit and in its order; a triangle holds the rows of its three vertices in the full vertex
    sequence, its normal towards free space; triangles come in ascending cell order (include/nrgbd.h has the conventions).
    workspace: a contiguous CUDA tensor of at least tsdf_mesh_workspace(X, Y, Z) bytes; vertices: contiguous CUDA fp32 [capacity,3] or
    None; faces: contiguous CUDA int32 [capacity,3] or None — the first min(found, capacity) rows of either are written; counts: CUDA
    int64 [4], written (vertices found, vertices written, triangles found, triangles written).  color: the volume's colour planes
    [3,Z,Y,X] and colors: contiguous CUDA fp32 [capacity,3] — row p gets the colour of vertex p (nrgbd_tsdf_extract_mesh_color: the
    same launches, vertices and faces); without them the colourless entry runs.  Nothing is allocated, nothing synchronised."""
    tsdf, weight = _tsdf_volume(tsdf, weight, "tsdf_extract_mesh")
    dev = tsdf.device
    if color is not None:
        color = _tsdf_color(color, tsdf, "tsdf_extract_mesh")
    if not isinstance(workspace, torch.Tensor) or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("tsdf_extract_mesh: workspace must be a contiguous tensor on %s" % (dev,))
    if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or counts.device != dev or not counts.is_contiguous()
            or tuple(counts.shape) != (4,)):
        raise ValueError("tsdf_extract_mesh: counts must be a contiguous int64 tensor [4] on %s" % (dev,))
    caps = []
    for t, nm, dt in ((vertices, "vertices", torch.float32), (faces, "faces", torch.int32)):
        if t is None:
            caps.append(0)
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise TypeError("tsdf_extract_mesh: %s must be a %s tensor" % (nm, dt))
        if t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous() or t.device != dev:
            raise ValueError("tsdf_extract_mesh: %s must be a contiguous [capacity,3] tensor on %s" % (nm, dev))
        caps.append(t.shape[0])
    colors = _tsdf_colors(colors, vertices, color, dev, "tsdf_extract_mesh")
    o = _vec3(origin, "tsdf_extract_mesh: origin")
    Z, Y, X = tsdf.shape
    coloured = color is not None                                    # the coloured entry: `color` after weight, `colors` after vertices
    name = "nrgbd_tsdf_extract_mesh_color" if coloured else "nrgbd_tsdf_extract_mesh"
    args = ([_p(tsdf), _p(weight)] + [_p(color)] * coloured
            + [X, Y, Z, o[0], o[1], o[2], float(voxel_size), float(w_min), _p(workspace), workspace.numel() * workspace.element_size(),
               _p(vertices if caps[0] else None)] + [_p(colors if caps[0] else None)] * coloured
            + [caps[0], _p(faces if caps[1] else None), caps[1], _p(counts), _stream(tsdf)])
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), name)(*args)
    _lib.check(rc, name)


TSDF_RAYCAST_TILE = _lib.TSDF_RAYCAST_TILE      # side of the pixel tile a workgroup of nrgbd_tsdf_raycast_f32 owns (a wave: 8 x 8)


def camera_centre(pose):
    """The camera centre -R^T t of a world -> camera pose: float32(pose[:3,:4]) promoted to float64, the three sums formed in a
    fixed order, rounded to float32 once (what nrgbd_tsdf_raycast_f32 takes as `centre`)."""
    p = np.asarray(pose)[:3, :4].astype(np.float32).astype(np.float64)
    return np.array([-((p[0, k] * p[0, 3] + p[1, k] * p[1, 3]) + p[2, k] * p[2, 3]) for k in range(3)], dtype=np.float64).astype(np.float32)


def tsdf_raycast(tsdf, weight, origin, voxel_size, pose, intrinsics, size, depth_range, w_min=1.0, step=None, normals=False, out=None,
                 color=None, rgb=False):
    """A TSDF volume seen from a camera, one launch (nrgbd_tsdf_raycast_f32; the per-pixel operation sequence is written out in
    include/nrgbd.h): z-depth [H,W] of the first zero crossing along every pixel's ray, 0 where there is none, and with normals=True
    (depth, normal [3,H,W]), the unit surface normals in the camera frame ((0,0,0) where there is none).
    tsdf / weight: contiguous CUDA fp32 [Z,Y,X]; pose: host [3,4] or [4,4] world -> camera, cast to float32; intrinsics = (fx, fy, cx,
    cy) at size = (H, W); depth_range = [d_near, d_far]; a sample counts where the eight weights around it are >= w_min; step: the
    sample distance along the ray in metres (None: voxel_size).  out: a contiguous CUDA fp32 [H,W] tensor, or with normals=True the
    pair ([H,W], [3,H,W]), to write into; then nothing is allocated.  rgb=True with color, the volume's colour planes [3,Z,Y,X]
    (nrgbd_tsdf_raycast_color_f32: the same depth and normals): the trilinear colour at every hit [3,H,W], (0,0,0) where there is
    none, as one more element of the result — (depth, rgb) or (depth, normal, rgb), and `out` takes the same tuple.  Nothing is
    synchronised."""
    if rgb and color is None:
        raise ValueError("tsdf_raycast: rgb=True needs the volume's color planes")
    tsdf, weight = _tsdf_volume(tsdf, weight, "tsdf_raycast")
    dev = tsdf.device
    if rgb:
        color = _tsdf_color(color, tsdf, "tsdf_raycast")
    H, W = (int(n) for n in size)
    pose = _tsdf_pose("tsdf_raycast", pose)
    centre = np.ascontiguousarray(camera_centre(pose))
    k = tuple(float(x) for x in intrinsics)
    if len(k) != 4:
        raise ValueError("tsdf_raycast: intrinsics = (fx, fy, cx, cy)")
    o = _vec3(origin, "tsdf_raycast: origin")
    wanted = [("out depth", (H, W)), ("out normal", (3, H, W))][:2 if normals else 1] + ([("out rgb", (3, H, W))] if rgb else [])
    if out is None:
        if H <= 0 or W <= 0:
            raise ValueError("tsdf_raycast: size = (H, W), positive; got %s" % (size,))
        outs = [torch.empty(shape, dtype=torch.float32, device=dev) for _, shape in wanted]
    else:
        if len(wanted) > 1 and (not isinstance(out, (tuple, list)) or len(out) != len(wanted)):
            raise ValueError("tsdf_raycast: out=(%s)" % ", ".join(nm[4:] for nm, _ in wanted) if rgb else
                             "tsdf_raycast: normals=True takes out=(depth, normal)")
        outs = list(out) if len(wanted) > 1 else [out]
        for t, (nm, shape) in zip(outs, wanted):
            t = _need(t, nm, shape, strided=True)
            if t.device != dev or not t.is_contiguous():
                raise ValueError("tsdf_raycast: %s must be contiguous and on %s" % (nm, dev))
    normal = outs[1] if normals else None
    Z, Y, X = tsdf.shape
    name = "nrgbd_tsdf_raycast_color_f32" if rgb else "nrgbd_tsdf_raycast_f32"        # `color` after weight, the rgb output after normal
    rgb = bool(rgb)
    args = ([_p(tsdf), _p(weight)] + [_p(color)] * rgb
            + [X, Y, Z, o[0], o[1], o[2], float(voxel_size), ctypes.c_void_p(pose.ctypes.data), ctypes.c_void_p(centre.ctypes.data), k[0],
               k[1], k[2], k[3], H, W, float(depth_range[0]), float(depth_range[1]), float(w_min),
               float(voxel_size if step is None else step), _p(outs[0]), _p(normal)] + [_p(outs[-1])] * rgb + [_stream(tsdf)])
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), name)(*args)
    _lib.check(rc, name)
    return tuple(outs) if len(outs) > 1 else outs[0]


# ---- frame-to-model tracking (icp.hip; neuralrgbd_amd/tracking.py) --------------------------------------------------------------

ICP_STATE_WORDS = _lib.ICP_STATE_BYTES // 8         # the state as float64 words: T [12], then Tf [12] fp32, flag and iterations int32
ICP_RECORD_WORDS = _lib.ICP_RECORD_BYTES // 8       # a partial record as float64 words: 28 sums, the int64 count, padding


def icp_workgroups(Hs, Ws):
    """Partial records nrgbd_icp_terms_f32 writes for an Hs x Ws visit (needs no GPU)."""
    rc = _lib.load().nrgbd_icp_workgroups(int(Hs), int(Ws))
    if rc < 0:
        _lib.check(rc, "nrgbd_icp_workgroups")
    return rc


def icp_workspace(Hs, Ws):
    """Bytes of `partial` nrgbd_icp_terms_f32 needs for an Hs x Ws visit (needs no GPU)."""
    rc = _lib.load().nrgbd_icp_workspace(int(Hs), int(Ws))
    if rc < 0:
        _lib.check(rc, "nrgbd_icp_workspace")
    return rc


def _icp_words(t, name, words, dev, who):
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() < words
            or (dev is not None and t.device != dev) or not t.is_cuda):
        raise ValueError("%s: %s must be a contiguous CUDA float64 tensor of at least %d elements%s"
                         % (who, name, words, "" if dev is None else " on %s" % (dev,)))
    return t


def _icp_terms_args(who, depth, intrinsics, sub, mdepth, mnormal, model_intrinsics, state, partial, gate, resid, image=None, mrgb=None,
                    resid_photo=None, photo=False):
    """The checks icp_terms and icp_terms_photo share -> (dev, H, W, Hm, Wm, k, km, sub)."""
    depth = _need(depth, "depth", strided=True)
    if depth.dim() != 2:
        raise ValueError("%s: depth must be [H,W], got %s" % (who, tuple(depth.shape),))
    dev = depth.device
    H, W = depth.shape
    mdepth = _need(mdepth, "mdepth", strided=True)
    if mdepth.dim() != 2:
        raise ValueError("%s: mdepth must be [Hm,Wm], got %s" % (who, tuple(mdepth.shape),))
    Hm, Wm = mdepth.shape
    maps = [(depth, "depth", (H, W)), (gate, "gate", (H, W)), (resid, "resid", (H, W)), (mdepth, "mdepth", (Hm, Wm)),
            (mnormal, "mnormal", (3, Hm, Wm))]
    if photo:
        maps += [(image, "image", (3, H, W)), (mrgb, "mrgb", (3, Hm, Wm)), (resid_photo, "resid_photo", (H, W))]
    for t, nm, shape in maps:
        if t is None and nm in ("gate", "resid", "resid_photo"):
            continue
        t = _need(t, nm, shape, strided=True)
        if t.device != dev or not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous and on %s" % (who, nm, dev))
    k, km = tuple(float(x) for x in intrinsics), tuple(float(x) for x in model_intrinsics)
    if len(k) != 4 or len(km) != 4:
        raise ValueError("%s: intrinsics = (fx, fy, cx, cy)" % who)
    _icp_words(state, "state", ICP_STATE_WORDS, dev, who)
    _icp_words(partial, "partial", 0, dev, who)
    return dev, H, W, Hm, Wm, k, km, int(sub)


def icp_terms(depth, intrinsics, sub, mdepth, mnormal, model_intrinsics, state, partial, dist_thr, huber, depth_range=(0.0, float("inf")),
              gate=None, gate_thr=0.0, resid=None):
    """Association, point-to-plane residuals and the partial normal equations of one Gauss-Newton iteration, one launch
    (nrgbd_icp_terms_f32; the per-pixel operation sequence is written out in include/nrgbd.h).
    depth (and gate, resid, or None): contiguous CUDA fp32 [H,W]; intrinsics = (fx, fy, cx, cy) at H x W; sub: every sub-th pixel
    is visited; mdepth [Hm,Wm] / mnormal [3,Hm,Wm]: the model maps of tsdf_raycast with model_intrinsics at their size; state: float64
    [ICP_STATE_WORDS] (icp_update's); partial: float64, at least icp_workspace(H // sub, W // sub) bytes; depth_range = (d_near,
    d_far].  Returns the number of records written.  Nothing is allocated, nothing synchronised."""
    dev, H, W, Hm, Wm, k, km, sub = _icp_terms_args("icp_terms", depth, intrinsics, sub, mdepth, mnormal, model_intrinsics, state, partial,
                                                    gate, resid)
    with torch.cuda.device(dev):
        rc = _lib.load().nrgbd_icp_terms_f32(_p(depth), _p(gate), float(gate_thr), H, W, float(depth_range[0]), float(depth_range[1]),
                                             k[0], k[1], k[2], k[3], sub, _p(mdepth), _p(mnormal), Hm, Wm, km[0], km[1], km[2], km[3],
                                             _p(state), float(dist_thr), float(huber), _p(partial), partial.numel() * 8, _p(resid),
                                             _stream(depth))
    _lib.check(rc, "nrgbd_icp_terms_f32")
    return icp_workgroups(H // sub, W // sub)


def icp_terms_photo(depth, intrinsics, sub, mdepth, mnormal, model_intrinsics, state, partial, dist_thr, huber, image, mrgb,
                    photo_weight, photo_huber, image_affine=None, depth_range=(0.0, float("inf")), gate=None, gate_thr=0.0, resid=None,
                    resid_photo=None):
    """icp_terms with one photometric residual more per pair, added to the same normal equations, one launch
    (nrgbd_icp_terms_photo_f32; the operation sequence is written out in include/nrgbd.h): the frame's luminance at the visited pixel
    against the model's, interpolated bilinearly in mrgb where the point projects.  image: contiguous CUDA fp32 [3,H,W], the frame's
    picture at the depth map's size; image_affine = (a [3], b [3]): a pixel's colour is image * a + b per channel (None: a = 1,
    b = 0), as tsdf_integrate_color takes it; mrgb [3,Hm,Wm]: the rgb of tsdf_raycast beside mdepth and mnormal; photo_weight: a
    photometric term's weight beside a geometric one's; photo_huber: intensity residuals beyond it are down-weighted; resid_photo
    (or None): [H,W].  Everything else, and the result, as icp_terms: resid, the geometric pair count and nrgbd_icp_update's reading
    of the record are unchanged; the record's last word holds the count of photometric pairs.  Nothing is allocated on the device,
    nothing synchronised."""
    dev, H, W, Hm, Wm, k, km, sub = _icp_terms_args("icp_terms_photo", depth, intrinsics, sub, mdepth, mnormal, model_intrinsics, state,
                                                    partial, gate, resid, image, mrgb, resid_photo, photo=True)
    if image_affine is None:
        image_affine = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    affine = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float32).reshape(-1) for v in image_affine]))
    if affine.shape != (6,):
        raise ValueError("icp_terms_photo: image_affine = (a [3], b [3])")
    with torch.cuda.device(dev):
        rc = _lib.load().nrgbd_icp_terms_photo_f32(_p(depth), _p(gate), float(gate_thr), H, W, float(depth_range[0]), float(depth_range[1]),
                                                   k[0], k[1], k[2], k[3], sub, _p(mdepth), _p(mnormal), Hm, Wm, km[0], km[1], km[2],
                                                   km[3], _p(state), float(dist_thr), float(huber), _p(partial), partial.numel() * 8,
                                                   _p(resid), _p(image), ctypes.c_void_p(affine.ctypes.data),
                                                   ctypes.c_void_p(affine.ctypes.data + 12), _p(mrgb), float(photo_weight),
                                                   float(photo_huber), _p(resid_photo), _stream(depth))
    _lib.check(rc, "nrgbd_icp_terms_photo_f32")
    return icp_workgroups(H // sub, W // sub)


def icp_update(state, step, partial=None, nwg=0, min_pairs=6, min_pivot=1e-6, log=None, init=None):
    """The solve and the pose update of one Gauss-Newton iteration, one launch of one workgroup (nrgbd_icp_update; every operation is
    written out in include/nrgbd.h).  step == 0: the state from `init` (a host [3,4] or [4,4] float64 motion; None: the identity).
    step >= 1: the `nwg` records of `partial` added in index order, the tests, the L D L^T solve, T <- exp(xi) T; row step - 1 of
    log (float64 [rows,4]) = (count, E, |xi|^2, flag).  Nothing is allocated, nothing synchronised."""
    state = _icp_words(state, "state", ICP_STATE_WORDS, None, "icp_update")
    dev = state.device
    step = int(step)
    cinit = None
    if init is not None:
        m = np.asarray(init, dtype=np.float64)
        if m.shape not in ((3, 4), (4, 4)):
            raise ValueError("icp_update: init is a [3,4] or [4,4] motion, got %s" % (m.shape,))
        cinit = (ctypes.c_double * 12)(*m[:3, :4].reshape(-1).tolist())
    if step > 0:
        partial = _icp_words(partial, "partial", int(nwg) * ICP_RECORD_WORDS, dev, "icp_update")
        log = _icp_words(log, "log", 4 * step, dev, "icp_update")
    with torch.cuda.device(dev):
        rc = _lib.load().nrgbd_icp_update(_p(state), cinit, step, _p(partial if step > 0 else None), int(nwg), int(min_pairs),
                                          float(min_pivot), _p(log if step > 0 else None), _stream(state))
    _lib.check(rc, "nrgbd_icp_update")


# ---- multi-view depth consistency (consistency.hip; neuralrgbd_amd/fusion.py) -------------------------------------------------------

CONSISTENCY_MAX_SRC = _lib.CONSISTENCY_MAX_SRC


def depth_consistency(depth, intrinsics, src_depth, src_T, rel_thr, min_views, depth_range=(0.0, float("inf")), gate=None, gate_thr=0.0,
                      src_gate=None, src_slots=None, votes=None, depth_out=None):
    """A depth map cross-checked against other views' maps, one launch (nrgbd_depth_consistency_f32; the per-pixel operation sequence
    is written out in include/nrgbd.h): every valid pixel is lifted, moved into each source camera, projected, and compared with the
    source's depth at the nearest pixel; a source agrees where |ds - q_z| <= rel_thr q_z.
    depth (and gate, or None): contiguous CUDA fp32 [H,W]; intrinsics = (fx, fy, cx, cy) at H x W, the sources' too; src_depth (and
    src_gate, given exactly when gate is): CUDA fp32 [S,H,W], the maps contiguous and any stride >= H W between them (None: no
    sources); src_slots: which map of the stack each source is (default 0 .. S-1; repeats allowed); src_T: host [n,3,4] or [n,4,4],
    reference camera -> source camera, one per entry of src_slots, rounded to fp32 once; depth_range = (d_near, d_far]: what a pixel
    of either map needs to count; min_views: the agreeing sources a pixel needs to stay.
    votes / depth_out: a tensor [H,W] to write into, None: allocated here, False: not produced.  Returns (votes, depth_out) with
    None for what was not produced: votes = the agreeing sources per pixel as fp32, -1 at an invalid pixel; depth_out = depth where
    votes >= min_views, else 0; depth_out may be `depth` itself.  Nothing else is allocated, nothing synchronised."""
    who = "depth_consistency"
    depth = _need(depth, "depth", strided=True)
    if depth.dim() != 2:
        raise ValueError("%s: depth must be [H,W], got %s" % (who, tuple(depth.shape),))
    dev = depth.device
    H, W = depth.shape
    if votes is False and depth_out is False:
        raise ValueError("%s: neither votes nor depth_out is asked for" % who)
    for t, nm in ((depth, "depth"), (gate, "gate"), (votes, "votes"), (depth_out, "depth_out")):
        if t is None or t is False:
            continue
        t = _need(t, nm, (H, W), strided=True)
        if t.device != dev or not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous and on %s" % (who, nm, dev))
    k = tuple(float(x) for x in intrinsics)
    if len(k) != 4:
        raise ValueError("%s: intrinsics = (fx, fy, cx, cy)" % who)
    n_src, stride, slots, cT = 0, 0, None, None
    if src_depth is None:
        if src_gate is not None or src_slots:
            raise ValueError("%s: src_gate and src_slots come with src_depth" % who)
    else:
        if (gate is None) != (src_gate is None):
            raise ValueError("%s: gate and src_gate come together" % who)
        src_depth = _need(src_depth, "src_depth", strided=True)
        if src_depth.dim() != 3 or tuple(src_depth.shape[1:]) != (H, W):
            raise ValueError("%s: src_depth must be [S,%d,%d], got %s" % (who, H, W, tuple(src_depth.shape),))
        S = src_depth.shape[0]
        stride = src_depth.stride(0) if S > 1 else H * W
        for t, nm in ((src_depth, "src_depth"), (src_gate, "src_gate")):
            if t is None:
                continue
            t = _need(t, nm, (S, H, W), strided=True)
            if t.device != dev or not t[0].is_contiguous() or (S > 1 and (t.stride(0) != stride or stride < H * W)):
                raise ValueError("%s: %s must hold contiguous maps, the same stride >= H W apart, on %s" % (who, nm, dev))
        slots = list(range(S)) if src_slots is None else [int(s) for s in src_slots]
        if any(s < 0 or s >= S for s in slots):
            raise ValueError("%s: src_slots %s name maps of a stack of %d" % (who, slots, S))
        n_src = len(slots)
        if n_src > CONSISTENCY_MAX_SRC:
            raise ValueError("%s: %d sources, at most %d" % (who, n_src, CONSISTENCY_MAX_SRC))
    if n_src:
        m = np.asarray(src_T, dtype=np.float64)
        if m.ndim != 3 or m.shape[0] != n_src or m.shape[1:] not in ((3, 4), (4, 4)):
            raise ValueError("%s: src_T is [%d,3,4] or [%d,4,4], got %s" % (who, n_src, n_src, m.shape))
        with np.errstate(over="ignore"):
            cT = np.ascontiguousarray(m[:, :3, :4].astype(np.float32)).reshape(-1)      # rounded once
        slots = (ctypes.c_int * n_src)(*slots)
    if votes is None:
        votes = torch.empty((H, W), dtype=torch.float32, device=dev)
    if depth_out is None:
        depth_out = torch.empty((H, W), dtype=torch.float32, device=dev)
    votes = None if votes is False else votes
    depth_out = None if depth_out is False else depth_out
    with torch.cuda.device(dev):
        rc = _lib.load().nrgbd_depth_consistency_f32(_p(depth), _p(gate), float(gate_thr), H, W, float(depth_range[0]), float(depth_range[1]),
                                                     k[0], k[1], k[2], k[3], _p(src_depth if n_src else None),
                                                     _p(src_gate if n_src else None), int(stride), slots if n_src else None,
                                                     ctypes.c_void_p(cT.ctypes.data) if n_src else None, n_src, float(rel_thr),
                                                     int(min_views), _p(votes), _p(depth_out), _stream(depth))
    _lib.check(rc, "nrgbd_depth_consistency_f32")
    return votes, depth_out
