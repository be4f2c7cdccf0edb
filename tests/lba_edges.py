"""Edge-case inputs of the local bundle adjustment's fused pass (lba.hip::lba_grad_kernel) and the exact-position comparator the
tests hold it against.

`edge_level(H, W, N, content)` builds one pyramid level (ref [3,H,W], src [N,3,H,W], dmap, conf, K, rays, R [N,3,3], t [N,3]),
float32 on the CPU, from a rendered window.  Contents:
  "small"   poses perturbed by 0.01 rad / 0.02 (the existing test's inputs);
  "zeros"   a zero border in every channel of every source, and one channel zeroed over a region of every other source (the
            per-channel mask warped != 0, opt_pose_numerical.py:258-266);
  "conf0"   exact zeros over a region of the confidence map;
  "large"   0.1 rad / 0.3 perturbations: a large share of the pixels partly or wholly out of frame (the tap validity flags);
  "behind"  a translation that puts the nearer points behind the camera (P_z < 0; the warp has no epsilon), none at P_z = 0;
  "true"    the true poses: the gradient nearly cancels;
  "mixed"   the view kinds small, large, behind, true in turn, with the zero regions and the confidence zeros.

`exact_sums(level)` is the comparator.  Its sample positions are bit-identical to the kernel's (oracle_warp_depth_fwd: the same
fp32 fma chains): the warped values come from cpu_oracle.warp_depth_fwd, the mask, residual r = w c - ref c, |r| and sign(r) c
are formed in float64, and the gradient comes from cpu_oracle.warp_depth_bwd (accumulated in double) with g_out = sign(r) c mask.
What the kernel may still differ by is rounding: `bound` holds, per view and component, SUM_C 2^-24 times the float64 absolute
sum of the per-pixel terms (cpu_oracle.warp_depth_bwd_abs), plus what the "tie" channels can move — those whose |r| (or whose
warped value, for the mask) is within rounding of 0 (TIE_C 2^-24 of the magnitudes it is formed from), where sign (or the mask)
may legitimately differ (the max_tie_flips idea of conftest.py: a bound from the tie population, not a constant).
"""
import numpy as np
import torch

from neuralrgbd_amd import camera, synth
from oracle import cpu_oracle as co

U = 2.0 ** -24
# Rounding steps between a pixel's inputs and the kernel's partial sum: the warped value (4 fma), the residual (3), the tap
# differences and their fma chain over 3 channels (~9), dY (~8), the per-lane accumulation (<= 2 pixels per lane at every size
# tested), the wave tree (6) and the four-wave sum (2): ~32; SUM_C doubles that.
SUM_C = 64.0
# |r_kernel - r| <= (2 + 2 + 1) u (|w|_abs + |ref|) c: the kernel's and the oracle's warped values each within 2 u of the exact
# bilinear sum (4-term fp32 sums of the same products in another order), the two products and the difference; TIE_C doubles
# that and more.
TIE_C = 16.0
SIZES = [(7, 9), (65, 97), (256, 256), (256, 257), (256, 384)]
KINDS = ("small", "large", "behind", "true")

_windows = {}


def _window(H, W, V=16, seed=61):
    key = (H, W, V, seed)
    if key not in _windows:
        cam = camera.scannet_intrinsics(W, H)
        ref, src, poses, depth = synth.rendered_window(seed, H, W, cam, V=V)
        _windows[key] = (ref[0].float().numpy(), src[0].float().numpy(), poses[0].numpy().astype(np.float64), depth, cam)
    return _windows[key]


def _behind(rng, true, depth):
    """A pose moved back along the optical axis by the median depth: the nearer half of the reference points lands behind the
    source camera."""
    P = true.copy()
    P[:3, 3] += np.array([0.05 * rng.standard_normal(), 0.05 * rng.standard_normal(), -float(np.median(depth)) - 0.0123])
    return P


def edge_level(H, W, N, content, seed=61):
    ref, src, poses, depth, cam = _window(H, W, max(N, 16), seed)
    rng = np.random.RandomState(seed + 7 * N + H)
    src = src[:N].copy()
    conf = (0.2 + 0.8 * rng.rand(H, W)).astype(np.float32)
    kinds = [content] * N if content in KINDS else (list(KINDS) * 4)[:N] if content == "mixed" else ["small"] * N
    if content in ("zeros", "mixed"):
        b = max(1, min(10, min(H, W) // 5))
        src[:, :, :b] = 0; src[:, :, -b:] = 0; src[:, :, :, :b] = 0; src[:, :, :, -b:] = 0
        for v in range(1, N, 2):                 # one channel of every other source zeroed over a region
            src[v, v % 3, H // 4:H // 4 + max(1, H // 3), W // 3:W // 3 + max(1, W // 3)] = 0
    if content in ("conf0", "mixed"):
        conf[rng.rand(H, W) < 0.15] = 0
        conf[H // 2:H // 2 + max(1, H // 6), :] = 0
    P = np.empty((N, 4, 4), np.float64)
    for v in range(N):
        true = poses[v]
        if kinds[v] == "small":
            P[v] = synth.random_pose(rng, 0.01, 0.02).astype(np.float64) @ true
        elif kinds[v] == "large":
            d = synth.rotvec_to_R(rng.standard_normal(3) * (0.1 / np.sqrt(3)))
            pert = np.eye(4); pert[:3, :3] = d; pert[:3, 3] = rng.standard_normal(3) * (0.3 / np.sqrt(3))
            P[v] = pert @ true
        elif kinds[v] == "behind":
            P[v] = _behind(rng, true, depth)
        else:
            P[v] = true
    P = P.astype(np.float32)
    K = cam["intrinsic_M_cuda"].numpy().astype(np.float32)
    rays = cam["unit_ray_array_2D"].numpy().astype(np.float32)
    R, t = P[:, :3, :3].copy(), P[:, :3, 3].copy()
    X = depth.reshape(1, -1).astype(np.float64) * rays
    for v in range(N):                             # P_z of every point well away from 0 (the division has no epsilon)
        while np.abs(R[v, 2].astype(np.float64) @ X + t[v, 2]).min() < 1e-4:
            t[v, 2] += np.float32(3.7e-4)
    if "behind" in kinds:
        assert (np.einsum("nj,jp->np", R[:, 2].astype(np.float64), X) + t[:, 2:3] < 0).any()
    return ref, src, depth.astype(np.float32), conf, K, rays, R, t


def exact_sums(level):
    """Unnormalised sums the kernel's partials hold, from the exact-position comparator: dict with
    loss [N] = sum |r|, g [N,12] = (dL/dR row-major, dL/dt) with L = sum |r|, and the bounds loss_bound [N], g_bound [N,12]."""
    ref, src, dmap, conf, K, rays, R, t = level
    N, C, H, W = src.shape
    w = co.warp_depth_fwd(src, dmap, K, R, t, rays).astype(np.float64)                 # the kernel's positions, bit for bit
    w_abs = co.warp_depth_fwd(np.abs(src), dmap, K, R, t, rays).astype(np.float64)     # sum |tap| weight
    c = conf.astype(np.float64)[None, None]
    ref64 = ref.astype(np.float64)[None]
    mask = w != 0
    r = (w * c - ref64 * c) * mask
    scale = (w_abs + np.abs(ref64)) * c
    tie = ((np.abs(r) <= TIE_C * U * scale) & (c > 0) & mask) | ((np.abs(w) <= TIE_C * U * w_abs) & (w_abs > 0))
    g_out = (np.sign(r) * c * mask).astype(np.float32)
    gR, gt = co.warp_depth_bwd(src, dmap, K, R, t, rays, g_out)
    aR, at = co.warp_depth_bwd_abs(src, dmap, K, R, t, rays, (c * mask).astype(np.float32) * np.ones_like(w, np.float32))
    tR, tt = co.warp_depth_bwd_abs(src, dmap, K, R, t, rays, (2.0 * c * tie).astype(np.float32) * np.ones_like(w, np.float32))
    loss = np.abs(r).sum(axis=(1, 2, 3))
    loss_bound = SUM_C * U * (scale * mask).sum(axis=(1, 2, 3)) + ((np.abs(ref64) * c + TIE_C * U * scale) * tie).sum(axis=(1, 2, 3))
    g = np.concatenate([gR.reshape(N, 9), gt], 1).astype(np.float64)
    g_bound = SUM_C * U * np.concatenate([aR.reshape(N, 9), at], 1) + np.concatenate([tR.reshape(N, 9), tt], 1)
    return {"loss": loss, "g": g, "loss_bound": loss_bound, "g_bound": g_bound, "ties": int(tie.sum()),
            "masked": int((~mask).sum()), "partial_taps": partial_taps(level)}


def partial_taps(level):
    """Pixels (over the views) whose sample has some but not all of its four taps inside the image."""
    _, src, dmap, _, K, rays, R, t = level
    ones = np.ones_like(src[:, :1])
    cover = co.warp_depth_fwd(ones, dmap, K, R, t, rays)        # sum of the in-image weights
    return int(((cover > 0) & (cover < 1 - 1e-6)).sum())


def fp64_level(level):
    """The level as the float64 restatement's input (lba_fp64.loss_and_grad)."""
    ref, src, dmap, conf, K, rays, R, t = level
    return (torch.from_numpy(ref).double()[None], torch.from_numpy(src).double(), torch.from_numpy(dmap).double(),
            torch.from_numpy(conf).double(), torch.from_numpy(K).double(), torch.from_numpy(rays).double())
