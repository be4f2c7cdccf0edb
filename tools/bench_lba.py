"""Local bundle adjustment benchmark: ms per local_BA_direct_parallel call (4 sources, dw_scales [4, 2, 1], 20 iterations, lr 0.01)
at config S (256 x 384) and B-size images (768 x 1024), beside an eager composition of the reference algorithm on the same GPU
(DepthWarp autograd, ATen mask / L1, the torch quaternion code, torch.optim.Adam).

    python tools/bench_lba.py [--sizes S,B] [--reps 10] [--warmup 3] [--json out.json]
    python tools/bench_lba.py --trace-only          # a few calls for `rocprofv3 --kernel-trace --stats -- python ...`

Timing: HIP events around each call after a warm-up (median).  The call includes the pyramid, the uploads and the read-back of
the poses, as a user sees it.  Launches per call are counted from the design (1 pyramid + 1 initialisation + 2 per iteration).
Bytes per iteration of the fused pass (nrgbd_lba_grad at full resolution) are the unique bytes it must read: sources, reference
image, rays, depth and confidence; its kernel time comes from a separate rocprofv3 trace (tools/bench_lba.py --trace-only).
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralrgbd_amd import camera, misc, ops, opt_pose, synth  # noqa: E402
from neuralrgbd_amd.autograd import DepthWarp  # noqa: E402

SIZES = {"S": (256, 384), "B": (768, 1024)}
V, SCALES, ITERS, LR = 4, [4, 2, 1], 20, 0.01


def workload(H, W, seed=0):
    rng = np.random.RandomState(seed)
    ref = torch.from_numpy(synth.smooth_texture(rng, 3, H, W))[None]
    srcs = [torch.from_numpy(synth.smooth_texture(rng, 3, H, W))[None] for _ in range(V)]
    dmap = torch.from_numpy((0.6 + 3.0 * rng.rand(H, W)).astype(np.float32))[None, None]
    conf = torch.from_numpy(rng.rand(H, W).astype(np.float32))[None, None]
    poses = [p for p in synth.random_poses(rng, V)]
    cams = [camera.scannet_intrinsics(W // k, H // k) for k in SCALES]
    dev = "cuda:0"
    return ref.to(dev), [s.to(dev) for s in srcs], dmap.to(dev), conf.to(dev), cams, poses


def fused_call(w):
    ref, srcs, dmap, conf, cams, poses = w
    with contextlib.redirect_stdout(io.StringIO()):
        return opt_pose.local_BA_direct_parallel(ref, srcs, dmap, conf, cams, SCALES, poses, ITERS, LR, [1, 1])


def eager_call(w):
    """The reference algorithm composed from torch ops and the reference-named warp operator (what a user gets by swapping only
    the warp into ICP/opt_pose_numerical.py)."""
    ref, srcs, dmap, conf, cams, poses = w
    F = torch.nn.functional
    srcs = torch.cat(srcs, 0)
    lv = [(F.avg_pool2d(ref, k) if k > 1 else ref, F.avg_pool2d(srcs, k) if k > 1 else srcs,
           (F.avg_pool2d(dmap, k) if k > 1 else dmap).squeeze(), (F.avg_pool2d(conf, k) if k > 1 else conf).squeeze(),
           c["intrinsic_M_cuda"].cuda(), c["unit_ray_array_2D"].cuda()) for k, c in zip(SCALES, cams)]
    uq = torch.stack([misc.Rotation2UnitQ(torch.from_numpy(p[:3, :3].copy())) for p in poses]).cuda().requires_grad_(True)
    t = torch.stack([torch.from_numpy(p[:3, 3].copy()) for p in poses]).cuda().requires_grad_(True)
    opt = torch.optim.Adam([t, uq], lr=LR, betas=(.9, .999))
    loss_fn = torch.nn.L1Loss()
    for iscale, (r, s, d, c, K, rays) in enumerate(lv):
        if iscale > 0:
            for g in opt.param_groups:
                g["lr"] = LR / (2 ** iscale)
        for it in range(ITERS):
            R = torch.zeros(V, 3, 3, device="cuda")
            for n in range(V):
                q = torch.zeros(4, device="cuda")
                misc.unitQ_to_quat(uq[n], q)
                R[n] = misc.quaternion2Rotation(q, torch.zeros(3, 3, device="cuda"))
            opt.zero_grad()
            wp = DepthWarp.apply(s, d, K, R, t, rays)
            m = 1.0 - (wp == 0).type_as(wp)
            cc = c.unsqueeze(0).unsqueeze(0).expand(V, 3, -1, -1)
            loss = loss_fn(wp * m * cc, r * m * cc)
            if it == 0 or it == ITERS - 1:
                loss.item()
            loss.backward()
            opt.step()
    return t.detach().cpu(), uq.detach().cpu()


def time_ms(fn, w, reps, warmup):
    for _ in range(warmup):
        fn(w)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(w)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out))


def fused_bytes(H, W):
    """Unique bytes one full-resolution nrgbd_lba_grad pass must read: sources 3N, reference 3, rays 3, depth 1, confidence 1
    planes of fp32 (the per-view re-reads of the shared planes and the tap overlap are served by the caches)."""
    return 4 * H * W * (3 * V + 3 + 3 + 1 + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="S,B")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.trace_only:
        for s in a.sizes.split(","):
            w = workload(*SIZES[s])
            for _ in range(3):
                fused_call(w)
        torch.cuda.synchronize()
        return 0
    res = {"version": ops.version(), "device": torch.cuda.get_device_name(0), "views": V, "dw_scales": SCALES,
           "iterations_per_scale": ITERS, "launches_per_call": 2 + 2 * ITERS * len(SCALES),
           "fused_kernel_time": "not measured here (rocprofv3 --kernel-trace --stats, separate run)"}
    for s in a.sizes.split(","):
        H, W = SIZES[s]
        w = workload(H, W)
        f_med, f_min = time_ms(fused_call, w, a.reps, a.warmup)
        e_med, e_min = time_ms(eager_call, w, max(3, a.reps // 3), 1)
        res[s] = {"H": H, "W": W, "fused_ms_per_call": round(f_med, 3), "fused_ms_min": round(f_min, 3),
                  "eager_ms_per_call": round(e_med, 3), "eager_ms_min": round(e_min, 3),
                  "speedup": round(e_med / f_med, 2), "fused_grad_bytes_per_full_res_iteration": fused_bytes(H, W)}
        print(json.dumps({s: res[s]}), flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
