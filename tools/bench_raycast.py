"""TSDF ray-cast benchmark: nrgbd_tsdf_raycast_f32 (one launch per view) beside the same march written with torch operations on the
device (one grid_sample per step), at 128^3 and 256^3 voxels with views of 256 x 384 and 768 x 1024; and FusionVideoStream with one
render per frame beside the bare stream at config B.

    python tools/bench_raycast.py [--reps 50] [--warmup 5] [--repeats 3] [--json out.json]
    python tools/bench_raycast.py --trace-only --grid 256 --size 768x1024 --form hip [--normals]
                  # 20 calls of one form for `rocprofv3 --kernel-trace --stats -- python ...`
    python tools/bench_raycast.py --stats <kernel_stats.csv> [...]   # such a run's kernel time and launches per call
    python tools/bench_raycast.py --stream [--frames 40]             # frames/s of the two streams at config B, same process

Scene: the plane of tests/tsdf_ref.py fused from three poses near the origin into a 2.56 m cube from (-1.28, -1.28, 0.6), trunc = 3
voxels, seen from a fourth pose; one sample per voxel along the ray.  Samples and bytes per ray come from a counting pass of the torch
march (the same decisions up to rounding): a sample requests 8 weights (32 bytes) and, where they pass, 8 TSDF values (32 more) —
requested bytes, most of them cache hits, since neighbouring rays walk the same cells.  Timing: HIP events around `reps` back-to-back
calls after `warmup` untimed ones, per call; kernel durations come from the kernel trace (--trace-only)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from neuralrgbd_amd import camera, fusion, ops, synth  # noqa: E402

DEV = "cuda:0"
TRACE_CALLS = 20
SIZES = {"256x384": (256, 384), "768x1024": (768, 1024)}
GRIDS = (128, 256)
DEPTH_RANGE = (0.3, 3.0)


def time_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def scene(n, size):
    import tsdf_ref as ref
    H, W = SIZES[size]
    K = fusion.intrinsics_at(camera.scannet_intrinsics(W, H), H, W)
    rng = np.random.RandomState(7)
    poses = [synth.random_pose(rng, 0.08, 0.15) for _ in range(4)]
    vol = fusion.TSDFVolume((n, n, n), 2.56 / n, (-1.28, -1.28, 0.6), device=DEV)
    for m in poses[:3]:
        vol.integrate(torch.from_numpy(ref.plane_depth(m, K, H, W)).to(DEV), m, K, depth_range=DEPTH_RANGE)
    return vol, poses[3], K, (H, W)


def torch_march(vol, extM, K, size, count=False):
    """The march of include/nrgbd.h with torch operations: per step one grid_sample of (tsdf, weights pass) at every ray's sample and a
    handful of element-wise kernels over the image (fp32; not the kernel's bits).  The number of steps is the longest ray's, found
    before the loop (one read-back).  count=True: also (samples, VALID samples) per ray up to its hit."""
    H, W = size
    X, Y, Z = vol.dims
    fx, fy, cx, cy = K
    p = torch.from_numpy(np.float32(extM[:3, :4])).to(DEV)
    c = torch.from_numpy(ops.camera_centre(extM)).to(DEV)
    xn = ((torch.arange(W, device=DEV, dtype=torch.float32) + 0.5 - cx) / fx)[None, :].expand(H, W)
    yn = ((torch.arange(H, device=DEV, dtype=torch.float32) + 0.5 - cy) / fy)[:, None].expand(H, W)
    d = torch.stack([p[0, k] * xn + p[1, k] * yn + p[2, k] for k in range(3)], -1)
    dzs = vol.voxel_size / d.norm(dim=-1)
    o = torch.tensor(vol.origin, device=DEV)
    go, gd = (c - o) / vol.voxel_size, d / vol.voxel_size
    last = torch.tensor([X - 1., Y - 1., Z - 1.], device=DEV)
    ta, tb = (0. - go) / gd, (last - go) / gd
    z0 = torch.minimum(ta, tb).amax(-1).clamp(min=DEPTH_RANGE[0])
    z1 = torch.maximum(ta, tb).amin(-1).clamp(max=DEPTH_RANGE[1])
    steps = int(((z1 - z0) / dzs).clamp(min=-1).max().item()) + 1
    field = torch.stack([vol.tsdf, (vol.weight >= 1.).float()])[None]
    depth = torch.zeros(H, W, device=DEV)
    done = ~(z0 <= z1)
    prev_ok = torch.zeros(H, W, dtype=torch.bool, device=DEV)
    prev_T, prev_z = torch.zeros(H, W, device=DEV), torch.zeros(H, W, device=DEV)
    n_s, n_v = torch.zeros(H, W, device=DEV), torch.zeros(H, W, device=DEV)
    for k in range(steps):
        zk = z0 + k * dzs
        g = (go + zk[..., None] * gd) / last * 2. - 1.
        s = F.grid_sample(field, g[None, None], mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0]
        live = ~done & (zk <= z1)
        ok = live & (s[1] > 0.999) & (g.abs() <= 1.).all(-1)        # all eight weights pass (up to the rounding of the blend)
        hit = ok & prev_ok & (prev_T > 0) & (s[0] <= 0)
        depth = torch.where(hit, prev_z + dzs * prev_T / (prev_T - s[0]), depth)
        if count:
            n_s += live
            n_v += ok
        done = done | hit | ~live
        prev_ok, prev_T, prev_z = ok, s[0], zk
    return (depth, steps, float(n_s.mean()), float(n_v.mean())) if count else depth


def forms(n, size, normals=False):
    vol, extM, K, hw = scene(n, size)
    out = (torch.empty(hw, device=DEV), torch.empty((3,) + hw, device=DEV))
    return {"hip": lambda: vol.raycast(extM, K, hw, depth_range=DEPTH_RANGE, normals=normals, out=out if normals else out[0]),
            "torch": lambda: torch_march(vol, extM, K, hw)}, vol, extM, K, hw


def stats_per_call(path):
    """{kernel name: (microseconds, launches) per call} of a rocprofv3 --kernel-trace --stats run of --trace-only (TRACE_CALLS + 1 calls)."""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            out[row["Name"]] = (float(row["TotalDurationNs"]) / 1e3 / (TRACE_CALLS + 1), float(row["Calls"]) / (TRACE_CALLS + 1))
    return out


def stream_rates(frames):
    """frames/s of the bare VideoDepthStream and of FusionVideoStream (256^3 volume) with one render(normals=True) per frame at
    config B (1024 x 768 images, 64 candidates), hipGraph, same process and lease, wall time over `frames` pushes."""
    import neuralrgbd_amd
    import video_ref as vr
    from neuralrgbd_amd import video
    H, W, D, r = 768, 1024, 64, 2
    cam, d_candi = camera.scannet_intrinsics(W // 4, H // 4), np.linspace(0.1, 5, D)
    model = neuralrgbd_amd.KVNET(64, cam, d_candi, 10.0, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=r)
    model.load_state_dict(synth.seeded_state_dict(model, 0))
    model = model.to(DEV)
    imgs = [torch.from_numpy(f).to(DEV) for f in vr.noise_frames(5, 8, H, W)]
    extMs = vr.trajectory(6, frames + 12)
    out = {}
    for name in ("video", "fusion", "fusion_render", "video_again"):
        if name.startswith("fusion"):
            vol = fusion.TSDFVolume((256, 256, 256), 0.02, (-2.56, -2.56, 0.2), device=DEV)
            s = fusion.FusionVideoStream(model, cam, d_candi, vol, t_win_r=r, depth_range=(0.2, 4.9), use_graph=True)
            buf = (torch.empty((H, W), device=DEV), torch.empty((3, H, W), device=DEV))
        else:
            s = video.VideoDepthStream(model, cam, d_candi, t_win_r=r, use_graph=True)

        def push(i):
            s.push(imgs[i % len(imgs)], extMs[i])
            if name == "fusion_render" and s.n_integrated:
                s.render(normals=True, out=buf)
        for i in range(12):                                         # first frame, eager update frame, capture, replays
            push(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(12, 12 + frames):
            push(i)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        s.check()
        out[name] = {"frames_per_s": frames / dt, "ms_per_frame": 1e3 * dt / frames}
        if name == "fusion_render":
            out[name]["pixels_hit"] = int((buf[0] > 0).sum())
        print("%-14s %.2f frames/s (%.2f ms per frame over %d pushes)" % (name, frames / dt, 1e3 * dt / frames, frames))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--grid", type=int, choices=GRIDS, default=256)
    ap.add_argument("--size", choices=sorted(SIZES), default="768x1024")
    ap.add_argument("--form", choices=("hip", "torch"), default="hip")
    ap.add_argument("--normals", action="store_true")
    ap.add_argument("--stats", nargs="*", default=None)
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--frames", type=int, default=40)
    a = ap.parse_args()
    if a.stats is not None:
        for path in a.stats:
            per = stats_per_call(path)
            print("%s: %.2f us of kernels and %.1f launches per call" % (path, sum(v[0] for v in per.values()), sum(v[1] for v in per.values())))
            for name, (us, calls) in sorted(per.items(), key=lambda kv: -kv[1][0])[:8]:
                print("    %8.2f us  %6.1f x  %s" % (us, calls, name[:100]))
        return 0
    if a.trace_only:
        fn = forms(a.grid, a.size, a.normals)[0][a.form]
        for _ in range(TRACE_CALLS + 1):
            fn()
        torch.cuda.synchronize()
        return 0
    out = {"version": ops.version()}
    if a.stream:
        out["stream"] = stream_rates(a.frames)
    else:
        for n in GRIDS:
            for size in sorted(SIZES):
                res = {}
                fs, vol, extM, K, hw = forms(n, size)
                depth, steps, per_ray, valid_per_ray = torch_march(vol, extM, K, hw, count=True)
                hip = fs["hip"]().clone()
                hits = int((hip > 0).sum())
                close = float(((hip - depth).abs() < 1e-3)[hip > 0].float().mean()) if hits else 0.0
                res["scene"] = {"pixels": hw[0] * hw[1], "hits": hits, "torch_agrees_within_1mm": close, "torch_steps": steps,
                                "samples_per_ray": per_ray, "valid_samples_per_ray": valid_per_ray,
                                "requested_bytes_per_ray": 32 * (per_ray + valid_per_ray)}
                for normals in (False, True):
                    fn = forms(n, size, normals)[0]["hip"]
                    t = [time_ms(fn, a.reps, a.warmup) for _ in range(a.repeats)]
                    med = float(np.median(t))
                    res["hip_normals" if normals else "hip"] = {"ms": t, "median_ms": med, "spread_ms": max(t) - min(t),
                                                                "ns_per_sample": 1e6 * med / (per_ray * hw[0] * hw[1])}
                    print("%d^3 %-9s hip%s %.4f ms per call (spread %.4f)  %d of %d pixels hit, %.1f samples (%.1f valid) = %.0f requested "
                          "bytes per ray, %.3f ns per sample" % (n, size, " +normals" if normals else "         ", med, max(t) - min(t), hits,
                                                                 hw[0] * hw[1], per_ray, valid_per_ray, 32 * (per_ray + valid_per_ray),
                                                                 1e6 * med / (per_ray * hw[0] * hw[1])))
                t = [time_ms(fs["torch"], max(a.reps // 10, 3), 1) for _ in range(a.repeats)]
                res["torch"] = {"ms": t, "median_ms": float(np.median(t)), "spread_ms": max(t) - min(t), "steps": steps}
                print("%d^3 %-9s torch          %.4f ms per call (spread %.4f), %d steps; agrees with the kernel within 1 mm on %.4f of its hits"
                      % (n, size, res["torch"]["median_ms"], max(t) - min(t), steps, close))
                out["%d_%s" % (n, size)] = res
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
