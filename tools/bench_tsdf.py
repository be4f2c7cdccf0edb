"""TSDF fusion benchmark: nrgbd_tsdf_integrate_f32 (one launch per depth frame) beside the same update written with torch operations
on the device, at 256^3 and 128^3 voxels with depth maps of 256 x 384 and 768 x 1024, with and without the frustum box; the three
extraction launches; and FusionVideoStream beside the bare VideoDepthStream at config B.

    python tools/bench_tsdf.py [--reps 100] [--warmup 10] [--repeats 3] [--json out.json]
    python tools/bench_tsdf.py --trace-only --grid 256 --size 768x1024 --form hip [--no-cull]
                  # 50 calls of one form for `rocprofv3 --kernel-trace --stats -- python ...`
    python tools/bench_tsdf.py --stats <kernel_stats.csv> [...]      # such a run's kernel time and launches per call
    python tools/bench_tsdf.py --stream [--frames 40]                # frames/s of the two streams at config B, same process

Scene: the plane of tests/tsdf_ref.py (normal ~ (0.1, -0.15, 1), 1.6 m away) seen from a pose near the origin; the volume is a 2.56 m
cube from (-1.28, -1.28, 0.6), trunc = 3 voxels.  A voxel is updated when it projects into the map and lies no further than trunc
behind the surface: the free space in front of the plane counts.  Timing: HIP events around `reps` back-to-back calls after `warmup`
untimed ones, per call; kernel durations come from the kernel trace (--trace-only).  Byte floor: an updated voxel moves 16 bytes (tsdf
and weight, read and written) — the depth map and the voxels that are only tested move less than that and are left out; it is set
against the 8 TB/s HBM peak, though a 128^3 volume (16.8 MB for both arrays) and a 256^3 one (134 MB) fit the 256 MB last-level cache
between back-to-back calls."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from neuralrgbd_amd import camera, fusion, ops, synth  # noqa: E402

DEV = "cuda:0"
HBM_TBS = 8.0
TRACE_CALLS = 50
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
    extM = synth.random_pose(np.random.RandomState(7), 0.08, 0.15)
    depth = torch.from_numpy(ref.plane_depth(extM, K, H, W)).to(DEV)
    vol = fusion.TSDFVolume((n, n, n), 2.56 / n, (-1.28, -1.28, 0.6), device=DEV)
    return vol, depth, extM, K


def torch_integrate(vol, depth, extM, K):
    """The update of include/nrgbd.h with torch operations over the whole grid (fp32; not the kernel's bits: ATen fuses and reorders)."""
    X, Y, Z = vol.dims
    H, W = depth.shape
    r = torch.from_numpy(np.float32(extM[:3, :4])).to(DEV)
    fx, fy, cx, cy = K
    o, vs = vol.origin, vol.voxel_size
    xw = o[0] + vs * torch.arange(X, device=DEV, dtype=torch.float32)[None, None, :]
    yw = o[1] + vs * torch.arange(Y, device=DEV, dtype=torch.float32)[None, :, None]
    zw = o[2] + vs * torch.arange(Z, device=DEV, dtype=torch.float32)[:, None, None]
    xc, yc, zc = (r[k, 0] * xw + r[k, 1] * yw + r[k, 2] * zw + r[k, 3] for k in range(3))
    u, v = fx * (xc / zc) + cx, fy * (yc / zc) + cy
    ok = (zc > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    iu, iv = torch.where(ok, u.floor(), 0.).long(), torch.where(ok, v.floor(), 0.).long()
    d = depth[iv, iu]
    s = d - zc
    ok = ok & torch.isfinite(d) & (d > DEPTH_RANGE[0]) & (d <= DEPTH_RANGE[1]) & ~(s < -vol.trunc)
    t = torch.clamp(s / vol.trunc, max=1.)
    T, Wt = vol.tsdf, vol.weight
    vol.tsdf.copy_(torch.where(ok, (T * Wt + t) / (Wt + 1.), T))
    vol.weight.copy_(torch.where(ok, torch.clamp(Wt + 1., max=vol.w_max), Wt))


def forms(n, size, cull=True):
    vol, depth, extM, K = scene(n, size)
    return {"hip": lambda: vol.integrate(depth, extM, K, depth_range=DEPTH_RANGE, cull=cull),
            "torch": lambda: torch_integrate(vol, depth, extM, K)}, vol, extM, K


def stats_per_call(path):
    """{kernel name: (microseconds, launches) per call} of a rocprofv3 --kernel-trace --stats run of --trace-only (TRACE_CALLS + 1 calls)."""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            out[row["Name"]] = (float(row["TotalDurationNs"]) / 1e3 / (TRACE_CALLS + 1), float(row["Calls"]) / (TRACE_CALLS + 1))
    return out


def stream_rates(frames):
    """frames/s of the bare VideoDepthStream and of FusionVideoStream (256^3 volume, refined source, confidence weights behind a gate)
    at config B (1024 x 768 images, grid 256 x 192, 64 candidates), hipGraph, same process and lease, wall time over `frames` pushes."""
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
    for name in ("video", "fusion", "video_again"):
        if name == "fusion":
            vol = fusion.TSDFVolume((256, 256, 256), 0.02, (-2.56, -2.56, 0.2), device=DEV)
            s = fusion.FusionVideoStream(model, cam, d_candi, vol, t_win_r=r, weight="conf", conf_threshold=0.01, depth_range=(0.2, 4.9),
                                         use_graph=True)
        else:
            s = video.VideoDepthStream(model, cam, d_candi, t_win_r=r, use_graph=True)
        for i in range(12):                                         # first frame, eager update frame, capture, replays
            s.push(imgs[i % len(imgs)], extMs[i])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(12, 12 + frames):
            s.push(imgs[i % len(imgs)], extMs[i])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        s.check()
        out[name] = {"frames_per_s": frames / dt, "ms_per_frame": 1e3 * dt / frames}
        if name == "fusion":
            out[name]["voxels_observed"] = int((vol.weight > 0).sum())
        print("%-12s %.2f frames/s (%.2f ms per frame over %d pushes)" % (name, frames / dt, 1e3 * dt / frames, frames))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--grid", type=int, choices=GRIDS, default=256)
    ap.add_argument("--size", choices=sorted(SIZES), default="768x1024")
    ap.add_argument("--form", choices=("hip", "torch", "extract"), default="hip")
    ap.add_argument("--no-cull", action="store_true")
    ap.add_argument("--stats", nargs="*", default=None)
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--frames", type=int, default=40)
    a = ap.parse_args()
    if a.stats is not None:
        for path in a.stats:
            per = stats_per_call(path)
            print("%s: %.2f us of kernels and %.1f launches per call" % (path, sum(v[0] for v in per.values()), sum(v[1] for v in per.values())))
            for name, (us, calls) in sorted(per.items(), key=lambda kv: -kv[1][0])[:12]:
                print("    %8.2f us  %5.1f x  %s" % (us, calls, name[:100]))
        return 0
    if a.trace_only:
        fs, vol = forms(a.grid, a.size, not a.no_cull)[:2]
        fn = fs[a.form] if a.form != "extract" else (lambda: vol.points(w_min=1.0))
        if a.form == "extract":
            fs["hip"]()
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
                for cull in (True, False):
                    fs, vol, extM, K = forms(n, size, cull)
                    fs["hip"]()
                    updated = int((vol.weight > 0).sum())
                    box = fusion.frustum_box(extM, K, SIZES[size], DEPTH_RANGE[1] + vol.trunc, vol)
                    launched = (box[3] - box[0]) * (box[4] - box[1]) * (box[5] - box[2]) if cull else n ** 3
                    t = [time_ms(fs["hip"], a.reps, a.warmup) for _ in range(a.repeats)]
                    med = float(np.median(t))
                    res["hip_cull" if cull else "hip_whole_grid"] = {
                        "ms": t, "median_ms": med, "spread_ms": max(t) - min(t), "voxels_updated": updated, "voxels_launched": launched,
                        "floor_bytes": 16 * updated, "hbm_fraction": 16 * updated / (med * 1e-3) / (HBM_TBS * 1e12)}
                    print("%d^3 %-9s hip %-10s %.4f ms per call (spread %.4f)  %d of %d voxels updated, %.1f MB = %.3f of %g TB/s" % (
                        n, size, "cull" if cull else "whole grid", med, max(t) - min(t), updated, launched, 16 * updated / 1e6,
                        res["hip_cull" if cull else "hip_whole_grid"]["hbm_fraction"], HBM_TBS))
                vol.reset()
                t = [time_ms(fs["torch"], max(a.reps // 10, 5), 2) for _ in range(a.repeats)]
                res["torch"] = {"ms": t, "median_ms": float(np.median(t)), "spread_ms": max(t) - min(t)}
                print("%d^3 %-9s torch            %.4f ms per call (spread %.4f)" % (n, size, res["torch"]["median_ms"], max(t) - min(t)))
                vol.reset()
                for _ in range(6):
                    fs["hip"]()
                t = [time_ms(lambda: vol.points(w_min=1.0), max(a.reps // 10, 5), 2) for _ in range(a.repeats)]
                pts, found = vol.points(w_min=1.0)
                res["extract"] = {"ms": t, "median_ms": float(np.median(t)), "points": found}
                print("%d^3 %-9s points()         %.4f ms per call (two passes: count, then write; %d points; includes the read-back)" % (
                    n, size, res["extract"]["median_ms"], found))
                out["%d_%s" % (n, size)] = res
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
