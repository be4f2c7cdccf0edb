"""Frame-to-model tracking benchmark: nrgbd_icp_terms_f32 and nrgbd_icp_update alone, the ray casts of the tracker's three levels, and
a whole TSDFVolume.track() at the default levels ((4, 10), (2, 5), (1, 4): 19 iterations, 3 ray casts, 42 launches, one read-back),
on a 256^3 volume with a 768 x 1024 map (config B's image, the size of its refined maps) and a 192 x 256 map (config B's plane-sweep
grid, the size of source='dpv').

    python tools/bench_icp.py [--reps 50] [--warmup 5] [--repeats 3] [--json out.json]
    python tools/bench_icp.py --photo ...                       # also the photometric track (colour ICP) beside the geometric one
    python tools/bench_icp.py --trace-only --size 768x1024     # 20 track() calls for `rocprofv3 --kernel-trace --stats -- python ...`
    python tools/bench_icp.py --stats <kernel_stats.csv> [...]  # such a run's kernel time and launches per track()

Scene: the room corner of tests/icp_ref.py (three walls, all six degrees of freedom constrained) as an analytic field in a 2.56 m
cube of 256^3 voxels, trunc = 3 voxels; the frame is the volume's own ray cast from the true pose, the track starts 2 cm / 0.04 rad
off.  Timing: HIP events around `reps` back-to-back calls after `warmup` untimed ones, per call, the median of `repeats` such
measurements and their spread; track() ends with a device-to-host copy, so its event time is also its wall time (printed beside
it); the calls of one entry timed back to back give its call period (launch included), the kernels' own durations come from the
kernel trace (--trace-only).  --photo: the volume also carries a texture (tests/icp_photo_ref.texture, sheared along z), the frame's
picture is its own colour ray cast, and every level's colour ray cast, icp_terms_photo and a whole track(image=...) are timed
beside the geometric ones, in total and per icp_terms_photo launch.  There is no other implementation to compare with: the numbers say where a tracked frame's time goes."""
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

from neuralrgbd_amd import fusion, ops, tracking  # noqa: E402

DEV = "cuda:0"
SIZES = {"768x1024": (768, 1024), "192x256": (192, 256)}
N, EXTENT = 256, 2.56
TRACE_CALLS = 20


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


def measure(fn, a):
    t = [time_ms(fn, a.reps, a.warmup) for _ in range(a.repeats)]
    return {"ms": t, "median_ms": float(np.median(t)), "spread_ms": max(t) - min(t)}


def scene(photo=False):
    import icp_ref as ir
    vs = EXTENT / N
    origin = (-1.2, -1.2, 0.0)
    field = ir.corner_field((N, N, N), origin, vs, 3 * vs, ir.CORNER["planes"])
    vol = fusion.TSDFVolume((N, N, N), vs, origin, device=DEV, color=photo)
    vol.tsdf.copy_(torch.from_numpy(field[0]))
    vol.weight.copy_(torch.from_numpy(field[1]))
    if photo:                                                       # plane by plane: the host never holds 3 x 256^3 float64
        import icp_photo_ref as pr
        x, y, z = pr.lattice((N, N, N), origin, vs)
        for k in range(N):
            vol.color[:, k].copy_(torch.from_numpy(pr.texture(x[0] + z[k], y[0] + z[k]).astype(np.float32)))
    truth, guess = ir.corner_poses()
    return vol, truth, guess, ir


def stats_per_call(path):
    """{kernel name: (microseconds, launches) per track()} of a rocprofv3 --kernel-trace --stats run of --trace-only."""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            out[row["Name"]] = (float(row["TotalDurationNs"]) / 1e3 / TRACE_CALLS, float(row["Calls"]) / TRACE_CALLS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--size", choices=sorted(SIZES), default="768x1024")
    ap.add_argument("--stats", nargs="*", default=None)
    ap.add_argument("--photo", action="store_true")
    a = ap.parse_args()
    if a.stats is not None:
        for path in a.stats:
            per = stats_per_call(path)
            print("%s: %.2f us of kernels and %.1f launches per track()" % (path, sum(v[0] for v in per.values()), sum(v[1] for v in per.values())))
            for name, (us, calls) in sorted(per.items(), key=lambda kv: -kv[1][0])[:8]:
                print("    %8.2f us  %6.1f x  (%.2f us each)  %s" % (us, calls, us / max(calls, 1e-9), name[:90]))
        return 0
    vol, truth, guess, ir = scene(a.photo)
    if a.trace_only:                                                # the scene's two launches (upload, frame) are in the trace as well
        H, W = SIZES[a.size]
        K = (0.9375 * W, 0.9375 * W, W / 2.0, H / 2.0)
        depth, picture = vol.raycast(truth, K, (H, W), color=True) if a.photo else (vol.raycast(truth, K, (H, W)), None)
        kw = dict(image=picture) if a.photo else {}
        for _ in range(TRACE_CALLS):
            vol.track(depth, guess, K, **kw)
        torch.cuda.synchronize()
        return 0
    out = {"version": ops.version(), "volume": N, "levels": tracking.DEFAULT_LEVELS}
    for name, (H, W) in sorted(SIZES.items()):
        K = (0.9375 * W, 0.9375 * W, W / 2.0, H / 2.0)              # the fixture's field of view
        depth = vol.raycast(truth, K, (H, W))
        res = {"pixels": H * W, "hits": int((depth > 0).sum())}
        tracker = tracking.FrameTracker(vol, (H, W), K)
        r = vol.track(depth, guess, K)
        e0, e1 = ir.pose_error(guess, truth), ir.pose_error(r.extM, truth)
        res["track_result"] = {"ok": r.ok, "start_m_rad": e0, "end_m_rad": e1, "pairs_per_level": [float(r.log[i, 0]) for i in (0, 10, 15)]}
        print("%s: track ok=%s, %.3g m / %.3g rad -> %.3g m / %.3g rad, pairs %s" % (name, r.ok, e0[0], e0[1], e1[0], e1[1],
                                                                                  res["track_result"]["pairs_per_level"]))
        ops.icp_update(tracker._state, 0)
        for sub, iters, (Hs, Ws), Kl, maps in tracker._levels:
            cast = lambda: vol.raycast(guess, Kl, (Hs, Ws), normals=True, out=maps)
            res["raycast_sub%d" % sub] = measure(cast, a)
            nwg = ops.icp_workgroups(Hs, Ws)
            terms = lambda: ops.icp_terms(depth, tracker.K, sub, maps[0], maps[1], Kl, tracker._state, tracker._partial,
                                          2 * vol.trunc, vol.voxel_size)
            res["terms_sub%d" % sub] = dict(measure(terms, a), visited=Hs * Ws, workgroups=nwg)
            update = lambda: ops.icp_update(tracker._state, 1, tracker._partial, nwg, min_pairs=6, log=tracker._log)
            res["update_sub%d" % sub] = measure(update, a)
            ops.icp_update(tracker._state, 0)                       # the timed updates moved the state: start the next level afresh
            print("%s sub %d (%d x %d, %d workgroups): raycast %.4f ms, icp_terms %.4f ms, icp_update %.4f ms (spreads %.4f / %.4f / %.4f)"
                  % (name, sub, Hs, Ws, nwg, res["raycast_sub%d" % sub]["median_ms"], res["terms_sub%d" % sub]["median_ms"],
                     res["update_sub%d" % sub]["median_ms"], res["raycast_sub%d" % sub]["spread_ms"], res["terms_sub%d" % sub]["spread_ms"],
                     res["update_sub%d" % sub]["spread_ms"]))
        res["track"] = measure(lambda: vol.track(depth, guess, K), a)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            vol.track(depth, guess, K)
        res["track"]["wall_ms"] = 1e3 * (time.perf_counter() - t0) / a.reps
        parts = sum(res["raycast_sub%d" % s]["median_ms"] + n * (res["terms_sub%d" % s]["median_ms"] + res["update_sub%d" % s]["median_ms"])
                    for s, n in tracker.levels)
        res["track"]["sum_of_parts_ms"] = parts
        print("%s: track() %.4f ms per call (spread %.4f; wall %.4f ms; its launches timed alone add up to %.4f ms)"
              % (name, res["track"]["median_ms"], res["track"]["spread_ms"], res["track"]["wall_ms"], parts))
        if a.photo:
            picture = vol.raycast(truth, K, (H, W), color=True)[1]
            ptracker = tracking.FrameTracker(vol, (H, W), K, photo=True)
            r = vol.track(depth, guess, K, image=picture)
            e1 = ir.pose_error(r.extM, truth)
            res["photo_track_result"] = {"ok": r.ok, "end_m_rad": e1}
            print("%s: photometric track ok=%s, -> %.3g m / %.3g rad" % (name, r.ok, e1[0], e1[1]))
            ops.icp_update(ptracker._state, 0)
            for sub, iters, (Hs, Ws), Kl, maps in ptracker._levels:
                cast = lambda: vol.raycast(guess, Kl, (Hs, Ws), normals=True, out=maps, color=True)
                res["raycast_color_sub%d" % sub] = measure(cast, a)
                terms = lambda: ops.icp_terms_photo(depth, ptracker.K, sub, maps[0], maps[1], Kl, ptracker._state, ptracker._partial,
                                                    2 * vol.trunc, vol.voxel_size, picture, maps[2], 0.1, 0.1)
                res["terms_photo_sub%d" % sub] = dict(measure(terms, a), visited=Hs * Ws)
                print("%s sub %d: colour raycast %.4f ms (depth and normals alone %.4f), icp_terms_photo %.4f ms (icp_terms %.4f); spreads "
                      "%.4f / %.4f" % (name, sub, res["raycast_color_sub%d" % sub]["median_ms"], res["raycast_sub%d" % sub]["median_ms"],
                                       res["terms_photo_sub%d" % sub]["median_ms"], res["terms_sub%d" % sub]["median_ms"],
                                       res["raycast_color_sub%d" % sub]["spread_ms"], res["terms_photo_sub%d" % sub]["spread_ms"]))
            res["photo_track"] = measure(lambda: vol.track(depth, guess, K, image=picture), a)
            print("%s: track(image=) %.4f ms per call (spread %.4f) against %.4f ms geometric"
                  % (name, res["photo_track"]["median_ms"], res["photo_track"]["spread_ms"], res["track"]["median_ms"]))
        out[name] = res
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
