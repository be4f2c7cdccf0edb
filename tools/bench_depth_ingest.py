"""Depth-label ingest benchmark: nrgbd_depth_ingest_u16 (one launch: both label maps and both metric maps of a uint16 depth frame)
beside the same work as torch operations on the device (index, multiply, bucketize, clamp), at ScanNet's sizes (480 x 640 ->
256 x 384 / 64 x 96, D = 64) and at config B's (480 x 640 -> 768 x 1024 / 192 x 256, D = 64).

    python tools/bench_depth_ingest.py [--reps 200] [--warmup 20] [--repeats 3] [--json out.json]
    python tools/bench_depth_ingest.py --trace-only --config scannet --form hip
                  # 50 calls of one form at one size for `rocprofv3 --kernel-trace --stats -- python ...`
    python tools/bench_depth_ingest.py --stats <kernel_stats.csv> [...]      # sums such a run's kernel time per call (50 calls)

Timing: HIP events around `reps` back-to-back calls after `warmup` untimed ones, per call.  The kernel takes microseconds: the
per-call figure is bounded below by the rate at which the host issues the calls, so the kernel's own duration comes from the kernel
trace (--trace-only), and between back-to-back calls every byte stays in the last-level cache.  Bytes: the frame is read at most once
(2 Hin Win) and 12 bytes are written per pixel of each map (8 label + 4 metres).  The torch form is NOT the loaders' arithmetic (its
bucketize compares fp32 metres with fp32 candidates): it stands for the cost of doing the work with library operations, not for
their result.  Host-to-device bytes per training step are printed too: one uint8 frame and one uint16 depth frame pushed, against the
five fp32 images and two int64 label maps of a prepared window."""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from neuralrgbd_amd import ops, train_video  # noqa: E402

DEV = "cuda:0"
HBM_TBS = 8.0
TRACE_CALLS = 50
CONFIGS = {"scannet": dict(frame=(480, 640), net=(256, 384), grid=(64, 96), D=64, rgb=(968, 1296)),
           "B": dict(frame=(480, 640), net=(768, 1024), grid=(192, 256), D=64, rgb=(968, 1296))}


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


def depth_frame(Hin, Win):
    rng = np.random.RandomState(0)
    d = rng.randint(300, 6000, (Hin, Win))
    d[rng.rand(Hin, Win) < 0.3] = 0
    return d.astype(np.uint16)


def forms(cfg):
    (Hin, Win), net, grid, D = cfg["frame"], cfg["net"], cfg["grid"], cfg["D"]
    d_candi = np.linspace(.1, 5, D)
    lab = train_video.DepthLabeler(d_candi, net, grid, device=DEV)
    host = depth_frame(Hin, Win)
    dev = torch.from_numpy(host.view(np.int16)).to(DEV)
    out = lab.empty_outputs()
    rf, cf, rq, cq, mr, mc = (t.long() for t in lab.tables(Hin, Win))
    wide = dev.to(torch.int32) & 0xFFFF                            # torch indexes no uint16: the frame widened once, outside the timing
    cand = torch.from_numpy(d_candi.astype(np.float32)).to(DEV)

    def torch_form():
        full = wide[rf][:, cf].float() * .001
        q = wide[rq][:, cq].float() * .001
        q = q * (wide[mr][:, mc] != 0)
        out["dmap_imgsize"][0].copy_(full)
        out["dmap_raw"][0].copy_(q)
        out["dmap_imgsize_digit"][0].copy_(torch.bucketize(full, cand, right=True).clamp_(0, D - 1))
        out["dmap"][0].copy_(torch.bucketize(q, cand, right=True).clamp_(0, D - 1))

    return {"hip": lambda: lab(dev, out=out), "hip_host_frame": lambda: lab(host, out=out), "torch": torch_form}, lab, host, out


def moved_bytes(cfg):
    (Hin, Win), (H, W), (h, w) = cfg["frame"], cfg["net"], cfg["grid"]
    return 2 * Hin * Win + 12 * (H * W + h * w)


def upload_bytes(cfg):
    (Hin, Win), (H, W), (h, w), (Hc, Wc) = cfg["frame"], cfg["net"], cfg["grid"], cfg["rgb"]
    return {"pushed_per_step": 3 * Hc * Wc + 2 * Hin * Win, "prepared_window_per_step": 5 * 12 * H * W + 8 * (H * W + h * w)}


def stats_us_per_call(path):
    """{kernel name: microseconds per call} of a rocprofv3 --kernel-trace --stats run of --trace-only (TRACE_CALLS + 1 calls)."""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            out[row["Name"]] = float(row["TotalDurationNs"]) / 1e3 / (TRACE_CALLS + 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="scannet")
    ap.add_argument("--form", choices=("hip", "torch"), default="hip")
    ap.add_argument("--stats", nargs="*", default=None)
    a = ap.parse_args()
    if a.stats is not None:
        for path in a.stats:
            per = stats_us_per_call(path)
            print("%s: %.2f us of kernels per call" % (path, sum(per.values())))
            for name, us in sorted(per.items(), key=lambda kv: -kv[1])[:12]:
                print("    %8.2f us  %s" % (us, name[:110]))
        return 0
    if a.trace_only:
        fn = forms(CONFIGS[a.config])[0][a.form]
        for _ in range(TRACE_CALLS + 1):                          # (the first call uploads the tables)
            fn()
        torch.cuda.synchronize()
        return 0
    import train_video_ref as tr
    out = {"version": ops.version()}
    for name, cfg in sorted(CONFIGS.items()):
        fs, lab, host, o = forms(cfg)
        fs["hip"]()
        want = tr.prepare_depth(host, cfg["net"], cfg["grid"], np.linspace(.1, 5, cfg["D"]))
        same = all(torch.equal(v.cpu(), want[k]) for k, v in o.items())
        res = {"sizes": cfg, "hip_equals_pillow_and_digitize": same, "bytes": moved_bytes(cfg), "host_to_device": upload_bytes(cfg)}
        for form, fn in fs.items():
            t = [time_ms(fn, a.reps, a.warmup) for _ in range(a.repeats)]
            med = float(np.median(t))
            res[form] = {"ms": t, "median_ms": med, "spread_ms": max(t) - min(t),
                         "hbm_fraction": moved_bytes(cfg) / (med * 1e-3) / (HBM_TBS * 1e12)}
            print("%-8s %-15s %.4f ms per call (spread %.4f)  %5.2f MB  = %.4f of %g TB/s" % (
                name, form, med, max(t) - min(t), moved_bytes(cfg) / 1e6, res[form]["hbm_fraction"], HBM_TBS))
        up = upload_bytes(cfg)
        print("%-8s bit-equal to the Pillow / np.digitize comparator: %s;  host-to-device per training step: %.2f MB pushed (uint8 %dx%d "
              "frame + uint16 depth) against %.2f MB of a prepared window" % (name, same, up["pushed_per_step"] / 1e6, cfg["rgb"][0],
                                                                                cfg["rgb"][1], up["prepared_window_per_step"] / 1e6))
        out[name] = res
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
