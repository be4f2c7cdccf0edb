"""Depth-evaluation benchmark: nrgbd_depth_eval (two launches: depth_eval_kernel and depth_eval_finalize_kernel, totals on the device)
beside the same figures computed with torch operations on the device (masking, divisions, log, comparisons, sums and the .item()
calls they force), at 256 x 384 and 768 x 1024 with J = 1 and J = 8 confidence sets.

    python tools/bench_eval.py [--reps 200] [--warmup 20] [--repeats 3] [--json out.json]
    python tools/bench_eval.py --trace-only --size 768x1024 --sets 8 --form hip
                  # 50 calls of one form at one size for `rocprofv3 --kernel-trace --stats -- python ...`
    python tools/bench_eval.py --stats <kernel_stats.csv> [...]      # such a run's kernel time and launches per call (50 calls)

Timing: HIP events around `reps` back-to-back calls after `warmup` untimed ones, per call.  The kernels take microseconds: the per-call
figure of the HIP form is bounded below by the rate at which the host issues the calls, so the kernels' own durations come from the
kernel trace (--trace-only), and between back-to-back calls every byte stays in the last-level cache.  Bytes: depth_eval_kernel reads
12 per pixel (depth, confidence, ground truth) and writes 4 with err_map.  The torch form synchronises once per .item(): its per-call
figure is wall time of a blocking evaluation, which is what a validation loop written with library operations pays."""
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

from neuralrgbd_amd import evaluate, ops  # noqa: E402

DEV = "cuda:0"
HBM_TBS = 8.0
TRACE_CALLS = 50
SIZES = {"256x384": (256, 384), "768x1024": (768, 1024)}
CONFS = {1: (0.,), 8: (0., .1, .2, .3, .4, .5, .6, .7)}
GT_RANGE = (0.75, 7.0)


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


def forms(size, J):
    import depth_eval_ref as ref
    H, W = SIZES[size]
    conf = CONFS[J]
    d, m, g = (torch.from_numpy(a.reshape(H, W)).to(DEV) for a in ref.make_inputs(H * W, 1, conf))
    ev = evaluate.DepthMetrics(conf, GT_RANGE, device=DEV)
    err = torch.empty_like(d)
    thr = [float(t) for t in ev.log_thr]

    def torch_form():
        """One frame's metrics per confidence set with device operations, read back as Python floats."""
        valid = (g > 0) & (g >= GT_RANGE[0]) & (g <= GT_RANGE[1])
        ok = valid & (d > 0) & torch.isfinite(d) & ~torch.isnan(m)
        err.copy_((g - d).abs() * (g > 0))
        dd, gd = d.double(), g.double()
        e = dd - gd
        q = dd / gd
        lg = torch.log(q)
        r = torch.maximum(q, gd / dd)
        out = []
        for t in thr:
            s = ok & (m >= t)
            n = s.sum().item()
            rec = [n]
            for term in (e.abs(), e.abs() / gd, e * e / gd, e * e, lg * lg, lg):
                rec.append(torch.where(s, term, 0.0).sum().item())
            for edge in (1.25, 1.5625, 1.953125):
                rec.append((s & (r < edge)).sum().item())
            out.append(rec)
        return out

    return {"hip": lambda: ev.update(d, m, g, err), "torch": torch_form}, ev, (d, m, g)


def stats_per_call(path):
    """{kernel name: (microseconds, launches) per call} of a rocprofv3 --kernel-trace --stats run of --trace-only (TRACE_CALLS + 1 calls)."""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            out[row["Name"]] = (float(row["TotalDurationNs"]) / 1e3 / (TRACE_CALLS + 1), float(row["Calls"]) / (TRACE_CALLS + 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--size", choices=sorted(SIZES), default="768x1024")
    ap.add_argument("--sets", type=int, choices=sorted(CONFS), default=8)
    ap.add_argument("--form", choices=("hip", "torch"), default="hip")
    ap.add_argument("--stats", nargs="*", default=None)
    a = ap.parse_args()
    if a.stats is not None:
        for path in a.stats:
            per = stats_per_call(path)
            print("%s: %.2f us of kernels and %.1f launches per call" % (path, sum(v[0] for v in per.values()), sum(v[1] for v in per.values())))
            for name, (us, calls) in sorted(per.items(), key=lambda kv: -kv[1][0])[:10]:
                print("    %8.2f us  %5.1f x  %s" % (us, calls, name[:100]))
        return 0
    if a.trace_only:
        fn = forms(a.size, a.sets)[0][a.form]
        for _ in range(TRACE_CALLS + 1):
            fn()
        torch.cuda.synchronize()
        return 0
    import depth_eval_ref as ref
    out = {"version": ops.version()}
    for size in sorted(SIZES):
        for J in sorted(CONFS):
            fs, ev, (d, m, g) = forms(size, J)
            ev.reset()
            fs["hip"]()
            want = ref.evaluate(d.cpu().numpy(), m.cpu().numpy(), g.cpu().numpy(), ev.log_thr, GT_RANGE)
            same = bool(np.array_equal(ev.frame[1].cpu().numpy(), want["counts"]))
            tf = fs["torch"]()
            same_torch = [int(rec[0]) for rec in tf] == want["counts"][:, 0].tolist()
            n = d.numel()
            res = {"pixels": n, "sets": J, "counts_equal_comparator": same, "torch_counts_equal_comparator": same_torch, "bytes": 16 * n}
            for form, fn in fs.items():
                t = [time_ms(fn, a.reps if form == "hip" else max(a.reps // 10, 5), a.warmup if form == "hip" else 3) for _ in range(a.repeats)]
                med = float(np.median(t))
                res[form] = {"ms": t, "median_ms": med, "spread_ms": max(t) - min(t), "hbm_fraction": 16 * n / (med * 1e-3) / (HBM_TBS * 1e12)}
                print("%-9s J=%d %-6s %.4f ms per call (spread %.4f)  %5.2f MB  = %.4f of %g TB/s" % (
                    size, J, form, med, max(t) - min(t), 16 * n / 1e6, res[form]["hbm_fraction"], HBM_TBS))
            print("%-9s J=%d counts equal to the float64 comparator: hip %s, torch %s" % (size, J, same, same_torch))
            out["%s_J%d" % (size, J)] = res
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
