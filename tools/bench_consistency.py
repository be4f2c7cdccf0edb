"""The multi-view depth consistency launch, measured: ops.depth_consistency at 192 x 256 and 768 x 1024 with 1, 4, 8 and 16 sources,
without and with gates, votes and the filtered map both written.

    python tools/bench_consistency.py [--reps 200] [--warmup 20] [--repeats 5] [--json out.json]

Scene: a smooth surface 1.3 - 1.8 m away seen from cameras a few centimetres apart (tests/consistency_ref.py's seeded maps without the
seeded holes: every pixel is valid, every source is read), the sources a stack of n_src maps.  Timing: HIP events, per launch, two
ways — `reps` launches captured into one graph and replayed (the kernel and the gap between two kernels: the figure the rates are
formed from), and `reps` back-to-back eager calls after `warmup` untimed ones (the Python wrapper's host time included, which is what
a small launch costs a caller); the cases alternate, `repeats` times each, in one process; medians and spreads are printed.  Bytes: what the launch has to move — the reference map, one gather of 4 bytes per pixel and source (two with
gates: 8), two maps written — over the time, beside bench.py's HBM_PEAK_GBS.  The working set of the largest case (16 sources with
gates at 768 x 1024: 110 MB) fits the 256 MiB Infinity Cache and the launches repeat on the same maps, so the rate is a cache-resident
one, not an HBM rate; it says how far the launch is from the memory system's ceiling, not what a cold frame costs."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralrgbd_amd import ops, synth  # noqa: E402

DEV = "cuda:0"
SIZES = ((192, 256), (768, 1024))
N_SRC = (1, 4, 8, 16)
HBM_PEAK_GBS = 8000.0           # bench.py's
REL, DEPTH_RANGE, GATE_THR = 0.01, (0.1, 10.0), 0.15


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


def captured(fn, reps):
    """`reps` launches captured into one graph: its replay leaves the wrapper's host time (argument checks, ctypes) out."""
    from neuralrgbd_amd.distributed import graph_capture_mode
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=graph_capture_mode()):
        for _ in range(reps):
            fn()
    return g


def scene(H, W, n_src, gated):
    rng = np.random.RandomState(1000 * H + n_src)
    Y, X = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = 1.5 + 0.2 * np.sin(X / (W / 12.0)) + 0.1 * np.cos(Y / (H / 12.0))
    noisy = lambda: torch.from_numpy((base * (1.0 + REL * rng.choice([0.0, 0.5, -0.5, 1.5], (H, W)))).astype(np.float32)).to(DEV)
    gate = lambda: torch.from_numpy((0.2 + 0.8 * rng.rand(H, W)).astype(np.float32)).to(DEV)
    T = []
    for _ in range(n_src):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = synth.rotvec_to_R(rng.normal(0, 0.01, 3)), rng.normal(0, 0.02, 3)
        T.append(m[:3])
    K = (0.9 * W, 0.9 * W, W / 2.0, H / 2.0)
    args = dict(src_T=np.stack(T), rel_thr=REL, min_views=min(2, n_src), depth_range=DEPTH_RANGE,
                votes=torch.empty(H, W, device=DEV), depth_out=torch.empty(H, W, device=DEV))
    if gated:
        args.update(gate=gate(), gate_thr=GATE_THR, src_gate=torch.stack([gate() for _ in range(n_src)]))
    depth, stack = noisy(), torch.stack([noisy() for _ in range(n_src)])
    return lambda: ops.depth_consistency(depth, K, stack, **args), args["votes"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_consistency: no GPU (nothing is measured without one)")
    out = {"version": ops.version(), "hbm_peak_gbs": HBM_PEAK_GBS, "cases": {}}
    for H, W in SIZES:
        cases = {}
        for gated in (False, True):
            for n in N_SRC:
                fn, votes = scene(H, W, n, gated)
                fn()
                torch.cuda.synchronize()
                per = (2 if gated else 1) * 4
                agreeing = float(votes.clamp(min=0).mean())
                graph = captured(fn, a.reps)
                cases["%dx%d n_src %2d %s" % (H, W, n, "gated" if gated else "plain")] = dict(
                    fn=fn, graph=graph, bytes=H * W * (per * (1 + n) + 8), agreeing=agreeing)
        t, tg = {k: [] for k in cases}, {k: [] for k in cases}
        for _ in range(a.repeats):                                  # alternating: what else runs on the host touches all alike
            for k, c in cases.items():
                t[k].append(time_ms(c["fn"], a.reps, a.warmup))
                tg[k].append(time_ms(c["graph"].replay, 3, 1) / a.reps)
        for k, c in cases.items():
            med, eager = float(np.median(tg[k])), float(np.median(t[k]))
            gbs = c["bytes"] / med / 1e6
            out["cases"][k] = dict(median_us=1e3 * med, spread_us=1e3 * (max(tg[k]) - min(tg[k])), eager_call_us=1e3 * eager,
                                   bytes=c["bytes"], gb_per_s=gbs, frac_of_hbm_peak=gbs / HBM_PEAK_GBS, mean_agreeing=c["agreeing"])
            print("%-28s %8.2f us per launch in a graph (spread %.2f), %8.2f us per eager call   %6.2f MB   %7.1f GB/s = %.3f of %g   "
                  "mean agreeing %.2f" % (k, 1e3 * med, 1e3 * (max(tg[k]) - min(tg[k])), 1e3 * eager, c["bytes"] / 1e6, gbs,
                                          gbs / HBM_PEAK_GBS, HBM_PEAK_GBS, c["agreeing"]))
        del cases
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
