"""The moving TSDF volume's launch, measured: ops.tsdf_shift on a 256^3 grid with 2 and 5 planes, spill off and on, for the shifts
(8,0,0), (0,8,0), (0,0,8), (8,8,8) and (5,0,0) — the last takes the element source form (sx % 4 != 0).

    python tools/bench_shift.py [--reps 20] [--warmup 2] [--repeats 5] [--json out.json]

Yardsticks, measured in the same run: a device-to-device `copy_` of the same buffer (every byte read once and written once: the
floor of a launch that moves the whole volume), and the same result formed with torch device operations (one slice copy, a zero fill
per entering slab, and with spill one more slice fill of the source's two planes).  Timing: HIP events around `reps` launches captured
into one graph and replayed (the wrapper's host time left out), the cases alternated, `repeats` times each, in one process; medians
and spreads are printed.  Bytes: what the launch has to move — four bytes read per retained voxel and plane, four written per voxel
and plane, and with spill eight more written per retained voxel that is not on the rim — over the time, beside bench.py's
HBM_PEAK_GBS.  Two buffers of 5 x 256^3 floats are 671 MB, well past the 256 MiB Infinity Cache: HBM rates.  Two buffers of
2 x 256^3 floats are 268 MB, about the cache's size, and the launches repeat on them: those rates are helped by the cache (the copy_
itself comes out above the HBM peak there), so read the 2-plane figures against their copy_, not against the peak."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralrgbd_amd import ops  # noqa: E402

DEV = "cuda:0"
N = 256
SHIFTS = ((8, 0, 0), (0, 8, 0), (0, 0, 8), (8, 8, 8), (5, 0, 0))
HBM_PEAK_GBS = 8000.0           # bench.py's


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


def _slices(s, n):
    """Per axis (x, y, z): (dst slice that has a source, the source slice, dst slice that enters, source slice retained off the rim)."""
    out = []
    for v in s:
        if v >= 0:
            out.append((slice(0, n - v), slice(v, n), slice(n - v, n), slice(v + 1 if v else 0, n)))
        else:
            out.append((slice(-v, n), slice(0, n + v), slice(0, -v), slice(0, n + v - 1)))
    return out


def torch_shift(src, dst, s, spill):
    """The launch's result with torch device operations: a slice copy, a zero fill per entering slab, and the spill's slice fill."""
    (dx, fx, ex, rx), (dy, fy, ey, ry), (dz, fz, ez, rz) = _slices(s, src.shape[-1])
    dst[:, dz, dy, dx] = src[:, fz, fy, fx]
    if s[0]:
        dst[:, :, :, ex] = 0
    if s[1]:
        dst[:, :, ey, :] = 0
    if s[2]:
        dst[:, ez, :, :] = 0
    if spill:
        src[:2, rz, ry, rx] = 0


def moved_bytes(planes, s, spill, n):
    kept = [n - abs(v) for v in s]
    retained = kept[0] * kept[1] * kept[2]
    off_rim = 1
    for k, v in zip(kept, s):
        off_rim *= k - 1 if v else k
    return 4 * planes * (retained + n ** 3) + (8 * off_rim if spill else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shift: no GPU (nothing is measured without one)")
    out = {"version": ops.version(), "hbm_peak_gbs": HBM_PEAK_GBS, "grid": N, "cases": {}}
    src5, dst5 = torch.rand(5, N, N, N, device=DEV), torch.empty(5, N, N, N, device=DEV)
    # the torch form against the kernel once, on a small grid (bits), before anything is timed
    a_, b_, c_, d_ = (torch.rand(5, 32, 32, 32, device=DEV) for _ in range(4))
    c_.copy_(a_)
    for s in SHIFTS + ((-8, 4, -5),):
        for spill in (False, True):
            a_.copy_(c_)
            ops.tsdf_shift(a_, b_, s, spill=spill)
            want_src = a_.clone()
            a_.copy_(c_)
            d_.fill_(7.0)
            torch_shift(a_, d_, s, spill)
            assert torch.equal(b_, d_) and torch.equal(a_, want_src), "the torch form differs from the kernel at %s" % (s,)
    cases = {}
    for planes in (2, 5):
        src, dst = src5[:planes], dst5[:planes]
        assert src.is_contiguous() and dst.is_contiguous()
        cases["copy_ %d planes" % planes] = dict(fn=lambda src=src, dst=dst: dst.copy_(src), bytes=8 * planes * N ** 3, planes=planes)
        for spill in (False, True):
            for s in SHIFTS:
                key = "%d planes %s spill %d" % (planes, s, spill)
                cases[key] = dict(fn=lambda src=src, dst=dst, s=s, spill=spill: ops.tsdf_shift(src, dst, s, spill=spill),
                                  bytes=moved_bytes(planes, s, spill, N), planes=planes)
                cases[key + " torch"] = dict(fn=lambda src=src, dst=dst, s=s, spill=spill: torch_shift(src, dst, s, spill),
                                             bytes=moved_bytes(planes, s, spill, N), planes=planes)
    for c in cases.values():
        c["fn"]()
        torch.cuda.synchronize()
        c["graph"] = captured(c["fn"], a.reps)
    t = {k: [] for k in cases}
    for _ in range(a.repeats):                                      # alternating: what else runs on the machine touches all alike
        for k, c in cases.items():
            t[k].append(time_ms(c["graph"].replay, 2, a.warmup) / a.reps)
    med = {k: float(np.median(v)) for k, v in t.items()}
    for k, c in cases.items():
        copy = med["copy_ %d planes" % c["planes"]]
        tbs = c["bytes"] / med[k] / 1e9
        out["cases"][k] = dict(median_us=1e3 * med[k], spread_us=1e3 * (max(t[k]) - min(t[k])), bytes=c["bytes"], tb_per_s=tbs,
                               frac_of_hbm_peak=1e3 * tbs / HBM_PEAK_GBS, ratio_to_copy=med[k] / copy)
        print("%-38s %8.1f us per launch (spread %.1f)   %7.1f MB   %5.2f TB/s = %.3f of %g GB/s   %.3f x copy_"
              % (k, 1e3 * med[k], 1e3 * (max(t[k]) - min(t[k])), c["bytes"] / 1e6, tbs, 1e3 * tbs / HBM_PEAK_GBS, HBM_PEAK_GBS, med[k] / copy))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
