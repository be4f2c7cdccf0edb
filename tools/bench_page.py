"""The paged TSDF volume's launches, measured: ops.tsdf_blocks_gather / ops.tsdf_blocks_scatter on a 256^3 grid with 2 and 5 planes, for
the x slab a default follow step moves (8 x 256 x 256 voxels: 1,024 blocks) and for the corner set of an (8,8,8) shift (the three slabs'
union: 2,977 blocks), and the whole TSDFVolume.shift(store=...) with its host copy.

    python tools/bench_page.py [--reps 20] [--warmup 2] [--repeats 5] [--json out.json]

Yardstick, measured in the same run: the same voxels moved by torch slice copies into and out of contiguous staging tensors (one copy
for the slab, three for the corner set — the y and z slabs without what the x slab already holds).  That form exists only for
block-aligned slabs inside the grid and gives no flags; the kernels also do the clipped, the unaligned and the flagged cases.
Timing of the launches: HIP events around `reps` launches captured into one graph and replayed (the wrapper's host time and the
origin upload left out), the cases alternated, `repeats` times each, in one process; medians and spreads are printed.  Bytes: four
read and four written per voxel and plane.  A slab's rows are 32-byte pieces a whole grid row apart, so neither form coalesces on
the volume side.  The whole shift is timed on the host clock around the call and a synchronisation — it reads the blocks back and
files them in the store —, alternating +8 and -8 along x on a volume whose every block holds something, beside the plain shift and
beside the plain shift followed by the torch slab copy and a `.cpu()` of the staging tensor."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralrgbd_amd import fusion, ops  # noqa: E402
from bench_shift import captured, time_ms  # noqa: E402  (tools/ is the script's directory)

DEV = "cuda:0"
N, B = 256, 8


def slab_origins():
    g = np.arange(0, N, B)
    z, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([np.zeros(z.size, np.int64), y.ravel(), z.ravel()], axis=1)


def corner_origins():
    g = np.arange(0, N, B)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    o = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    return o[(o == 0).any(axis=1)]


CORNER_SLICES = ((slice(None), slice(None), slice(0, B)), (slice(None), slice(0, B), slice(B, N)), (slice(0, B), slice(B, N), slice(B, N)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_page: no GPU (nothing is measured without one)")
    out = {"version": ops.version(), "grid": N, "cases": {}, "shift": {}}
    buf5 = torch.rand(5, N, N, N, device=DEV)
    sets = {"x slab": slab_origins(), "corner (8,8,8)": corner_origins()}
    assert len(sets["x slab"]) == 1024 and len(sets["corner (8,8,8)"]) == 32 ** 3 - 31 ** 3
    cases = {}
    for planes in (2, 5):
        buf = buf5[:planes]
        for name, origins in sets.items():
            up = ops.tsdf_block_origins(origins, DEV)
            n = len(origins)
            staged = torch.empty(n, planes, B, B, B, device=DEV)
            flags = torch.empty(n, dtype=torch.int32, device=DEV)
            slices = CORNER_SLICES[:1] if name == "x slab" else CORNER_SLICES
            stage = [torch.empty_like(buf[(slice(None),) + s]) for s in slices]
            assert sum(t.numel() for t in stage) == staged.numel()
            # the torch form against the kernel once (the same voxels), before anything is timed
            ops.tsdf_blocks_gather(buf, up, out=staged, nonempty=flags)
            for t, s in zip(stage, slices):
                t.copy_(buf[(slice(None),) + s])
            assert bool(flags.all()) and abs(float(staged.double().sum()) - sum(float(t.double().sum()) for t in stage)) < 1e-6 * staged.numel()
            nbytes = 8 * staged.numel()
            key = "%d planes %s" % (planes, name)

            def torch_gather(buf=buf, stage=stage, slices=slices):
                for t, s in zip(stage, slices):
                    t.copy_(buf[(slice(None),) + s])

            def torch_scatter(buf=buf, stage=stage, slices=slices):
                for t, s in zip(stage, slices):
                    buf[(slice(None),) + s] = t
            cases[key + " gather"] = dict(fn=lambda buf=buf, up=up, staged=staged, flags=flags: ops.tsdf_blocks_gather(buf, up, out=staged, nonempty=flags),
                                          bytes=nbytes, torch=key + " gather torch")
            cases[key + " gather torch"] = dict(fn=torch_gather, bytes=nbytes, torch=None)
            cases[key + " scatter"] = dict(fn=lambda buf=buf, up=up, staged=staged: ops.tsdf_blocks_scatter(buf, up, staged), bytes=nbytes,
                                           torch=key + " scatter torch")
            cases[key + " scatter torch"] = dict(fn=torch_scatter, bytes=nbytes, torch=None)
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
        ratio = med[k] / med[c["torch"]] if c["torch"] else 1.0
        out["cases"][k] = dict(median_us=1e3 * med[k], spread_us=1e3 * (max(t[k]) - min(t[k])), bytes=c["bytes"],
                               gb_per_s=c["bytes"] / med[k] / 1e6, ratio_to_torch=ratio)
        print("%-40s %8.1f us per launch (spread %.1f)   %6.1f MB   %7.1f GB/s   %.2f x the torch form"
              % (k, 1e3 * med[k], 1e3 * (max(t[k]) - min(t[k])), c["bytes"] / 1e6, c["bytes"] / med[k] / 1e6, ratio))
    del cases, buf5
    # the whole shift, with its host copy: the host clock around the call and a synchronisation
    for planes in (2, 5):
        vol = fusion.TSDFVolume((N, N, N), 0.01, (0.0, 0.0, 0.0), device=DEV, color=planes == 5)
        store = fusion.BlockStore(planes)
        stage = torch.empty(planes, N, N, B, device=DEV)

        def paged(s):
            vol._buf.add_(1.0)                                      # every block holds something, the one that just entered too
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vol.shift(s, store=store)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def plain(s, host):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vol.shift(s)
            if host:                                                # the leaving slab of the old buffer, by a slice copy, to the host
                stage.copy_(vol._spare[:, :, :, :B] if s[0] > 0 else vol._spare[:, :, :, N - B:])
                stage.cpu()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        runs = {"shift(store=)": [], "shift()": [], "shift() + torch slab + .cpu()": []}
        for i in range(a.warmup + a.repeats):
            for s in ((B, 0, 0), (-B, 0, 0)):
                got = (paged(s), plain(s, False), plain(tuple(-v for v in s), False), plain(s, True), plain(tuple(-v for v in s), True))
                if i >= a.warmup:
                    runs["shift(store=)"].append(got[0])
                    runs["shift()"] += [got[1], got[2]]
                    runs["shift() + torch slab + .cpu()"] += [got[3], got[4]]
        for k, v in runs.items():
            out["shift"]["%d planes %s" % (planes, k)] = dict(median_ms=1e3 * float(np.median(v)), spread_ms=1e3 * (max(v) - min(v)))
            print("%d planes %-32s %8.2f ms per call (spread %.2f)" % (planes, k, 1e3 * float(np.median(v)), 1e3 * (max(v) - min(v))))
        print("%d planes: the store holds %d blocks, %.1f MB; paged out %d, in %d" % (planes, len(store), store.nbytes / 1e6, store.n_put, store.n_taken))
        del vol, store, stage
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
