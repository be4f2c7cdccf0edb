"""Colour in the TSDF volume, measured: the coloured launches beside the colourless ones on the same 256^3 volume and the config-B frame
(a 768 x 1024 depth map and the 768 x 1024 picture it came from) — integrate (with the frustum box and over the whole grid),
points() / mesh() and the ray cast.

    python tools/bench_tsdf_color.py [--reps 100] [--warmup 10] [--repeats 5] [--json out.json]
    python tools/bench_tsdf_color.py --trace-only --form integrate|integrate_color|raycast|raycast_color
                  # 50 calls of one form for `rocprofv3 --kernel-trace --stats -- python ...` (tools/bench_tsdf.py --stats reads the csv)

Scene: tools/bench_tsdf.py's (the plane of tests/tsdf_ref.py from a pose near the origin, a 2.56 m cube, trunc = 3 voxels); the picture
is seeded noise in [0, 1), so neighbouring voxels gather unrelated pixels.  Timing: HIP events around `reps` back-to-back calls after
`warmup` untimed ones, per call; the two forms of a pair alternate, `repeats` times each, in one process, and the median and the
spread of either are printed with the ratio of the medians.  Bytes: an updated group of four voxels moves 16 B per voxel without
colour (tsdf and weight, read and written) and 40 B with it (three more planes), plus the gathered pixels: 2.5 x by bytes alone.  The
256^3 volume (134 MB without colour, 336 MB with it) no longer fits the 256 MB last-level cache once it carries colour."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from neuralrgbd_amd import camera, fusion, ops, synth  # noqa: E402

DEV = "cuda:0"
N = 256
SIZE = (768, 1024)
DEPTH_RANGE = (0.3, 3.0)
TRACE_CALLS = 50
AFFINE = ((0.229, 0.224, 0.225), (0.485, 0.456, 0.406))


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


def scene():
    import tsdf_ref as ref
    H, W = SIZE
    K = fusion.intrinsics_at(camera.scannet_intrinsics(W, H), H, W)
    extM = synth.random_pose(np.random.RandomState(7), 0.08, 0.15)
    depth = torch.from_numpy(ref.plane_depth(extM, K, H, W)).to(DEV)
    image = torch.from_numpy(np.random.RandomState(8).rand(3, H, W).astype(np.float32)).to(DEV)
    plain = fusion.TSDFVolume((N, N, N), 2.56 / N, (-1.28, -1.28, 0.6), device=DEV)
    coloured = fusion.TSDFVolume((N, N, N), 2.56 / N, (-1.28, -1.28, 0.6), device=DEV, color=True)
    return plain, coloured, depth, image, extM, K


def pairs():
    """{name: (colourless call, coloured call)} on two volumes that hold the same six observations."""
    plain, coloured, depth, image, extM, K = scene()
    integrate = lambda cull: (lambda: plain.integrate(depth, extM, K, depth_range=DEPTH_RANGE, cull=cull),
                              lambda: coloured.integrate(depth, extM, K, depth_range=DEPTH_RANGE, cull=cull, color=image, color_affine=AFFINE))
    for _ in range(6):
        for f in integrate(True):
            f()
    torch.cuda.synchronize()
    assert torch.equal(plain.tsdf.view(torch.int32), coloured.tsdf.view(torch.int32)) and torch.equal(plain.weight, coloured.weight)
    pts, found = plain.points()
    (v, f, _), out = plain.mesh(), {}
    outs = (torch.empty(SIZE, device=DEV), torch.empty((3,) + SIZE, device=DEV), torch.empty((3,) + SIZE, device=DEV))
    out["integrate_cull"] = integrate(True)
    out["integrate_whole_grid"] = integrate(False)
    out["points"] = (lambda: plain.points(capacity=found), lambda: coloured.points(capacity=found, colors=True))
    out["mesh"] = (lambda: plain.mesh(capacity=(len(v), len(f))), lambda: coloured.mesh(capacity=(len(v), len(f)), colors=True))
    out["raycast_normals"] = (lambda: plain.raycast(extM, K, SIZE, DEPTH_RANGE, normals=True, out=outs[:2]),
                              lambda: coloured.raycast(extM, K, SIZE, DEPTH_RANGE, normals=True, color=True, out=outs))
    out["raycast"] = (lambda: plain.raycast(extM, K, SIZE, DEPTH_RANGE, out=outs[0]),
                      lambda: coloured.raycast(extM, K, SIZE, DEPTH_RANGE, color=True, out=(outs[0], outs[2])))
    info = {"voxels_updated": int((plain.weight > 0).sum()), "points": found, "vertices": len(v), "triangles": len(f),
            "hits": int((plain.raycast(extM, K, SIZE, DEPTH_RANGE) != 0).sum())}
    return out, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--form", choices=("integrate", "integrate_color", "raycast", "raycast_color"), default="integrate_color")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_color: no GPU (nothing is measured without one)")
    ps, info = pairs()
    if a.trace_only:
        fn = ps["integrate_cull" if a.form.startswith("integrate") else "raycast_normals"][a.form.endswith("_color")]
        for _ in range(TRACE_CALLS + 1):
            fn()
        torch.cuda.synchronize()
        return 0
    out = {"version": ops.version(), "scene": dict(info, grid=N, size=SIZE)}
    print("256^3, %d x %d: %d voxels observed, %d points, %d triangles, %d ray hits" % (SIZE + (info["voxels_updated"], info["points"],
                                                                                         info["triangles"], info["hits"])))
    for name, (plain, coloured) in ps.items():
        reps = a.reps if name.startswith(("integrate", "raycast")) else max(a.reps // 10, 5)      # the extractions read a count back
        t = ([], [])
        for _ in range(a.repeats):                                  # alternating: what else runs on the host touches both alike
            t[0].append(time_ms(plain, reps, a.warmup))
            t[1].append(time_ms(coloured, reps, a.warmup))
        med = [float(np.median(x)) for x in t]
        out[name] = {"colourless_ms": t[0], "coloured_ms": t[1], "median_ms": med, "spread_ms": [max(x) - min(x) for x in t],
                     "ratio": med[1] / med[0]}
        print("%-22s colourless %.4f ms (spread %.4f)   coloured %.4f ms (spread %.4f)   ratio %.2f" % (
            name, med[0], max(t[0]) - min(t[0]), med[1], max(t[1]) - min(t[1]), med[1] / med[0]))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
