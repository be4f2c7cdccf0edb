"""TSDF mesh extraction benchmark: the device work of TSDFVolume.mesh (ops.tsdf_extract_mesh, four launches) beside that of
TSDFVolume.points (ops.tsdf_extract_points, three launches) on the same volume, at the volumes of tools/bench_tsdf.py: the plane scene
integrated into 128^3 and 256^3 voxels from a 768 x 1024 depth map.

    python tools/bench_mesh.py [--reps 50] [--warmup 5] [--repeats 3] [--json out.json]
    python tools/bench_mesh.py --trace-only --grid 256 --form mesh      # 50 calls for `rocprofv3 --kernel-trace --stats -- python ...`

Timing: HIP events around `reps` back-to-back calls into preallocated outputs after `warmup` untimed ones, per call; no read-back, no
allocation inside the window.  Both the count-only call (capacity 0: what mesh() / points() run first) and the writing call are timed;
"mesh()" and "points()" are their sums, the device work of one call of either method.  Effective rate: 8 bytes per voxel (tsdf and
weight, read once) over the time of ONE pass, although the count pass and the writing passes each stream the volume; a 128^3 volume
(16.8 MB) and a 256^3 one (134 MB) fit the 256 MB last-level cache between back-to-back calls."""
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

from neuralrgbd_amd import ops  # noqa: E402
import bench_tsdf  # noqa: E402

DEV = bench_tsdf.DEV
SIZE = "768x1024"
TRACE_CALLS = 50


def setup(n):
    fs, vol = bench_tsdf.forms(n, SIZE)[:2]
    for _ in range(6):
        fs["hip"]()
    args = (vol.tsdf, vol.weight, vol.origin, vol.voxel_size, 1.0)
    X, Y, Z = vol.dims
    p_ws = torch.empty(ops.tsdf_extract_workspace(X, Y, Z) // 8, dtype=torch.int64, device=DEV)
    m_ws = torch.empty(ops.tsdf_mesh_workspace(X, Y, Z) // 8 + 1, dtype=torch.int64, device=DEV)
    p_counts, m_counts = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    ops.tsdf_extract_mesh(*args, m_ws, None, None, m_counts)
    nv, _, nf, _ = (int(v) for v in m_counts.cpu())
    pts = torch.empty((nv, 3), device=DEV)
    vertices, faces = torch.empty((nv, 3), device=DEV), torch.empty((nf, 3), dtype=torch.int32, device=DEV)
    forms = {"points_count": lambda: ops.tsdf_extract_points(*args, p_ws, None, p_counts),
             "points_write": lambda: ops.tsdf_extract_points(*args, p_ws, pts, p_counts),
             "mesh_count": lambda: ops.tsdf_extract_mesh(*args, m_ws, None, None, m_counts),
             "mesh_write": lambda: ops.tsdf_extract_mesh(*args, m_ws, vertices, faces, m_counts)}
    for f in forms.values():
        f()
    torch.cuda.synchronize()
    assert int(p_counts[0]) == nv and torch.equal(pts.view(torch.int32), vertices.view(torch.int32))      # the same vertices
    assert nf > 0 and int(faces.max()) < nv and int(faces.min()) >= 0
    return forms, nv, nf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--grid", type=int, choices=bench_tsdf.GRIDS, default=256)
    ap.add_argument("--form", choices=("points", "mesh"), default="mesh")
    a = ap.parse_args()
    if a.trace_only:
        forms = setup(a.grid)[0]
        for _ in range(TRACE_CALLS):
            forms[a.form + "_count"]()
            forms[a.form + "_write"]()
        torch.cuda.synchronize()
        return 0
    out = {"version": ops.version()}
    for n in bench_tsdf.GRIDS:
        forms, nv, nf = setup(n)
        res = {"vertices": nv, "triangles": nf}
        for name, fn in forms.items():
            t = [bench_tsdf.time_ms(fn, a.reps, a.warmup) for _ in range(a.repeats)]
            res[name] = {"ms": t, "median_ms": float(np.median(t)), "spread_ms": max(t) - min(t)}
        for what in ("points", "mesh"):
            res[what] = res[what + "_count"]["median_ms"] + res[what + "_write"]["median_ms"]
        res["ratio"] = res["mesh"] / res["points"]
        gb = 8 * n ** 3 / 1e9
        print("%d^3: %d vertices, %d triangles" % (n, nv, nf))
        for name in forms:
            print("    %-13s %.4f ms per call (spread %.4f)" % (name, res[name]["median_ms"], res[name]["spread_ms"]))
        print("    points() %.4f ms, mesh() %.4f ms: ratio %.2f; %.1f MB per pass: %.0f GB/s (points) and %.0f GB/s (mesh) as one pass"
              % (res["points"], res["mesh"], res["ratio"], 1e3 * gb, gb / (res["points"] * 1e-3), gb / (res["mesh"] * 1e-3)))
        out[str(n)] = res
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
