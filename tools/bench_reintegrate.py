"""Re-integration after a pose correction, measured: TSDFVolume.reintegrate (one launch: a frame out at its old pose and in at the new
one) beside the pair it replaces, deintegrate + integrate (two launches), and beside one integrate alone, on a 256^3 volume and the
config-B frame (a 768 x 1024 depth map and its picture), colourless and coloured.

    python tools/bench_reintegrate.py [--reps 100] [--warmup 10] [--repeats 5] [--json out.json]
    python tools/bench_reintegrate.py --lib PATH      # `integrate` alone with another build of the library (the parent's, which has
                                                      # no reintegrate entry): a process of its own, to set beside the numbers above

Scene: tools/bench_tsdf.py's (the plane of tests/tsdf_ref.py seen from six poses near the origin, a 2.56 m cube, trunc = 3 voxels), all
six views fused; the moved frame is view 3, between its pose and one 2 cm / 0.01 rad off — a small correction, whose two frustum
boxes nearly coincide — and, as the other extreme, one 0.6 m off.  Every call moves the frame the other way (a -> b, b -> a, ...), so
the volume always holds the frame where the next call removes it.  Timing: HIP events around `reps` back-to-back calls after `warmup`
untimed ones, per call; the three forms alternate, `repeats` times each, in one process; medians and spreads are printed with the
ratio reintegrate / pair.  Bytes: a lane group that either pose touches is read and written once by the fused launch and twice by the
pair (16 B per voxel and direction without colour, 40 B with it); the chain runs twice in both."""
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

from neuralrgbd_amd import _lib, camera, fusion, ops, synth  # noqa: E402

DEV = "cuda:0"
N = 256
SIZE = (768, 1024)
DEPTH_RANGE = (0.3, 3.0)
AFFINE = ((0.229, 0.224, 0.225), (0.485, 0.456, 0.406))
MOVES = {"small": (0.01, 0.02), "large": (0.05, 0.6)}              # (rotation sigma rad, translation sigma m) of the correction


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


def scene(color):
    import tsdf_ref as ref
    H, W = SIZE
    K = fusion.intrinsics_at(camera.scannet_intrinsics(W, H), H, W)
    pr = np.random.RandomState(7)
    poses = [synth.random_pose(pr, 0.08, 0.15) for _ in range(6)]
    depths = [torch.from_numpy(ref.plane_depth(m, K, H, W)).to(DEV) for m in poses]
    image = torch.from_numpy(np.random.RandomState(8).rand(3, H, W).astype(np.float32)).to(DEV)
    vol = fusion.TSDFVolume((N, N, N), 2.56 / N, (-1.28, -1.28, 0.6), device=DEV, color=color)
    kw = dict(depth_range=DEPTH_RANGE, color=image, color_affine=AFFINE) if color else dict(depth_range=DEPTH_RANGE)
    for m, d in zip(poses, depths):
        vol.integrate(d, m, K, **kw)
    return vol, depths[3], poses[3], K, kw


def forms(color, move):
    """{name: call}: every call of `reintegrate` and of `pair` moves view 3 to the pose it is not at."""
    vol, depth, a, K, kw = scene(color)
    rot, trans = MOVES[move]
    b = synth.random_pose(np.random.RandomState(9), rot, trans) @ a
    at = {"reintegrate": 0, "pair": 0}
    ends = (a, b)

    def reintegrate():
        i = at["reintegrate"]
        vol.reintegrate(depth, ends[i], ends[1 - i], K, **kw)
        at["reintegrate"] = 1 - i

    def pair():
        i = at["pair"]
        vol.deintegrate(depth, ends[i], K, **kw)
        vol.integrate(depth, ends[1 - i], K, **kw)
        at["pair"] = 1 - i
    boxes = [fusion.frustum_box(m, K, SIZE, DEPTH_RANGE[1] + vol.trunc, vol) for m in ends]
    info = {"voxels_observed": int((vol.weight > 0).sum()), "boxes": boxes}
    return {"reintegrate": reintegrate, "pair": pair, "integrate": lambda: vol.integrate(depth, a, K, **kw)}, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reintegrate: no GPU (nothing is measured without one)")
    if a.reps % 2 or a.warmup % 2:
        raise SystemExit("bench_reintegrate: --reps and --warmup are even (every second call moves the frame back)")
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)                       # before the first call loads it
        _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if "reintegrate" not in k}
    out = {"version": ops.version(), "grid": N, "size": SIZE, "lib": _lib.LIB_PATH}
    for color in (False, True):
        for move in MOVES:
            fs, info = forms(color, move)
            if a.lib:
                if move != "small":
                    continue
                fs = {"integrate": fs["integrate"]}
            name = "%s_%s" % ("coloured" if color else "colourless", move)
            t = {k: [] for k in fs}
            for _ in range(a.repeats):                              # alternating: what else runs on the host touches all alike
                for k, fn in fs.items():
                    t[k].append(time_ms(fn, a.reps, a.warmup))
            med = {k: float(np.median(v)) for k, v in t.items()}
            out[name] = dict(info, ms=t, median_ms=med, spread_ms={k: max(v) - min(v) for k, v in t.items()})
            print("%-18s boxes %s %s" % (name, info["boxes"][0], info["boxes"][1]))
            line = "   " + "   ".join("%s %.4f ms (spread %.4f)" % (k, med[k], max(t[k]) - min(t[k])) for k in fs)
            if "pair" in med:
                out[name]["ratio"] = med["reintegrate"] / med["pair"]
                line += "   reintegrate / pair %.2f" % out[name]["ratio"]
            print(line)
            del fs
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
