"""Keyframe-map benchmark: the fused launch (nrgbd_dpv_keyframe_maps) beside the composition it replaces, on the same GPU in
the same process: nrgbd_dpv_resample_to + 4 x nrgbd_depth_regress + ATen exp / pow (the LBA driver's
test_KVNet_LBA.py:414-423, :455, :495 on this path's own operators), at 256 x 384 and 768 x 1024, D = 64.

    python tools/bench_keyframe.py [--sizes S,B] [--reps 50] [--warmup 10] [--repeats 3] [--json out.json]
    python tools/bench_keyframe.py --trace-only        # a few calls for `rocprofv3 --kernel-trace --stats -- python ...`

Timing: HIP events around `reps` back-to-back calls after `warmup` untimed ones, per call; `repeats` such measurements give the
run-to-run spread (max - min).  Both forms are timed with and without the reference pair (the driver needs it only in a first
window).  Bytes: the fused form must read the volume once per pair it produces (2 D hw floats with the reference pair) and
writes four maps; the composition reads D hw and writes D hw for the resample and reads D hw four times: 7 D hw floats."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralrgbd_amd import camera, homography, lba_step, ops, synth  # noqa: E402

SIZES = {"S": (256, 384), "B": (768, 1024)}
D = 64
DEV = "cuda:0"
HBM_TBS = 8.0


def workload(H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    bv = torch.log_softmax(4.0 * torch.randn(D, H, W, generator=g), 0).to(DEV)[None]
    T = np.eye(4)
    T[:3, :3] = synth.rotvec_to_R([0.01, -0.02, 0.005])
    T[:3, 3] = [0.03, -0.02, 0.05]
    return bv, torch.from_numpy(T.astype(np.float32)).to(DEV), camera.scannet_intrinsics(W, H), np.linspace(0.5, 5.0, D)


def fused(w, want_ref):
    bv, pose, cam, d_candi = w
    return lba_step.keyframe_maps(bv, pose, cam, d_candi, want_ref=want_ref)


def composition(w, want_ref):
    bv, pose, cam, d_candi = w
    d_dev = homography._d_candi_dev(d_candi, DEV)
    res = homography.resample_vol_cuda(bv, ops.pose_inverse(pose), cam_intrinsic=cam, d_candi=d_candi, d_candi_new=d_candi,
                                       padding_value=math.log(1. / D), clamp=(-1000., 0.))
    dmap_kf = ops.depth_regress(res, d_dev, want_conf=False)[0]
    conf_kf = torch.exp(ops.depth_regress(res, d_dev)[1]) ** 2
    if not want_ref:
        return None, None, dmap_kf, conf_kf
    dmap_ref = ops.depth_regress(bv[0], d_dev, want_conf=False)[0]
    conf_ref = torch.exp(ops.depth_regress(bv[0], d_dev)[1]) ** 2
    return dmap_ref, conf_ref, dmap_kf, conf_kf


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="S,B")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    out = {"version": ops.version(), "D": D}
    for tag in a.sizes.split(","):
        H, W = SIZES[tag]
        w = workload(H, W)
        if a.trace_only:
            for _ in range(5):
                fused(w, True); fused(w, False); composition(w, True); composition(w, False)
            torch.cuda.synchronize()
            continue
        f, c = fused(w, True), composition(w, True)
        # the depth maps are the same bits; the composition's confidences come from ATen's exp (a 1-ulp function), the fused
        # ones from the path's correctly rounded exponential (tests/test_gpu_keyframe.py holds them against export_depth_u16)
        same = torch.equal(f[0], c[0]) and torch.equal(f[2], c[2])
        rec = {"H": H, "W": W, "depth_maps_bit_identical": same}
        vol = D * H * W * 4
        for want_ref, name in ((True, "with_ref"), (False, "kf_only")):
            tf = [time_ms(lambda: fused(w, want_ref), a.reps, a.warmup) for _ in range(a.repeats)]
            tc = [time_ms(lambda: composition(w, want_ref), a.reps, a.warmup) for _ in range(a.repeats)]
            must = (2 if want_ref else 1) * vol
            rec[name] = {"fused_ms": tf, "composition_ms": tc, "fused_median_ms": float(np.median(tf)),
                         "composition_median_ms": float(np.median(tc)), "fused_spread_ms": max(tf) - min(tf),
                         "composition_spread_ms": max(tc) - min(tc), "ratio": float(np.median(tc) / np.median(tf)),
                         "fused_bytes": must, "composition_bytes": (7 if want_ref else 4) * vol,
                         "fused_hbm_fraction": must / (float(np.median(tf)) * 1e-3) / (HBM_TBS * 1e12)}
            r = rec[name]
            print("%s %dx%d %-8s fused %.4f ms (spread %.4f)  composition %.4f ms (spread %.4f)  x%.2f  fused = %.3f of %g TB/s  depth bits %s"
                  % (tag, H, W, name, r["fused_median_ms"], r["fused_spread_ms"], r["composition_median_ms"],
                     r["composition_spread_ms"], r["ratio"], r["fused_hbm_fraction"], HBM_TBS, "equal" if same else "DIFFER"))
        out[tag] = rec
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
