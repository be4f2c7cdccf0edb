#!/usr/bin/env python
"""Backward of the fused cost volume: HIP-event timing, by default at the training grid (64x96, D = 64, V = 4, C = 67).
--deterministic     the bit-reproducible path (csrc/costvol_bwd_det.hip) instead of the atomic kernels
--shape H W D       another grid (e.g. 192 256 64: beyond the LDS budget, the atomic side runs its global-atomic kernel)
--dev loads libnrgbd_hip_dev.so, which honours NRGBD_BWD_ABL (1 = no atomics, 2 = no tap loads; results invalid)."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--dev" in sys.argv:
    from neuralrgbd_amd import _lib
    _lib.LIB_PATH = _lib.LIB_PATH.replace("libnrgbd_hip.so", "libnrgbd_hip_dev.so")
from neuralrgbd_amd import camera, ops, synth
from neuralrgbd_amd import homography as H
h, w, D, V, C = 64, 96, 64, 4, 67
if "--shape" in sys.argv:
    h, w, D = (int(x) for x in sys.argv[sys.argv.index("--shape") + 1:sys.argv.index("--shape") + 4])
det = "--deterministic" in sys.argv
dev = "cuda:0"
cam = camera.scannet_intrinsics(w, h)
rng = np.random.RandomState(0)
feats = torch.from_numpy(rng.standard_normal((V + 1, 64, h, w)).astype(np.float32)).to(dev)
frames = torch.from_numpy(rng.standard_normal((V + 1, 3, 4 * h, 4 * w)).astype(np.float32)).to(dev)
poses = torch.from_numpy(synth.random_poses(rng, V)).to(dev)
K, rays = H._cam_dev(cam, torch.device(dev))
d_dev = H._d_candi_dev(np.linspace(0.1, 5.0, D), torch.device(dev))
KR, Kt = H.homography_terms(K, poses[:, :3, :3], poses[:, :3, 3])
cx, cy = cam["intrinsic_M"][0, 2], cam["intrinsic_M"][1, 2]
tex = ops.pack_nhwc(feats, frames)
g = torch.from_numpy(rng.standard_normal((D, h, w)).astype(np.float32)).to(dev)
fn = lambda: ops.costvol_bwd(tex[V], tex[:V], KR, Kt, rays, d_dev, cx, cy, 10.0, C, g, deterministic=det)
for _ in range(3):          # steady state: clocks up, the allocator holds the workspace block
    fn()
torch.cuda.synchronize()
times = []
for _ in range(5):          # 5 timed groups of 10 launches: the median group, and the spread
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fn()
    e1.record(); torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) / 10)
times.sort()
print("costvol_bwd %dx%dx%d V=%d C=%d %s abl=%s: %.3f ms (median of 5 groups of 10; min %.3f max %.3f)"
      % (h, w, D, V, C, "deterministic" if det else "atomic", os.environ.get("NRGBD_BWD_ABL", "0"), times[2], times[0], times[4]))
