#!/usr/bin/env python
"""SHA-256 digests of the outputs of the cost-volume forward, for a before/after comparison of two libraries on one device (one
process per library): cost and logp of the generations "quad", "lds" and "gather" (all three deterministic: no atomics), L2 and L1,
both align_corners values.  Inputs as tests/test_gpu_ops.py::test_costvol_quad_vs_oracle builds them, plus the three ray tables of
test_costvol_quad_non_affine_ray_tables_vs_oracle (the quad kernel's escape re-evaluation).
--lib PATH          another libnrgbd_hip.so (e.g. one built from the parent commit)"""
import hashlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from neuralrgbd_amd import _lib
if "--lib" in sys.argv:
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
from neuralrgbd_amd import camera, ops, synth
from oracle import cpu_oracle as co
CASES = [  # h, w, D, V, C, rot, trans, seed, rays
    (192, 256, 64, 4, 67, 0.02, 0.05, 12, "pinhole"),    # fused softmax, scrambled XCD bands
    (120, 160, 128, 4, 67, 0.02, 0.05, 16, "pinhole"),   # 300 tiles x 4 chunks: the (tile, chunk)-list branch
    (64, 96, 64, 4, 67, 0.02, 0.05, 11, "pinhole"),      # config S
    (33, 70, 64, 5, 67, 0.02, 0.05, 13, "pinhole"),      # grid of 180: the plain branch, ragged tiles
    (192, 256, 33, 1, 67, 0.02, 0.05, 22, "pinhole"),    # second pass of one candidate
    (24, 40, 16, 8, 64, 0.02, 0.05, 17, "pinhole"),      # no RGB word
    (24, 40, 16, 3, 65, 0.02, 0.05, 18, "pinhole"),      # run-time tail
    (48, 64, 32, 4, 67, 0.0, 0.3, 20, "pinhole"),        # pure 0.3 m translation: unstaged groups, clamped patches
    (96, 128, 64, 3, 67, None, None, 77, "unit_norm"), (96, 128, 64, 3, 67, None, None, 77, "barrel"), (96, 128, 64, 3, 67, None, None, 77, "wavy")]
sha = lambda a: hashlib.sha256(a.cpu().numpy().tobytes()).hexdigest()[:32]
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def ray_table(cam, h, w, kind):
    rays = cam["unit_ray_array_2D"].numpy()
    if kind == "pinhole":
        return rays
    rays = rays.astype(np.float64).reshape(3, h, w)
    if kind == "unit_norm":
        rays = rays / np.linalg.norm(rays, axis=0, keepdims=True)
    elif kind == "barrel":
        r2 = rays[0] ** 2 + rays[1] ** 2
        rays = np.stack([rays[0] * (1 + 0.25 * r2), rays[1] * (1 + 0.25 * r2), rays[2]])
    else:
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        step = rays[0, 0, 1] - rays[0, 0, 0]
        rays = np.stack([rays[0] + 2.5 * step * np.sin(xs * 1.1 + ys * 0.7), rays[1] + 2.5 * step * np.cos(xs * 0.9 - ys * 1.3), rays[2]])
    return rays.reshape(3, h * w).astype(np.float32)


print("library %s" % _lib.LIB_PATH)
for h, w, D, V, C, rot, trans, seed, kind in CASES:
    cam = camera.scannet_intrinsics(w, h)
    rng = np.random.RandomState(seed)
    feat_ref = rng.standard_normal((C, h, w)).astype(np.float32)
    feat_src = rng.standard_normal((V, C, h, w)).astype(np.float32)
    poses = synth.random_poses(rng, V, rot_sigma=rot, trans_sigma=trans) if kind == "pinhole" else synth.random_poses(rng, V)
    KR, Kt = co.homography_terms(cam["intrinsic_M_cuda"].numpy(), poses[:, :3, :3], poses[:, :3, 3])
    cx, cy = cam["intrinsic_M"][0, 2], cam["intrinsic_M"][1, 2]
    tex = ops.pack_nhwc(dev(np.concatenate([feat_src, feat_ref[None]], 0)))
    args = (tex[V], tex[:V], dev(KR), dev(Kt), dev(ray_table(cam, h, w, kind)), dev(np.linspace(0.1, 5, D)), cx, cy, 10.0, C)
    name = "%dx%dx%d V%d C%d %s" % (h, w, D, V, C, kind)
    for gen in ("quad", "lds", "gather"):
        for dist in ("L2", "L1"):
            for align in (False, True):
                cost, logp = ops.costvol(*args, dist=dist, align_corners=align, want_cost=True, want_logp=True, generation=gen)
                torch.cuda.synchronize()
                print("%-32s %-6s %s align=%d  cost %s  logp %s" % (name, gen, dist, align, sha(cost), sha(logp)))
