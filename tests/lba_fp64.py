"""Inputs and a float64 restatement of the local bundle adjustment (ICP/opt_pose_numerical.py) for the LBA tests.

`inputs(seed)` rebuilds the scene the golden fixture tests/golden/lba_opt_small.npz was recorded on (tools/gen_lba_opt_golden.py):
a rendered window (synth.rendered_window) at 64 x 96 with 4 sources, a confidence map, and initial poses perturbed from the true
ones.  `run` is the optimiser restated in torch float64 on the CPU with autograd: the same pyramid, unit-quaternion chain
(s = 1/|q|^2 on the diagonal only), warp (K (R X + t), division by z, grid_sample zeros padding, align_corners False), mask,
confidence-weighted L1 mean and torch.optim.Adam, so the fp32 paths can be held against it.
"""
import numpy as np
import torch
import torch.nn.functional as F

from neuralrgbd_amd import camera, synth

H, W, V = 64, 96, 4
DW_SCALES = [4, 2, 1]
SEED = 22
MAX_ITER = 4
STEP = 0.01
OPT_VARS = ([1, 1], [1, 0], [0, 1])

# tests/golden/lba_opt_wide.npz: (a) local_BA_direct with the LBA driver's window (t_win 2 x dat_indx_step 5 on each side: 20
# sources) at its img_size 384 x 256; (b) local_BA_direct_parallel with 16 sources (every block of 4 of the update's reduction)
WIDE_H, WIDE_W, WIDE_V, WIDE_SEED = 256, 384, 20, 31
WIDE_OPT_VARS = ([1, 1], [0, 1])
PAR16_H, PAR16_W, PAR16_V, PAR16_SEED = 32, 48, 16, 41
DRIVER_D = 64


def cams(H_, W_, dw_scales=DW_SCALES):
    return [camera.scannet_intrinsics(W_ // k, H_ // k) for k in dw_scales]


def inputs(seed=SEED, H_=H, W_=W, V_=V, rot_sigma=0.01, trans_sigma=0.02, conf_kind="sigmoid"):
    """(ref_frame [1,3,H,W], src_frames [V x [1,3,H,W]], dmap_ref [1,1,H,W], conf_map_ref [1,1,H,W], rel_pose_inits [V,4,4]
    float32, true poses [V,4,4] float32) — all CPU.  conf_kind "sigmoid": a smooth map in (0, 1); "driver": built as
    test_KVNet_LBA.py builds it, exp(max over the depth candidates of the log-probability) ** 2, from a 64-candidate
    log_softmax of smooth logits — values in [1/64^2, 1] (down to 1.2e-2 on the recorded 20-view window)."""
    cam = camera.scannet_intrinsics(W_, H_)
    ref, src, poses, depth = synth.rendered_window(seed, H_, W_, cam, V=V_)
    rng = np.random.RandomState(seed + 1000)
    if conf_kind == "driver":
        logits = torch.from_numpy(4.0 * synth.smooth_texture(rng, DRIVER_D, H_, W_, octaves=2).astype(np.float32))
        conf = (torch.exp(F.log_softmax(logits, 0).max(0)[0]) ** 2).numpy()[None]
    else:
        conf = 1.0 / (1.0 + np.exp(-synth.smooth_texture(rng, 1, H_, W_, octaves=2)))      # in (0, 1), like a DPV confidence
    pert = synth.random_poses(rng, V_, rot_sigma, trans_sigma).astype(np.float64)
    true = poses[0].numpy().astype(np.float64)
    inits = np.stack([pert[v] @ true[v] for v in range(V_)]).astype(np.float32)
    return (ref.float(), [src[0, v:v + 1].float() for v in range(V_)], torch.from_numpy(depth)[None, None],
            torch.from_numpy(conf.astype(np.float32))[None], torch.from_numpy(inits), poses[0].float())


def uq_to_R(uq):
    """quaternion2Rotation(unitQ_to_quat(uq)) as differentiable float64 expressions."""
    ux, uy, uz = uq[0], uq[1], uq[2]
    a = ux ** 2 + uy ** 2 + uz ** 2
    w, x, y, z = 2 * ux / (a + 1), 2 * uy / (a + 1), 2 * uz / (a + 1), (1 - a) / (1 + a)
    s = 1 / (w ** 2 + x ** 2 + y ** 2 + z ** 2)
    return torch.stack([
        torch.stack([1 - 2 * s * (y ** 2 + z ** 2), 2 * (x * y - w * z), 2 * (x * z + w * y)]),
        torch.stack([2 * (x * y + w * z), 1 - 2 * s * (x ** 2 + z ** 2), 2 * (y * z - w * x)]),
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * s * (x ** 2 + y ** 2)])])


def warp(src, dmap, R, t, K, rays):
    """back_warp_th_Rt_msrc in float64: src [N,3,h,w], dmap [h,w], R [N,3,3], t [N,3], K [3,3], rays [3,hw]."""
    N, _, h, w = src.shape
    X = dmap.reshape(1, -1) * rays
    coords = []
    for n in range(N):
        P = K @ (R[n] @ X + t[n].reshape(3, 1))
        u, v = P[0] / P[2], P[1] / P[2]
        coords.append(torch.stack(((u - K[0, 2]) / K[0, 2], (v - K[1, 2]) / K[1, 2]), -1).reshape(h, w, 2))
    return F.grid_sample(src, torch.stack(coords), mode="bilinear", padding_mode="zeros", align_corners=False)


def level_inputs(ref_frame, src_frames, dmap_ref, conf_map_ref, cams_intrin, dw_scales=DW_SCALES):
    """Per scale (ref [1,3,h,w], src [N,3,h,w], dmap [h,w], conf [h,w], K, rays) in float64, pooled from full resolution."""
    def pool(x, k):
        return x if k <= 1 else F.avg_pool2d(x, k)
    srcs = torch.cat(src_frames, 0).double()
    out = []
    for k, cam in zip(dw_scales, cams_intrin):
        out.append((pool(ref_frame.double(), k), pool(srcs, k), pool(dmap_ref.double(), k)[0, 0],
                    pool(conf_map_ref.double(), k)[0, 0], cam["intrinsic_M_cuda"].double(), cam["unit_ray_array_2D"].double()))
    return out


def loss_and_grad(level, R_or_uq, t, joint=True, param="R"):
    """Loss (nn.L1Loss mean; per view when not joint) and its gradient w.r.t. (R or uq, t) at fixed poses, float64."""
    ref, src, dmap, conf, K, rays = level
    P = R_or_uq.detach().double().clone().requires_grad_(True)
    tt = t.detach().double().clone().requires_grad_(True)
    R = torch.stack([uq_to_R(P[n]) for n in range(P.shape[0])]) if param == "uq" else P
    wp = warp(src, dmap, R, tt, K, rays)
    m = (wp != 0).double()
    c = conf.expand_as(wp)
    d = (wp * m * c - ref * m * c).abs()
    losses = d.mean(dim=(1, 2, 3))
    L = d.mean() if joint else losses.sum()
    L.backward()
    return (float(L) if joint else losses.detach().numpy()), P.grad.numpy(), tt.grad.numpy()


def run(levels, uq0, t0, max_iter, LR, opt_vars, joint):
    """The optimiser in float64 from fp32 initial parameters uq0 [N,3], t0 [N,3]: returns dict of per-iteration losses
    [iters, 1 or N], g_t / g_uq [iters, N, 3], final t / uq [N,3]."""
    opt_R = opt_vars[0] == 1
    opt_t = (not opt_R) or opt_vars[1] == 1
    N = uq0.shape[0]
    uq = torch.as_tensor(uq0).double().clone().requires_grad_(True)
    t = torch.as_tensor(t0).double().clone().requires_grad_(True)
    groups = ([uq] if opt_R else []) + ([t] if opt_t else [])
    opts = [torch.optim.Adam(groups, lr=LR, betas=(.9, .999))] if joint else \
        [torch.optim.Adam(([uq] if opt_R else []) + ([t] if opt_t else []), lr=LR, betas=(.9, .999))]
    losses, gts, guqs = [], [], []
    for iscale, (ref, src, dmap, conf, K, rays) in enumerate(levels):
        for o in opts:
            for g in o.param_groups:
                g['lr'] = LR / (2 ** iscale) if iscale > 0 else LR
        for it in range(max_iter):
            for o in opts:
                o.zero_grad()
            R = torch.stack([uq_to_R(uq[n]) for n in range(N)])
            wp = warp(src, dmap, R, t, K, rays)
            m = (wp != 0).double().detach()
            c = conf.expand_as(wp)
            d = (wp * m * c - ref * m * c).abs()
            if joint:
                L = d.mean()
                losses.append([float(L)])
            else:
                per = d.mean(dim=(1, 2, 3))      # N independent optimisations: per-view means, gradients do not mix
                L = per.sum()
                losses.append(per.detach().numpy().tolist())
            L.backward()
            gts.append(t.grad.detach().numpy().copy())
            guqs.append(uq.grad.detach().numpy().copy())
            if not opt_R:
                uq.grad = None
            if not opt_t:
                t.grad = None
            for o in opts:
                o.step()
    return {"loss": np.asarray(losses), "g_t": np.asarray(gts), "g_uq": np.asarray(guqs),
            "t": t.detach().numpy(), "uq": uq.detach().numpy()}


def pose_error(poses, true):
    """(max translation error, max rotation angle in rad) over the views."""
    et, er = 0.0, 0.0
    for P, T in zip(poses, true):
        P = np.asarray(P, np.float64); T = np.asarray(T, np.float64)
        et = max(et, float(np.linalg.norm(P[:3, 3] - T[:3, 3])))
        c = (np.trace(P[:3, :3].T @ T[:3, :3]) - 1) / 2
        er = max(er, float(np.arccos(np.clip(c, -1, 1))))
    return et, er


def uq_to_pose(uq, t):
    out = []
    for n in range(uq.shape[0]):
        P = np.eye(4)
        P[:3, :3] = uq_to_R(torch.as_tensor(uq[n]).double()).numpy()
        P[:3, 3] = t[n]
        out.append(P)
    return out
