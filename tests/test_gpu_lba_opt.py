"""Local bundle adjustment on the GPU (lba.hip through neuralrgbd_amd/opt_pose.py): the fused loss + gradient pass against the
float64 restatement, the update kernel against torch.optim.Adam, both public forms against the unmodified reference's recorded
run (tests/golden/lba_opt_small.npz), determinism, the step-0 debug mode, the sync-free device loop and convergence."""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

import lba_fp64 as lf
from conftest import GOLDEN
from neuralrgbd_amd import camera, misc, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "lba_opt_small.npz")))


@pytest.fixture(scope="module")
def scene():
    return lf.inputs()


def _call(fn, scene, opt_vars, max_iter=lf.MAX_ITER, step=lf.STEP, dw_scales=lf.DW_SCALES):
    ref_frame, src_frames, dmap, conf, inits, _ = scene
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        poses = fn(ref_frame.to(DEV), [s.to(DEV) for s in src_frames], dmap.to(DEV), conf.to(DEV), lf.cams(lf.H, lf.W, dw_scales),
                   dw_scales, [inits[v].numpy() for v in range(lf.V)], max_iter, step, opt_vars)
    return poses, buf.getvalue().strip().split("\n")


def _d_losses(lines):
    return [(m.group(1), float(m.group(2))) for m in (re.match(r"(opt_pose\(\): scale=\d+, iter \d+/\d+), d_loss = (\S+)", s)
                                                       for s in lines)]


@pytest.mark.parametrize("H,W", [(64, 96), (480, 640)])
def test_fused_gradient_vs_fp64_at_fixed_poses(H, W):
    rng = np.random.RandomState(5)
    N = 4
    cam = camera.scannet_intrinsics(W, H)
    ref, src, poses, depth = synth.rendered_window(9, H, W, cam, V=N)
    conf = (0.2 + 0.8 * rng.rand(H, W)).astype(np.float32)
    pert = synth.random_poses(rng, N, 0.01, 0.02)
    P = np.stack([pert[v].astype(np.float64) @ poses[0, v].numpy() for v in range(N)]).astype(np.float32)
    R, t = torch.from_numpy(P[:, :3, :3].copy()), torch.from_numpy(P[:, :3, 3].copy())
    K, rays = cam["intrinsic_M_cuda"], cam["unit_ray_array_2D"]
    level64 = (ref.double(), src[0].double(), torch.from_numpy(depth).double(), torch.from_numpy(conf).double(), K.double(),
               rays.double())
    L, gR, gt = lf.loss_and_grad(level64, R, t, joint=True, param="R")
    state = torch.zeros((N, ops.LBA_STATE))
    state[:, 3:6] = t
    state[:, 6:15] = R.reshape(N, 9)
    partial = torch.empty(N * ops.lba_workgroups(H, W) * 13, device=DEV)
    ops.lba_grad(ref[0].to(DEV), src[0].contiguous().to(DEV), torch.from_numpy(depth).to(DEV), torch.from_numpy(conf).to(DEV),
                 K.to(DEV), rays.to(DEV), state.to(DEV), partial)
    s = partial[:N * ops.lba_workgroups(H, W) * 13].view(N, -1, 13).double().sum(1).cpu().numpy() / (N * 3.0 * H * W)
    e_L = abs(s[:, 12].sum() - L) / L
    e_R = np.abs(s[:, :9].reshape(N, 3, 3) - gR).max() / np.abs(gR).max()
    e_t = np.abs(s[:, 9:12] - gt).max() / np.abs(gt).max()
    print("[parity] lba_grad %dx%d vs fp64: loss rel %.2e  g_R %.2e  g_t %.2e (of max |g|)" % (H, W, e_L, e_R, e_t))
    assert e_L < 1e-5 and e_R <= 1e-4 and e_t <= 1e-4


def test_update_kernel_vs_torch_adam_across_a_scale_change():
    """Synthetic partials -> the update kernel, against torch.optim.Adam (CPU, fp32) fed the same gradients (d/d uq through the
    reference's quaternion chain by fp32 autograd), lr halved after 3 steps as at a scale change."""
    rng = np.random.RandomState(2)
    N, H, W, nwg = 3, 8, 16, 1
    uq0 = (0.01 * rng.standard_normal((N, 3))).astype(np.float32)
    t0 = (0.1 * rng.standard_normal((N, 3))).astype(np.float32)
    state = torch.empty((N, ops.LBA_STATE), device=DEV)
    ops.lba_init(torch.from_numpy(np.concatenate([uq0, t0], 1)).to(DEV), state)
    # step 0 writes R exactly as the host mirror of UnitQ2Rotation computes it
    for n in range(N):
        assert torch.equal(state[n, 6:15].cpu().view(3, 3), misc.UnitQ2Rotation(torch.from_numpy(uq0[n])))
    uq = torch.from_numpy(uq0.copy()).requires_grad_(True)
    t = torch.from_numpy(t0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([t, uq], lr=0.01, betas=(.9, .999))
    log = torch.empty((1, 6), device=DEV)
    norm = N * 3.0 * H * W
    for step in range(1, 7):
        lr = 0.01 if step <= 3 else 0.005
        for g in opt.param_groups:
            g["lr"] = lr
        part = (rng.standard_normal((N, nwg, 13)) * 50).astype(np.float32)
        ops.lba_update(torch.from_numpy(part).to(DEV), state, log, step - 1, H, W, True, step, lr, True, True)
        G = torch.from_numpy(part.sum(1).astype(np.float64) / norm)
        opt.zero_grad()
        R = torch.stack([_uq_to_R_f32(uq[n]) for n in range(N)])
        (R * G[:, :9].float().view(N, 3, 3)).sum().backward()
        t.grad = G[:, 9:12].float().clone()
        opt.step()
        assert abs(float(log[0, step - 1]) - float(part[:, :, 12].astype(np.float64).sum() / norm)) <= 1e-6 * abs(float(log[0, step - 1]))
    got = state.cpu()
    e_uq = (got[:, 0:3] - uq.detach()).abs().max().item()
    e_t = (got[:, 3:6] - t.detach()).abs().max().item()
    print("[parity] lba_update vs torch.optim.Adam: |uq| %.2e  |t| %.2e" % (e_uq, e_t))
    assert e_uq <= 1e-6 and e_t <= 1e-6
    for n in range(N):
        assert torch.equal(got[n, 6:15].view(3, 3), misc.UnitQ2Rotation(got[n, 0:3]))


def _uq_to_R_f32(uq):
    """The reference's UnitQ2Rotation as differentiable fp32 torch ops (the autograd path of opt_pose_numerical.py:250)."""
    q = torch.zeros(4)
    misc.unitQ_to_quat(uq, q)
    return misc.quaternion2Rotation(q)


@pytest.mark.parametrize("form", ["parallel", "single"])
@pytest.mark.parametrize("ov", lf.OPT_VARS, ids=lambda v: "%d%d" % tuple(v))
def test_public_forms_vs_reference_golden(golden, scene, form, ov):
    from neuralrgbd_amd import opt_pose
    tag = "%s_%d%d" % (form, ov[0], ov[1])
    joint = form == "parallel"
    ref_frame, src_frames, dmap, conf, inits, _ = scene
    levels, init = opt_pose._prepare(ref_frame, src_frames, dmap, conf, lf.cams(lf.H, lf.W), lf.DW_SCALES,
                                     [inits[v].numpy() for v in range(lf.V)])
    opt_R, opt_t = opt_pose._flags(ov, False, conf, 'unit_quat', lf.MAX_ITER)
    state, log = opt_pose._run(levels, init, lf.MAX_ITER, lf.STEP, opt_R, opt_t, joint)
    st, lg = state.cpu().numpy(), log.cpu().numpy().T
    want_loss = golden[tag + "_loss"]
    e_loss = (np.abs(lg - want_loss) / np.abs(want_loss)).max()
    e_t = np.abs(st[:, 3:6] - golden[tag + "_t"]).max()
    e_uq = np.abs(st[:, 0:3] - golden[tag + "_uq"]).max()
    fn = opt_pose.local_BA_direct_parallel if joint else opt_pose.local_BA_direct
    poses, lines = _call(fn, scene, ov)
    e_P = np.abs(np.stack([p.numpy() for p in poses]) - golden[tag + "_poses"]).max()
    got_d, want_d = _d_losses(lines), _d_losses(list(golden[tag + "_prints"]))
    e_d = max(abs(a[1] - b[1]) for a, b in zip(got_d, want_d))
    print("[parity] LBA %s GPU vs reference: loss rel %.2e  |t| %.2e  |uq| %.2e  |pose| %.2e  d_loss %.1e" % (tag, e_loss, e_t, e_uq, e_P, e_d))
    assert e_loss <= 1e-4 and e_t <= 1e-4 and e_uq <= 1e-4 and e_P <= 1e-4
    assert [a[0] for a in got_d] == [b[0] for b in want_d] and len(got_d) == len(want_d) == len(lines)
    assert e_d <= 2e-3     # d_loss = 100 x a difference of two losses, each within 1e-4 relative (losses ~0.1)
    assert all(isinstance(p, torch.Tensor) and p.device.type == "cpu" and p.dtype == torch.float32 and p.shape == (4, 4)
               for p in poses)


def test_private_forms_return_values(golden, scene):
    from neuralrgbd_amd import opt_pose
    ref_frame, src_frames, dmap, conf, inits, _ = scene
    lv = lf.level_inputs(ref_frame, src_frames, dmap, conf, lf.cams(lf.H, lf.W))
    imgs_ref = [x[0].float() for x in lv]
    with contextlib.redirect_stdout(io.StringIO()):
        t, uq, warps, ref_img = opt_pose._opt_pose_warping_parallel(
            imgs_ref, [x[2].float() for x in lv], [x[1].float() for x in lv], torch.from_numpy(golden["uq0"]),
            inits[:, :3, 3].clone(), lf.cams(lf.H, lf.W), max_iter=lf.MAX_ITER, LR=lf.STEP, opt_vars=[1, 1],
            conf_maps_ref=[x[3].float() for x in lv])
    assert warps == [] and ref_img.shape == (lf.H, lf.W, 3)
    assert np.abs(ref_img - golden["ref_img"]).max() < 1e-6
    assert np.abs(t.cpu().numpy() - golden["parallel_11_t"]).max() <= 1e-4
    assert np.abs(uq.cpu().numpy() - golden["parallel_11_uq"]).max() <= 1e-4
    R0 = torch.from_numpy(golden["uq0"][1])
    with contextlib.redirect_stdout(io.StringIO()):
        t1, r1, _, _ = opt_pose._opt_pose_warping(imgs_ref, [x[2].float() for x in lv], [x[1][1:2].float() for x in lv], R0,
                                                  inits[1, :3, 3].clone(), lf.cams(lf.H, lf.W), max_iter=lf.MAX_ITER,
                                                  LR=lf.STEP, opt_vars=[0, 1], conf_maps_ref=[x[3].float() for x in lv])
    assert r1 is R0 and np.abs(t1.cpu().numpy() - golden["single_01_t"][1]).max() <= 1e-4


def test_two_runs_are_bitwise_identical(scene):
    from neuralrgbd_amd import opt_pose
    a, _ = _call(opt_pose.local_BA_direct_parallel, scene, [1, 1], max_iter=6)
    b, _ = _call(opt_pose.local_BA_direct_parallel, scene, [1, 1], max_iter=6)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_step_zero_returns_the_initial_pose_round_trip(scene):
    from neuralrgbd_amd import opt_pose
    _, _, _, _, inits, _ = scene
    poses, lines = _call(opt_pose.local_BA_direct_parallel, scene, [1, 1], max_iter=1, step=0)
    for v in range(lf.V):
        uq = misc.Rotation2UnitQ(inits[v, :3, :3])
        assert torch.equal(poses[v][:3, :3], misc.UnitQ2Rotation(uq))
        assert torch.equal(poses[v][:3, 3], inits[v, :3, 3])
    assert all(s.endswith("d_loss = 0.000000") for s in lines) and len(lines) == 3


def test_device_loop_does_not_synchronize(scene):
    from neuralrgbd_amd import opt_pose
    ref_frame, src_frames, dmap, conf, inits, _ = scene
    levels, init = opt_pose._prepare(ref_frame, src_frames, dmap, conf, lf.cams(lf.H, lf.W), lf.DW_SCALES,
                                     [inits[v].numpy() for v in range(lf.V)])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        state, log = opt_pose._run(levels, init, 20, 0.01, True, True, joint=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(state).all() and torch.isfinite(log).all()


def test_converges_on_the_rendered_scene(scene):
    from neuralrgbd_amd import opt_pose
    _, _, _, _, inits, true = scene
    poses, _ = _call(opt_pose.local_BA_direct_parallel, scene, [1, 1], max_iter=20, step=0.01)
    e0 = lf.pose_error(inits.numpy(), true.numpy())
    e1 = lf.pose_error([p.numpy() for p in poses], true.numpy())
    print("[lba] GPU rendered scene: pose error (t, rad) %.4f %.4f -> %.4f %.4f" % (e0[0], e0[1], e1[0], e1[1]))
    assert e1[0] < e0[0] and e1[1] < e0[1]
