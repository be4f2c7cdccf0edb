"""The LBA inference step on the GPU (neuralrgbd_amd/lba_step.py): the keyframe maps and lba_update against the unmodified
reference's recorded step (tests/golden/lba_step.npz), the no-optimisation branch, convergence on the rendered window, and
LBADepthStream against the hand-written sequence test_step.test -> keyframe_maps -> opt_pose.* -> trajectory update."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import lba_step_inputs as li
from conftest import GOLDEN
import neuralrgbd_amd
from neuralrgbd_amd import camera, homography, lba_step, misc, ops, opt_pose, synth, test_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POSE_GATE = 1e-4          # the gate of tests/test_gpu_lba_opt.py::test_public_forms_vs_reference_golden, unchanged


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "lba_step.npz")))


@pytest.fixture(scope="module")
def scene():
    return li.scene()


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def test_maps_vs_reference_golden(golden, scene):
    """|dmap - ref| <= (D + 3) 2^-24 sum_k p_k d_k and |conf - ref| <= 4 2^-24 conf against a float64 recomputation on the
    RECORDED resampled volume (1 ulp per expf, half an ulp per multiply and per add; half an ulp for exp_rn doubled by the
    square, the square's own rounding, one unit of slack); the reference's own fp32 maps with 1 ulp more for its ATen exp.
    This path's resampled volume is compared with the recording first: a difference there would add a propagated term."""
    D = li.D
    u = 2.0 ** -24
    pose_next = torch.from_numpy(golden["pose_next"])
    got = lba_step.keyframe_maps(scene["BV"].to(DEV), pose_next, li.cams()[2], li.D_CANDI)
    got = [g.cpu().numpy().astype(np.float64) for g in got]
    # the volume this path would have resampled, with the REFERENCE's inverse so that only the resampling is compared
    res = homography.resample_vol_cuda(scene["BV"].to(DEV), torch.from_numpy(golden["pose_next_inv"]), cam_intrinsic=li.cams()[2],
                                       d_candi=li.D_CANDI, d_candi_new=li.D_CANDI, padding_value=np.log(1. / D),
                                       clamp=(-1000., 0.)).cpu().numpy()
    d_res = np.abs(res.astype(np.float64) - golden["resampled"]).max()
    inv_own = ops.pose_inverse(pose_next.to(DEV)).cpu().numpy()
    d_inv = np.abs(inv_own - golden["pose_next_inv"]).max()
    print("[lba-step] resampled volume vs reference: max|d| %.3e; inverse pose max|d| %.3e" % (d_res, d_inv))
    d = li.D_CANDI.astype(np.float32).astype(np.float64).reshape(-1, 1, 1)
    for tag, vol, dmap, conf in (("ref", scene["BV"][0].numpy(), got[0], got[1]), ("kf", golden["resampled"], got[2], got[3])):
        v = vol.astype(np.float64)
        want_d = (np.exp(v) * d).sum(0)
        want_c = np.exp(v.max(0)) ** 2
        bound_d = (D + 3) * u * want_d
        bound_c = 4 * u * want_c
        if tag == "kf":
            # propagated term of a resampled volume that differs from the recording (own inverse / own sampling): d exp = exp dv
            dv = np.abs(homography.resample_vol_cuda(
                scene["BV"].to(DEV), torch.from_numpy(inv_own), cam_intrinsic=li.cams()[2], d_candi=li.D_CANDI,
                d_candi_new=li.D_CANDI, padding_value=np.log(1. / D), clamp=(-1000., 0.)).cpu().numpy().astype(np.float64) - v)
            bound_d = bound_d + (np.exp(v) * np.expm1(dv) * d).sum(0)
            bound_c = bound_c + want_c * np.expm1(2 * dv.max(0))
        e_d, e_c = np.abs(dmap - want_d), np.abs(conf - want_c)
        print("[lba-step] %s maps vs float64: depth max err/bound %.3f  conf %.3f" % (tag, (e_d / bound_d).max(), (e_c / bound_c).max()))
        assert (e_d <= bound_d).all() and (e_c <= bound_c).all()
        # the reference's own fp32 maps: its expf / ATen exp granted 1 ulp more on its side
        r_d, r_c = golden["dmap_" + tag].astype(np.float64), golden["conf_" + tag].astype(np.float64)
        assert (np.abs(dmap - r_d) <= 2 * bound_d).all()
        assert (np.abs(conf - r_c) <= bound_c + 4 * u * want_c).all()


def _update(scene, max_iter, first=True):
    traj = [t.copy() for t in scene["traj"]]
    out = _quiet(lba_step.lba_update, traj, li.REF, scene["BV"].to(DEV), scene["frames"], li.cams(), li.D_CANDI, li.T_WIN_R,
                 li.STEP, max_iter, li.LBA_STEP, [1, 1], first)
    return traj, out


def test_lba_update_vs_reference_golden(golden, scene):
    """Poses and trajectory after the step against the reference's recording, at the gate of the existing reference comparison
    (tests/test_gpu_lba_opt.py).  The recording holds the reference's difference from ITSELF on this step (1 / 8 threads, oneDNN
    on / off); were it above half the gate, the gate would be twice that figure."""
    self_noise = max(float(golden["self_pose"]), float(golden["self_traj"]))
    gate = POSE_GATE if self_noise <= POSE_GATE / 2 else 2 * self_noise
    traj, (rel_pose_opt, srcs_idx) = _update(scene, li.MAX_ITER)
    assert list(srcs_idx) == golden["par_idx"].tolist()
    e_P = np.abs(np.stack([p.numpy() for p in rel_pose_opt]) - golden["par_poses"]).max()
    e_T = np.abs(np.stack(traj) - golden["traj_after_par"]).max()
    print("[lba-step] lba_update vs reference: |pose| %.2e  |traj| %.2e  (gate %.1e, reference self-noise %.1e)" % (e_P, e_T, gate, self_noise))
    assert e_P <= gate and e_T <= gate
    assert all(t.dtype == np.float64 and t.shape == (4, 4) for t in traj)
    # the first-window stage alone: stop before the joint stage by comparing its trajectory entries that the joint stage
    # does not rewrite (frame 0 is outside the next reference's window)
    assert np.abs(traj[0] - golden["traj_after_direct"][0]).max() <= gate


def test_lba_max_iter_1_is_the_drivers_no_optimisation_branch(scene):
    """LBA_max_iter <= 1 (test_KVNet_LBA.py:441-446, :468-475): ground-truth poses around the NEXT reference go through
    local_BA_direct with step 0 (a unit-quaternion round trip) and are applied to traj[ref_indx] in order, then the ground-truth
    poses of the next window are applied to traj[ref_indx + 1]: all host arithmetic, reproduced here operation for operation."""
    traj, (rel_pose_opt, srcs_idx) = _update(scene, 1)
    want = [t.copy() for t in scene["traj"]]
    nxt = li.REF + 1
    inits, idx = misc.get_twin_rel_pose(want, nxt, li.T_WIN_R * li.STEP, 1, use_gt_R=True, use_gt_t=True, dataset=scene["frames"])
    for k, i in enumerate(idx):
        P = torch.eye(4)
        P[:3, 3] = inits[k][:3, 3]
        P[:3, :3] = misc.UnitQ2Rotation(misc.Rotation2UnitQ(inits[k][:3, :3]))
        want[i] = np.matmul(P.numpy(), want[li.REF])
    poses, idx2 = misc.get_twin_rel_pose(want, nxt, li.T_WIN_R, li.STEP, use_gt_R=True, use_gt_t=True, dataset=scene["frames"])
    for k, i in enumerate(idx2):
        want[i] = np.matmul(poses[k].numpy(), want[nxt])
    assert list(srcs_idx) == list(idx2)
    assert all(torch.equal(a, b) for a, b in zip(rel_pose_opt, poses))
    for i in range(li.N_FRAMES):
        assert np.array_equal(traj[i], want[i]), i


def test_every_source_pose_of_the_first_window_improves(scene):
    """Perturbed initial poses + the peaked DPV: after the first-window optimisation every source pose is closer to the truth in
    translation and in rotation.  tests/test_lba_step_host.py shows the float64 restatement satisfies this for the seed."""
    traj = [t.copy() for t in scene["traj"]]
    idx = lba_step.window_indices(li.REF, li.T_WIN_R, li.STEP)
    e0 = li.rel_errors(traj, scene["true"], li.REF, idx)
    dmap_ref, conf_ref, _, _ = lba_step.keyframe_maps(
        scene["BV"].to(DEV), torch.FloatTensor(homography.get_rel_extrinsicM(traj[li.REF], traj[li.REF + 1])), li.cams()[2], li.D_CANDI)
    inits, idx_all = misc.get_twin_rel_pose(traj, li.REF, li.T_WIN_R * li.STEP, 1, dataset=scene["frames"])
    assert idx_all == idx
    poses = _quiet(opt_pose.local_BA_direct, scene["frames"][li.REF]["img"], [scene["frames"][i]["img"] for i in idx],
                   dmap_ref[None, None], conf_ref[None, None], li.cams(), li.DW_SCALES, inits, li.MAX_ITER, li.LBA_STEP, [1, 1])
    for k, i in enumerate(idx):
        traj[i] = np.matmul(poses[k].numpy(), traj[li.REF])
    e1 = li.rel_errors(traj, scene["true"], li.REF, idx)
    print("[lba-step] first window (t, rad): %s -> %s" % (e0, e1))
    for a, b in zip(e0, e1):
        assert b[0] < a[0] and b[1] < a[1]


# ---- the stream ---------------------------------------------------------------------------------------------------------
SH, SW, SD = 256, 384, 16
S_ITER, S_STEP = 3, 0.005
N_STREAM = 9


@pytest.fixture(scope="module")
def stream_setup():
    cams = [camera.scannet_intrinsics(SW // k, SH // k) for k in (4, 2, 1)]
    d_candi = np.linspace(0.5, 5.0, SD)
    model = neuralrgbd_amd.KVNET(64, cams[0], d_candi, 10.0, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=2)
    model.load_state_dict(synth.seeded_state_dict(model, 0))
    model = model.to(DEV)
    g = torch.Generator().manual_seed(77)
    frames = [{"img": torch.randn(1, 3, SH, SW, generator=g)} for _ in range(N_STREAM)]
    traj, _, _ = li.index_traj(N_STREAM, seed=9)
    return model, cams, d_candi, frames, traj


def _stream(setup, traj=None, **kw):
    model, cams, d_candi, frames, traj0 = setup
    return lba_step.LBADepthStream(model, cams, d_candi, 2, 1, traj0 if traj is None else traj, LBA_max_iter=S_ITER,
                                   LBA_step=S_STEP, opt_vars=[1, 1], **kw)


def _by_hand(setup, ref_indxs):
    """The driver's sequence written out on the public operators, with its own state."""
    model, cams, d_candi, frames, traj0 = setup
    traj = lba_step.copy_list(traj0)
    bv, first, outs = None, True, []
    for ref in ref_indxs:
        src_idx = [ref - 2, ref - 1, ref + 1, ref + 2]
        if bv is None:
            t_norms = lba_step.get_t_norms(traj, 1)
            lba_step.rescale_traj_t(traj, d_candi.max() / (cams[0]['focal_length'] * np.array(t_norms).mean() / 2))
        poses = torch.cat([torch.from_numpy(homography.get_rel_extrinsicM(traj[ref], traj[i]).astype(np.float32)).cuda().unsqueeze(0)
                           for i in src_idx], dim=0).unsqueeze(0)
        pose_next = torch.FloatTensor(homography.get_rel_extrinsicM(traj[ref], traj[ref + 1])).cuda()
        BV, bv = test_step.test(model, d_candi, [cams[0]], 2, [frames[ref]], [[frames[i] for i in src_idx]], poses, bv,
                                cam_pose_next=pose_next, R_net=True)
        dmap_ref, conf_ref, dmap_kf, conf_kf = lba_step.keyframe_maps(BV, pose_next, cams[2], d_candi, want_ref=first)
        if first:
            first = False
            inits, idx = misc.get_twin_rel_pose(traj, ref, 2, 1, dataset=frames)
            P = opt_pose.local_BA_direct(frames[ref]['img'], [frames[i]['img'] for i in idx], dmap_ref[None, None],
                                         conf_ref[None, None], cams, [4, 2, 1], inits, S_ITER, S_STEP, [1, 1])
            for k, i in enumerate(idx):
                traj[i] = np.matmul(P[k].numpy(), traj[ref])
        inits, idx = misc.get_twin_rel_pose(traj, ref + 1, 2, 1, dataset=frames)
        P = opt_pose.local_BA_direct_parallel(frames[ref + 1]['img'], [frames[i]['img'] for i in idx], dmap_kf[None, None],
                                              conf_kf[None, None], cams, [4, 2, 1], inits, S_ITER, S_STEP, [1, 1])
        for k, i in enumerate(idx):
            traj[i] = np.matmul(P[k].numpy(), traj[ref + 1])
        outs.append((BV.clone(), P, idx, bv.clone(), lba_step.copy_list(traj)))
    return outs


def test_stream_equals_the_hand_written_sequence_bit_for_bit(stream_setup):
    refs = [2, 3, 4]
    want = _quiet(_by_hand, stream_setup, refs)
    s = _stream(stream_setup)
    for ref, (BV, P, idx, bv, traj) in zip(refs, want):
        got_BV, got_P, got_idx = _quiet(s.step, ref, stream_setup[3])
        assert torch.equal(got_BV, BV) and got_BV.shape == (1, SD, SH, SW)
        assert list(got_idx) == list(idx) and all(torch.equal(a, b) for a, b in zip(got_P, P))
        assert torch.equal(s.bv_predict, bv)
        assert all(np.array_equal(a, b) for a, b in zip(s.traj_extMs, traj))
    assert s.first_frame is False and s.frame_cnt == 3
    # the caller's trajectory is not touched
    assert all(np.array_equal(a, b) for a, b in zip(stream_setup[4], li.index_traj(N_STREAM, seed=9)[0]))


def test_refresh_and_invalid_pose_reset_the_state(stream_setup):
    frames = stream_setup[3]
    # refresh (:329-334): at a frame divisible by refresh_frames the filter restarts from the initial trajectory, so the step
    # equals the first step of a fresh stream
    s = _stream(stream_setup, refresh_frames=3)
    _quiet(s.step, 2, frames)
    assert s.bv_predict is not None and s.first_frame is False
    got = _quiet(s.step, 3, frames)
    fresh = _stream(stream_setup)
    want = _quiet(fresh.step, 3, frames)
    assert torch.equal(got[0], want[0]) and all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
    assert all(np.array_equal(a, b) for a, b in zip(s.traj_extMs, fresh.traj_extMs))
    # a window with an invalid pose (:515-516): nothing is computed, the filter state is dropped, the trajectory is kept
    s = _stream(stream_setup)
    _quiet(s.step, 2, frames)
    _quiet(s.step, 3, frames)
    s.traj_extMs[6] = np.eye(4)                    # "the tracker did not return" for a frame of the next window
    before = lba_step.copy_list(s.traj_extMs)
    assert s.bv_predict is not None
    assert _quiet(s.step, 4, frames) == (None, None, None)
    assert s.bv_predict is None and all(np.array_equal(a, b) for a, b in zip(s.traj_extMs, before))
    # an invalid pose in the very first window: the stream stays unstarted
    traj = lba_step.copy_list(stream_setup[4])
    traj[4] = np.eye(4)
    s = _stream(stream_setup, traj=traj)
    assert _quiet(s.step, 2, frames) == (None, None, None) and s.bv_predict is None and s.first_frame is True
