"""Small helpers of the depth path (the used part of code/mutils/misc.py)."""
import math

import numpy as np
import torch

from . import homography as _homo
from . import ops


def valid_dpv(dpv_in):
    """True unless the volume is None or flagged invalid by a NaN at its first element
    (mutils/misc.py:100-115; the NaN convention comes from mdataloader/batch_loader.py:30-43).
    Reads one element back to the host, exactly like the reference."""
    if dpv_in is None:
        return False
    assert isinstance(dpv_in, torch.Tensor), 'input should a Tensor'
    if not 2 <= dpv_in.dim() <= 5:
        raise Exception('wrong dimension for input dpv !')
    ok = not bool(torch.isnan(dpv_in[(0,) * dpv_in.dim()]))
    if dpv_in.is_cuda:
        # the path's own failure report rides on this synchronisation: a BatchNorm whose batch statistics collapsed in the frame
        # that produced dpv_in raises here (nets.check_status) instead of passing on a wrong volume
        from .nets import check_status
        check_status(dpv_in.device)
    return ok


def depth_val_regression(BV_measure, d_candi_cur, BV_log=True, out=None):
    """Expected depth sum_d p_d * d of a [1,D,h,w] volume -> [1,h,w] (mutils/misc.py:532-548).
    One kernel instead of a Python loop over D.  `out` (extension): a contiguous fp32 [1,h,w] tensor to write the map into."""
    assert len(d_candi_cur) == BV_measure.shape[1], \
        'BV_measure should have the same # of slices as len(d_candi_cur) !'
    d_dev = _homo._d_candi_dev(d_candi_cur, BV_measure.device)
    logp = BV_measure[0] if BV_log else torch.log(BV_measure[0])
    # the refined volume is an NCHW view of channels-last memory (DPVUpsampleNet.forward_log, autograd.LogSoftmaxCL): read it there
    depth, _ = ops.depth_regress(logp, d_dev, want_conf=False, channels_last=ops.is_channels_last_view(logp),
                                 out=None if out is None else out.view(logp.shape[1:]))
    return depth.unsqueeze(0)


def d_candi_up4(d_candi):
    """The candidates of an up-sampled refined volume (KVNET(if_upsample_d=True): [1, 4D, H, W]): np.linspace(d_min, d_max, 4 D), as
    every data loader of the reference defines them next to `dmap_up4_imgsize_digit` (mdataloader/scanNet.py:327,419,
    kitti.py:273,378, dl_7scenes.py:250,346).  Pass them to depth_val_regression / export_res_img with such a volume."""
    d_candi = np.asarray(d_candi)
    return np.linspace(d_candi.min(), d_candi.max(), 4 * len(d_candi))


def dpv_confidence(BV_measure):
    """max_d log-prob -> [1,h,w] (test_utils/export_res.py:58-59)."""
    d_dev = torch.zeros(BV_measure.shape[1], dtype=torch.float32, device=BV_measure.device)
    _, conf = ops.depth_regress(BV_measure[0], d_dev, want_conf=True, channels_last=ops.is_channels_last_view(BV_measure[0]))
    return conf.unsqueeze(0)


def split_frame_list(frame_list, t_win_r):
    """ref = frame_list[t_win_r], src = the others in order (mutils/misc.py:509-517)."""
    ref = frame_list[t_win_r]
    src = [f for i, f in enumerate(frame_list) if i != t_win_r]
    return ref, src


def get_entries_list_dict(list_dict, keyname):
    return [d[keyname] for d in list_dict]


# ---- the pose helpers of the local bundle adjustment (opt_pose.py).  Host-side, fp32, operation for operation the reference's
# torch code, so the bits agree; only downsample_img runs on the device.

def downsample_img(img, kernel_size=4):
    """F.avg_pool2d(img, kernel_size) of an NCHW CUDA tensor (mutils/misc.py:139-144): nrgbd_lba_pyramid with one level."""
    if kernel_size <= 1:
        return img
    N, C, H, W = img.shape
    x = ops._need(img, "img").reshape(N * C, H, W)
    (out,) = ops.lba_pyramid([x[i] for i in range(N * C)], [kernel_size])
    return out.view(N, C, H // kernel_size, W // kernel_size)


def quaternion2Rotation(q, R_tensor=None):
    """TUM-format quaternion [x y z w] tensor -> 3x3 (mutils/misc.py:295-331, is_tensor=True): s = 1/|q|^2 on the diagonal only."""
    Rot = torch.zeros(3, 3) if R_tensor is None else R_tensor
    w, x, y, z = q[3], q[0], q[1], q[2]
    s = 1 / (w**2 + x**2 + y**2 + z**2)
    Rot[0, 0] = 1 - 2 * s * (y**2 + z**2)
    Rot[1, 1] = 1 - 2 * s * (x**2 + z**2)
    Rot[2, 2] = 1 - 2 * s * (x**2 + y**2)
    Rot[0, 1] = 2 * (x*y - w * z)
    Rot[1, 0] = 2 * (x*y + w * z)
    Rot[0, 2] = 2 * (x*z + w * y)
    Rot[2, 0] = 2 * (x*z - w * y)
    Rot[1, 2] = 2 * (y*z - w * x)
    Rot[2, 1] = 2 * (y*z + w * x)
    return Rot


def Rotation2Quaternion(R, quat):
    """mutils/misc.py:365-402, branches as written (the last three divide by quat[0] whatever they computed)."""
    assert quat.dim() == 1 and len(quat) == 4, 'quat should be of right shape !'
    if R[0, 0] + R[1, 1] + R[2, 2] + 1 > 0:
        quat[3] = .5 * math.sqrt(R[0, 0] + R[1, 1] + R[2, 2] + 1)
        s = 1 / 4 / quat[3]
        quat[0] = s * (R[2, 1] - R[1, 2])
        quat[1] = s * (R[0, 2] - R[2, 0])
        quat[2] = s * (R[1, 0] - R[0, 1])
    elif R[0, 0] - R[1, 1] - R[2, 2] + 1 > 0:
        quat[0] = .5 * math.sqrt(R[0, 0] - R[1, 1] - R[2, 2] + 1)
        s = 1 / 4 / quat[0]
        quat[1] = s * (R[1, 0] + R[0, 1])
        quat[2] = s * (R[0, 2] + R[2, 0])
        quat[3] = s * (R[2, 1] + R[1, 2])
    elif R[1, 1] - R[0, 0] - R[2, 2] + 1 > 0:
        quat[1] = .5 * math.sqrt(R[1, 1] - R[0, 0] - R[2, 2] + 1)
        s = 1 / 4 / quat[0]
        quat[0] = s * (R[1, 0] + R[0, 1])
        quat[2] = s * (R[1, 2] + R[2, 1])
        quat[3] = s * (R[0, 2] - R[2, 0])
    elif R[2, 2] - R[0, 0] - R[1, 1] + 1 > 0:
        quat[2] = .5 * math.sqrt(R[2, 2] - R[0, 0] - R[1, 1] + 1)
        s = 1 / 4 / quat[0]
        quat[0] = s * (R[2, 0] + R[0, 2])
        quat[1] = s * (R[2, 1] + R[1, 2])
        quat[3] = s * (R[1, 0] - R[0, 1])


def unitQ_to_quat(unitQ, quat):
    """3-vector unit-quaternion parameter -> TUM quaternion (mutils/misc.py:459-472): the parameter's x goes into w."""
    x, y, z = unitQ[0], unitQ[1], unitQ[2]
    alpha2 = x**2 + y**2 + z**2
    quat[3] = 2 * x / (alpha2 + 1)
    quat[0] = 2 * y / (alpha2 + 1)
    quat[1] = 2 * z / (alpha2 + 1)
    quat[2] = (1 - alpha2) / (1 + alpha2)


def quat_to_unitQ(quat, unitQ):
    """mutils/misc.py:487-502."""
    q1, q2, q3, q0 = quat[0], quat[1], quat[2], quat[3]
    alpha2 = (1 - q3) / (1 + q3)
    unitQ[0] = q0 * (alpha2 + 1) * .5
    unitQ[1] = q1 * (alpha2 + 1) * .5
    unitQ[2] = q2 * (alpha2 + 1) * .5


def UnitQ2Rotation(r_uq):
    """uq [3] -> R [3,3] on the host in fp32 (mutils/misc.py:404-409)."""
    assert isinstance(r_uq, torch.Tensor)
    r_q = torch.zeros(4)
    unitQ_to_quat(r_uq.detach().cpu(), r_q)
    return quaternion2Rotation(r_q)


def Rotation2UnitQ(R):
    """R [3,3] -> uq [3] on the host in fp32 (mutils/misc.py:411-416)."""
    R = torch.as_tensor(R, dtype=torch.float32).cpu()
    r_q = torch.zeros(4)
    r_uq = torch.zeros(3)
    Rotation2Quaternion(R, r_q)
    quat_to_unitQ(r_q, r_uq)
    return r_uq


def get_twin_rel_pose(traj_extMs, ref_indx, t_win_r, dat_indx_step, use_gt_R=False, use_gt_t=False, dataset=None,
                      add_noise_gt=False, noise_sigmas=None, traj_extMs_dso=None, use_dso_R=False, use_dso_t=False,
                      opt_next_frame=False):
    """Initial relative poses (reference -> source, 4x4 CPU float32 tensors) of the source frames of the local time window
    around ref_indx, and the trajectory indices they will be written back to (mutils/misc.py:21-98; same signature and
    returns).  The LAST frame of the window has no pose of its own yet: it starts from its neighbour's, index
    ref_indx + t_win_r * dat_indx_step - 1, while the returned index list names the frame itself.  opt_next_frame adds
    ref_indx + 1 after the past frames.  traj_extMs_dso (+ use_dso_R / use_dso_t) overrides the last pose's rotation /
    translation with the tracker's own motion ref -> last; use_gt_R / use_gt_t override every pose from dataset[i]['extM']
    (optionally with Gaussian noise of noise_sigmas = (sigma_R, sigma_t))."""
    if use_dso_R or use_dso_t:
        assert traj_extMs_dso is not None
    span = t_win_r * dat_indx_step
    past = list(range(ref_indx - span, ref_indx, dat_indx_step))
    nxt = [ref_indx + 1] if opt_next_frame else []
    last = ref_indx + span
    src_frame_idx = past + nxt + list(range(ref_indx + dat_indx_step, last - dat_indx_step + 1, dat_indx_step)) + [last - 1]
    src_frame_idx_opt = past + nxt + list(range(ref_indx + dat_indx_step, last + 1, dat_indx_step))

    ref_cam_extM = traj_extMs[ref_indx]
    src_cam_poses = [torch.from_numpy(_homo.get_rel_extrinsicM(ref_cam_extM, traj_extMs[i]).astype(np.float32))
                     for i in src_frame_idx]

    if traj_extMs_dso is not None:
        dRt = torch.FloatTensor(_homo.get_rel_extrinsicM(traj_extMs_dso[ref_indx].copy(), traj_extMs_dso[last].copy()))
        if use_dso_R:
            src_cam_poses[-1][:3, :3] = dRt[:3, :3]
        if use_dso_t:
            src_cam_poses[-1][:3, 3] = dRt[:3, 3]

    if use_gt_R or use_gt_t:
        for idx, srcidx in enumerate(src_frame_idx_opt):
            pose_gt = torch.from_numpy(_homo.get_rel_extrinsicM(dataset[ref_indx]['extM'], dataset[srcidx]['extM']))
            R_gt, t_gt = pose_gt[:3, :3], pose_gt[:3, 3]
            if use_gt_R:
                if add_noise_gt:
                    R_gt += torch.randn(R_gt.shape).type_as(R_gt) * noise_sigmas[0]
                src_cam_poses[idx][:3, :3] = R_gt
            if use_gt_t:
                if add_noise_gt:
                    t_gt += torch.randn(t_gt.shape).type_as(t_gt) * noise_sigmas[1]
                src_cam_poses[idx][:3, 3] = t_gt
    return src_cam_poses, src_frame_idx_opt
