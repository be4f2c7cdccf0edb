"""The LBA inference step: depth from a video whose poses come from a tracker and are refined frame by frame.

The reference's second inference mode (code/test_KVNet_LBA.py:306-528) as three pieces:

  keyframe_maps   <- :408-423, :455, :495   the depth / confidence maps the pose optimiser reads, from the R-Net's log-DPV in
                                            ONE launch (ops.dpv_keyframe_maps): the image-size resampled volume is never written
  lba_update      <- :408-512               maps -> opt_pose.local_BA_direct over the whole window on a first window,
                                            opt_pose.local_BA_direct_parallel for the next reference frame -> trajectory update
  LBADepthStream  <- :306-528               the driver loop as an object: validity check, refresh rule, scale heuristic,
                                            test_step.test(R_net=True), lba_update

DSO I/O, dataset readers and file export stay with the caller: `frames` is any index-addressable sequence of dicts with
'img' [1,3,H,W] (and 'extM' 4x4 where ground truth is used), the initial trajectory a list of numpy 4x4 extrinsics from any
tracker (an identity matrix = "the tracker did not return", as DSO/dso_io.py:262-272).
"""
import math

import numpy as np
import torch

from . import homography as warp_homo
from . import misc as m_misc
from . import opt_pose
from . import ops
from . import test_step
from ._lib import NrgbdError

DW_SCALES = [4, 2, 1]


def keyframe_maps(BV_measure, pose_next, cam_intrinsic, d_candi, want_ref=True, out=None):
    """(dmap_ref, conf_ref, dmap_kf, conf_kf), each [H,W], of the log-DPV BV_measure [1,D,H,W] (or [D,H,W]).

    pose_next: the relative pose reference -> next frame (4x4); its inverse is taken on the device (ops.pose_inverse, as
    test_step.test does).  The keyframe pair is depth_val_regression / exp(max)**2 of
    resample_vol_cuda(BV_measure, inv(pose_next), cam_intrinsic, d_candi, d_candi_new=d_candi, pad).clamp(-1000, 0), the
    reference pair the same of BV_measure itself; want_ref=False skips the latter (None, or untouched in `out`)."""
    vol = BV_measure[0] if BV_measure.dim() == 4 else BV_measure
    D = vol.shape[0]
    if len(d_candi) != D:
        raise ValueError("keyframe_maps: %d candidates for a volume of %d planes" % (len(d_candi), D))
    dev = vol.device
    _, rays = warp_homo._cam_dev(cam_intrinsic, dev)
    T = ops.pose_inverse(torch.as_tensor(pose_next).to(device=dev, dtype=torch.float32).contiguous())
    z_half, z_radius = warp_homo.z_range_f64(d_candi)
    d_dev = warp_homo._d_candi_dev(d_candi, dev)
    hhfov = math.radians(cam_intrinsic['hfov']) * .5
    hvfov = math.radians(cam_intrinsic['vfov']) * .5
    return ops.dpv_keyframe_maps(vol, T, rays, d_dev, d_dev, math.tan(hhfov), math.tan(hvfov), z_half, z_radius,
                                 math.log(1. / float(D)), clamp=(-1000., 0.), want_ref=want_ref, out=out)


def _apply(traj_extMs, rel_pose_opt, srcs_idx, ref):
    """traj[src] = rel_pose_opt @ traj[ref] (:464-465, :510-511)."""
    for idx, srcidx in enumerate(srcs_idx):
        traj_extMs[srcidx] = np.matmul(rel_pose_opt[idx].cpu().numpy(), traj_extMs[ref])


def lba_update(traj_extMs, ref_indx, BVs_measure, frames, cams_intrin, d_candi, t_win_r, dat_indx_step, LBA_max_iter,
               LBA_step, opt_vars, first_frame, dw_scales=DW_SCALES, use_gt_R=False, use_dso_R=False, use_gt_t=False,
               use_dso_t=False, opt_next_frame=False, traj_extMs_dso=None):
    """The pose refinement that follows the depth network in one frame of the LBA driver (test_KVNet_LBA.py:408-512).

    traj_extMs: list of numpy 4x4 extrinsics, UPDATED IN PLACE as rel_pose_opt[i] @ traj_extMs[ref].  BVs_measure: the
    R-Net's log-DPV [1,D,H,W] of frame ref_indx.  cams_intrin: the three camera dicts of dw_scales [4, 2, 1] (quarter, half,
    image size).  first_frame: the first window after a start or a refresh — every frame of the window
    (2 t_win_r dat_indx_step of them) is optimised on its own against the reference frame's own maps (:437-465) before the
    next reference frame's window is optimised jointly against the warped maps (:476-511).  LBA_max_iter <= 1 skips the
    optimisation as the driver does: ground-truth poses (frames[i]['extM']) replace the estimates.
    Returns (rel_pose_opt, srcs_idx) of the next reference frame's window."""
    idx_ref_ = ref_indx + 1
    cam_pose_nextframe = torch.FloatTensor(warp_homo.get_rel_extrinsicM(traj_extMs[ref_indx], traj_extMs[idx_ref_]))
    dmap_ref, conf_ref, dmap_kf, conf_kf = keyframe_maps(BVs_measure, cam_pose_nextframe, cams_intrin[2], d_candi,
                                                         want_ref=bool(first_frame))
    if LBA_max_iter <= 1:
        LBA_step = 0.

    if first_frame:
        span = t_win_r * dat_indx_step
        if LBA_max_iter <= 1:
            inits_all, idx_all = m_misc.get_twin_rel_pose(traj_extMs, idx_ref_, span, 1, use_gt_R=True, use_gt_t=True,
                                                          dataset=frames, add_noise_gt=False, noise_sigmas=None)
        else:
            inits_all, idx_all = m_misc.get_twin_rel_pose(traj_extMs, ref_indx, span, 1, use_gt_R=False, use_gt_t=False,
                                                          dataset=frames)
        rel_pose_opt = opt_pose.local_BA_direct(frames[ref_indx]['img'], [frames[i]['img'] for i in idx_all],
                                                dmap_ref[None, None], conf_ref[None, None], cams_intrin, dw_scales,
                                                inits_all, max_iter=LBA_max_iter, step=LBA_step, opt_vars=opt_vars)
        _apply(traj_extMs, rel_pose_opt, idx_all, ref_indx)

    if LBA_max_iter <= 1:
        rel_pose_opt, srcs_idx = m_misc.get_twin_rel_pose(traj_extMs, idx_ref_, t_win_r, dat_indx_step, use_gt_R=True,
                                                          use_gt_t=True, dataset=frames, add_noise_gt=False,
                                                          noise_sigmas=None)
    else:
        rel_pose_inits, srcs_idx = m_misc.get_twin_rel_pose(traj_extMs, idx_ref_, t_win_r, dat_indx_step, use_gt_R=use_gt_R,
                                                            use_dso_R=use_dso_R, use_gt_t=use_gt_t, use_dso_t=use_dso_t,
                                                            dataset=frames, traj_extMs_dso=traj_extMs_dso,
                                                            opt_next_frame=opt_next_frame)
        rel_pose_opt = opt_pose.local_BA_direct_parallel(frames[idx_ref_]['img'], [frames[i]['img'] for i in srcs_idx],
                                                         dmap_kf[None, None], conf_kf[None, None], cams_intrin, dw_scales,
                                                         rel_pose_inits, max_iter=LBA_max_iter, step=LBA_step,
                                                         opt_vars=opt_vars)
    _apply(traj_extMs, rel_pose_opt, srcs_idx, idx_ref_)
    return rel_pose_opt, srcs_idx


# ---- the driver's trajectory helpers (test_KVNet_LBA.py:39-72, DSO/dso_io.py:262-281) ---------------------------------------

def valid_pose(Rt):
    """False for the identity ("the tracker did not return") and for a matrix with a NaN."""
    Rt = np.asarray(Rt)
    return not (np.abs(np.eye(4) - Rt).max() == 0 or np.any(np.isnan(Rt)))


def valid_poses(Rts, src_idxs):
    return all(valid_pose(Rts[i]) for i in src_idxs)


def get_t_norms(traj_extM, dat_indx_step):
    """Baselines |t_i - t_(i - 2 step)| over the valid poses of traj_extM[1:]."""
    valid = [ext for ext in traj_extM[1:] if valid_pose(ext)]
    return np.array([np.linalg.norm(valid[i][:3, 3] - valid[i - 2 * dat_indx_step][:3, 3])
                     for i in range(2 * dat_indx_step, len(valid))])


def rescale_traj_t(traj_M, scale):
    for trajm in traj_M:
        trajm[:3, 3] *= scale


def copy_list(list_in):
    return [ele.clone() if isinstance(ele, torch.Tensor) else ele.copy() for ele in list_in]


def window_indices(ref_indx, t_win_r, dat_indx_step):
    """Source frame indices of the depth window around ref_indx (:313-316)."""
    return list(range(ref_indx - t_win_r * dat_indx_step, ref_indx, dat_indx_step)) + \
        list(range(ref_indx + dat_indx_step, ref_indx + t_win_r * dat_indx_step + 1, dat_indx_step))


class LBADepthStream:
    """The LBA driver loop (test_KVNet_LBA.py:306-528) as an object: one `step(ref_indx, frames)` per reference frame.

    model: KVNET(if_refined=True) on the GPU; cams_intrin: [quarter, half, image size] camera dicts; traj_extMs_init: the
    tracker's trajectory (list of numpy 4x4; kept, a private copy is refined); refresh_frames: every ref_indx divisible by it
    restarts the filter from the initial trajectory.  State: `traj_extMs` (refined so far), `bv_predict`, `first_frame`."""

    def __init__(self, model, cams_intrin, d_candi, t_win_r, dat_indx_step, traj_extMs_init, LBA_max_iter=20, LBA_step=.01,
                 opt_vars=(1, 1), refresh_frames=1000, min_frame_idx=0, use_gt_R=False, use_dso_R=False, use_gt_t=False,
                 use_dso_t=False, opt_next_frame=False, dw_scales=DW_SCALES):
        if len(cams_intrin) != 3:
            raise ValueError("LBADepthStream: three camera dicts (quarter, half, image size), got %d" % len(cams_intrin))
        from .nets import require_volume_refiner
        require_volume_refiner(model, "LBADepthStream")
        if getattr(model, "if_upsample_d", False):
            raise NrgbdError("LBADepthStream: a model with if_upsample_d refines to 4 D candidates, the keyframe maps take D (the reference's LBA driver never builds one)")
        self.model = model
        self.cams_intrin = list(cams_intrin)
        self.d_candi = np.asarray(d_candi)
        self.t_win_r = t_win_r
        self.dat_indx_step = dat_indx_step
        self.LBA_max_iter = LBA_max_iter
        self.LBA_step = LBA_step
        self.opt_vars = list(opt_vars)
        self.refresh_frames = refresh_frames
        self.min_frame_idx = min_frame_idx
        self.switches = dict(use_gt_R=use_gt_R, use_dso_R=use_dso_R, use_gt_t=use_gt_t, use_dso_t=use_dso_t,
                             opt_next_frame=opt_next_frame)
        self.dw_scales = list(dw_scales)
        self.traj_extMs_init = copy_list(traj_extMs_init)
        self.traj_extMs = copy_list(traj_extMs_init)
        self.traj_extMs_dso = None
        self.bv_predict = None
        self.first_frame = True
        self.frame_cnt = 0

    def _rel_poses(self, ref_indx, src_frame_idx):
        ref = self.traj_extMs[ref_indx]
        poses = [torch.from_numpy(warp_homo.get_rel_extrinsicM(ref, self.traj_extMs[i]).astype(np.float32)).cuda().unsqueeze(0)
                 for i in src_frame_idx]
        return torch.cat(poses, dim=0).unsqueeze(0)

    def step(self, ref_indx, frames):
        """One reference frame.  Returns (BVs_measure [1,D,H,W], rel_pose_opt, srcs_idx) — the R-Net's log-DPV of frame
        ref_indx and the refined relative poses of the next reference frame's window with their trajectory indices — or
        (None, None, None) when the window holds an invalid pose (the filter state is dropped, :515-516)."""
        src_frame_idx = window_indices(ref_indx, self.t_win_r, self.dat_indx_step)
        valid_seq = valid_poses(self.traj_extMs, src_frame_idx)
        if ref_indx < self.min_frame_idx:
            valid_seq = False
        if self.frame_cnt == 0 or not valid_seq:
            self.bv_predict = None
        if ref_indx % self.refresh_frames == 0:                    # :329-334
            self.bv_predict = None
            self.first_frame = True
            self.traj_extMs = copy_list(self.traj_extMs_init)
        frame_cnt = self.frame_cnt
        self.frame_cnt += 1
        if not valid_seq:
            self.bv_predict = None
            return None, None, None

        if frame_cnt == 0 or self.bv_predict is None:
            # the first window of a trajectory: tracker scale -> working scale (:353-361; the surviving line is :359)
            t_norms = get_t_norms(self.traj_extMs, self.dat_indx_step)
            scale_ = self.d_candi.max() / (self.cams_intrin[0]['focal_length'] * np.array(t_norms).mean() / 2)
            rescale_traj_t(self.traj_extMs, scale_)
            self.traj_extMs_dso = copy_list(self.traj_extMs)
        src_cam_poses = self._rel_poses(ref_indx, src_frame_idx)
        cam_pose_next = torch.FloatTensor(
            warp_homo.get_rel_extrinsicM(self.traj_extMs[ref_indx], self.traj_extMs[ref_indx + 1])).cuda()
        BVs_measure, self.bv_predict = test_step.test(
            self.model, self.d_candi, Ref_Dats=[frames[ref_indx]], Src_Dats=[[frames[i] for i in src_frame_idx]],
            Cam_Intrinsics=[self.cams_intrin[0]], t_win_r=self.t_win_r, Src_CamPoses=src_cam_poses,
            BV_predict=self.bv_predict, R_net=True, cam_pose_next=cam_pose_next, ref_indx=ref_indx)
        first, self.first_frame = self.first_frame, False
        rel_pose_opt, srcs_idx = lba_update(
            self.traj_extMs, ref_indx, BVs_measure, frames, self.cams_intrin, self.d_candi, self.t_win_r, self.dat_indx_step,
            self.LBA_max_iter, self.LBA_step, self.opt_vars, first, dw_scales=self.dw_scales,
            traj_extMs_dso=self.traj_extMs_dso, **self.switches)
        return BVs_measure, rel_pose_opt, srcs_idx
