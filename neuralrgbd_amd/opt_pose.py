"""Local bundle adjustment (pose refinement) of the LBA inference mode — ICP/opt_pose_numerical.py on gfx950 kernels.

Same names, arguments, defaults and return values as the reference's four functions.  The whole Adam schedule (scales x
iterations) runs on the device as two launches per iteration (lba.hip: the fused loss + gradient pass and the one-workgroup
pose update) with no host synchronisation; the host reads back only what the return values need (the poses, the last level's
reference image) and the loss log behind the reference's d_loss prints, which it prints after the run.  local_BA_direct takes
any number of source frames (the LBA driver passes 20) in groups of at most ops.MAX_V; the joint forms take at most ops.MAX_V.

Not reproduced (a clear error instead): bi_direct_warp=True (unimplemented in the parallel form, and its single-view branch
needs the inverse-warp quaternion the optimiser never uses), r_para other than 'unit_quat' (the reference's other branches test
string identity and are unused), conf_maps_ref=None (both forms index it before the check and crash), max_iter < 1 (the
reference returns an unassigned ref_img).
"""
import numpy as np
import torch

from . import homography as _homo
from . import misc as m_misc
from . import ops


def _normalize_img(img):
    """opt_pose_numerical.py:23-26, evaluated on the host."""
    img_ = img.detach().cpu()
    img_out = (img_ - img_.min()) / (img_.max() - img_.min())
    return img_out.squeeze().numpy().transpose([1, 2, 0])


def _flags(opt_vars, bi_direct_warp, conf_maps_ref, r_para, max_iter):
    """(opt_R, opt_t) as the reference selects its Adam parameters; raises for what is not reproduced."""
    if bi_direct_warp:
        raise NotImplementedError("local BA: bi_direct_warp=True is not supported (the reference's parallel form raises "
                                  "'not implemented' for it)")
    if r_para != 'unit_quat':
        raise NotImplementedError("local BA: only r_para='unit_quat' is supported, got %r" % (r_para,))
    if conf_maps_ref is None:
        raise ValueError("local BA: conf_maps_ref is required (the reference indexes it unconditionally)")
    if int(max_iter) < 1:
        raise ValueError("local BA: max_iter must be >= 1, got %r" % (max_iter,))
    opt_R = opt_vars[0] == 1
    if not opt_R:
        return False, True                    # R fixed from R_init; Adam over t alone (:60-66, :208-214)
    if opt_vars[1] == 1:
        return True, True
    if opt_vars[1] == 0:
        return True, False
    raise Exception('undefined optmization variable option')


def _device():
    if not torch.cuda.is_available():
        raise ops._lib.NrgbdError("local BA runs on the GPU only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _run(levels, init, max_iter, LR, opt_R, opt_t, joint):
    """The whole optimisation on the device, no host synchronisation.

    levels: per scale (ref [3,h,w], src [N,3,h,w], dmap [h,w], conf [h,w], K [3,3], rays [3,hw]), CUDA fp32, coarse first;
    init [N,6] = (uq, t) per view.  joint: one loss over all views (normaliser N 3 h w, _opt_pose_warping_parallel) or N
    independent losses (3 h w each: N separate _opt_pose_warping runs batched into the same launches).
    Returns (state [N, ops.LBA_STATE]: uq = [:, 0:3], t = [:, 3:6], R = [:, 6:15]; loss_log [1 or N, scales * max_iter]:
    the loss at each iteration before its step)."""
    N = levels[0][1].shape[0]
    dev = levels[0][1].device
    nwg = max(ops.lba_workgroups(lv[1].shape[2], lv[1].shape[3]) for lv in levels)
    state = torch.empty((N, ops.LBA_STATE), dtype=torch.float32, device=dev)
    partial = torch.empty(N * nwg * 13, dtype=torch.float32, device=dev)
    loss_log = torch.empty((1 if joint else N, len(levels) * max_iter), dtype=torch.float32, device=dev)
    ops.lba_init(init, state)
    step = 0
    for iscale, lv in enumerate(levels):
        lr = LR / (2 ** iscale) if iscale > 0 else LR
        level = ops.LbaLevel(*lv, state, partial, loss_log, joint, opt_R, opt_t)
        for it in range(max_iter):
            step += 1
            level.grad()
            level.update(iscale * max_iter + it, step, lr)
    return state, loss_log


def _print_d_loss(log, nscale, max_iter):
    """opt_pose_numerical.py:146-157 / :276-291 from the device log: (loss at max_iter-1 - loss at 0) * 100 per scale."""
    for iscale in range(nscale):
        loss_0 = np.asarray(log[iscale * max_iter], dtype=np.float32)
        loss_1 = np.asarray(log[iscale * max_iter + max_iter - 1], dtype=np.float32)
        print('opt_pose(): scale=%d, iter %d/%d, d_loss = %f' % (iscale, max_iter, max_iter, (loss_1 - loss_0) * 100))


def _cam_level(cam, h, w, dev):
    K, rays = _homo._cam_dev(cam, dev)
    if rays.shape[1] != h * w:
        raise ValueError("local BA: cams_intrinsic level has %d rays, the pooled level is %dx%d" % (rays.shape[1], h, w))
    return K, rays


def _levels_from_lists(imgs_ref, dmaps_ref, imgs_src, conf_maps_ref, cams_intrinsic, dev):
    levels = []
    for iscale in range(len(imgs_ref)):
        src = imgs_src[iscale].to(device=dev, dtype=torch.float32).contiguous()
        N, _, h, w = src.shape
        ref = imgs_ref[iscale].to(device=dev, dtype=torch.float32).reshape(3, h, w).contiguous()
        dmap = dmaps_ref[iscale].to(device=dev, dtype=torch.float32).reshape(h, w).contiguous()
        conf = conf_maps_ref[iscale].to(device=dev, dtype=torch.float32).reshape(h, w).contiguous()
        levels.append((ref, src, dmap, conf) + _cam_level(cams_intrinsic[iscale], h, w, dev))
    return levels


def _opt_pose(imgs_ref, dmaps_ref, imgs_src, R_init, t_init, cams_intrinsic, max_iter, LR, opt_vars, bi_direct_warp,
              conf_maps_ref, r_para, n_view):
    opt_R, opt_t = _flags(opt_vars, bi_direct_warp, conf_maps_ref, r_para, max_iter)
    if not 1 <= n_view <= ops.MAX_V:
        raise ValueError("local BA: %d source views, at most %d" % (n_view, ops.MAX_V))
    dev = _device()
    levels = _levels_from_lists(imgs_ref, dmaps_ref, imgs_src, conf_maps_ref, cams_intrinsic, dev)
    init = torch.cat((R_init.reshape(n_view, 3), t_init.reshape(n_view, 3)), 1).to(device=dev, dtype=torch.float32)
    state, log = _run(levels, init.contiguous(), int(max_iter), LR, opt_R, opt_t, joint=True)
    _print_d_loss(log[0].cpu().numpy(), len(levels), int(max_iter))
    ref_img = _normalize_img(imgs_ref[-1])
    return state[:, 3:6], state[:, 0:3], ref_img


def _opt_pose_warping(imgs_ref, dmaps_ref, imgs_src, R_init, t_init, cams_intrinsic, max_iter=100, LR=1e-2, opt_vars=[1, 1],
                      dmap_src=None, bi_direct_warp=False, conf_maps_ref=None, r_para='unit_quat'):
    """One source view (opt_pose_numerical.py:28-170): imgs_* lists over scales of [1,3,h,w], dmaps_ref / conf_maps_ref of
    [h,w], R_init the 3-vector unit quaternion, t_init [3].  Returns (t [3], uq [3] (R_init itself when R is not optimised),
    [], ref_img)."""
    if opt_vars[0] == 1:
        assert R_init.dim() == 1 and (len(R_init) == 3 or len(R_init) == 4), 'R_init should be of dim-1 3-ele/4-ele vector'
    t, uq, ref_img = _opt_pose(imgs_ref, dmaps_ref, imgs_src, R_init, t_init, cams_intrinsic, max_iter, LR, opt_vars,
                               bi_direct_warp, conf_maps_ref, r_para, 1)
    return t.reshape(3), (uq.reshape(3) if opt_vars[0] == 1 else R_init), [], ref_img


def _opt_pose_warping_parallel(imgs_ref, dmaps_ref, imgs_src, R_init, t_init, cams_intrinsic, max_iter=100, LR=1e-2,
                               opt_vars=[1, 1], dmap_src=None, bi_direct_warp=False, conf_maps_ref=None, r_para='unit_quat'):
    """N > 1 source views optimised jointly (opt_pose_numerical.py:172-303): imgs_src lists over scales of [N,3,h,w], R_init
    [N,3] unit quaternions, t_init [N,3].  Returns (t [N,3], uq [N,3] (R_init itself when R is not optimised), [], ref_img)."""
    assert imgs_src[0].shape[0] > 1  # should have more than one src view
    assert r_para == 'unit_quat'
    n_view = imgs_src[0].shape[0]
    t, uq, ref_img = _opt_pose(imgs_ref, dmaps_ref, imgs_src, R_init, t_init, cams_intrinsic, max_iter, LR, opt_vars,
                               bi_direct_warp, conf_maps_ref, r_para, n_view)
    return t, (uq if opt_vars[0] == 1 else R_init), [], ref_img


def _prepare(ref_frame, src_frames, dmap_ref, conf_map_ref, cams_intrin, dw_scales, rel_pose_inits):
    """Pyramids (one nrgbd_lba_pyramid launch) and the initial parameters (Rotation2UnitQ on the host, fp32)."""
    assert isinstance(ref_frame, torch.Tensor) and isinstance(src_frames[0], torch.Tensor) \
        and isinstance(dmap_ref, torch.Tensor) and isinstance(conf_map_ref, torch.Tensor)
    N = len(src_frames)
    if not 1 <= N <= ops.MAX_V or len(rel_pose_inits) != N:
        raise ValueError("local BA: %d source frames / %d initial poses (equal, at most %d)" % (N, len(rel_pose_inits), ops.MAX_V))
    if len(cams_intrin) < len(dw_scales):
        raise ValueError("local BA: %d scales but %d camera levels" % (len(dw_scales), len(cams_intrin)))
    H, W = ref_frame.shape[2], ref_frame.shape[3]
    ks = [max(1, int(k)) for k in dw_scales]
    for iscale, k in enumerate(ks):
        npts = cams_intrin[iscale]['unit_ray_array_2D'].shape[1]
        if npts != (H // k) * (W // k):
            raise ValueError("local BA: cams_intrin[%d] has %d rays, the level pooled by %d is %dx%d"
                             % (iscale, npts, k, H // k, W // k))
    uq0, t0 = [], []
    for init_pose in rel_pose_inits:
        init_pose_th = torch.FloatTensor(np.asarray(init_pose)).clone()
        t0.append(init_pose_th[:3, 3])
        uq0.append(m_misc.Rotation2UnitQ(init_pose_th[:3, :3]))
    init_host = torch.cat((torch.stack(uq0), torch.stack(t0)), 1)
    dev = _device()
    frames = [ref_frame] + list(src_frames)
    for f in frames:
        if tuple(f.shape) != (1, 3, H, W):
            raise ValueError("local BA: frames must be [1,3,%d,%d], got %s" % (H, W, tuple(f.shape)))
    planes = []
    for f in frames:
        f = f.to(device=dev, dtype=torch.float32).contiguous()
        planes += [f[0, c] for c in range(3)]
    planes.append(dmap_ref.to(device=dev, dtype=torch.float32).reshape(H, W).contiguous())
    planes.append(conf_map_ref.to(device=dev, dtype=torch.float32).reshape(H, W).contiguous())
    init = init_host.to(dev)
    levels = []
    for iscale, lv in enumerate(ops.lba_pyramid(planes, ks)):
        h, w = lv.shape[1], lv.shape[2]
        levels.append((lv[0:3], lv[3:3 + 3 * N].view(N, 3, h, w), lv[3 + 3 * N], lv[4 + 3 * N])
                      + _cam_level(cams_intrin[iscale], h, w, dev))
    return levels, init


def _poses(state):
    """[[UnitQ2Rotation(uq), t], [0,0,0,1]] per view as 4x4 CPU float tensors (opt_pose_numerical.py:348-354, :410-415)."""
    host = state.cpu()
    out = []
    for i in range(host.shape[0]):
        rel_pose = torch.eye(4)
        rel_pose[:3, 3] = host[i, 3:6]
        rel_pose[:3, :3] = m_misc.UnitQ2Rotation(host[i, 0:3])
        out.append(rel_pose)
    return out


def local_BA_direct_parallel(ref_frame, src_frames, dmap_ref, conf_map_ref, cams_intrin, dw_scales, rel_pose_inits, max_iter,
                             step, opt_vars):
    """Optimise the poses of all source frames jointly (opt_pose_numerical.py:306-355).  ref_frame [1,3,H,W], src_frames list
    of [1,3,H,W], dmap_ref / conf_map_ref [1,1,H,W], cams_intrin per scale (the pooled sizes), dw_scales e.g. [4, 2, 1],
    rel_pose_inits 4x4 (ref -> src).  Returns the list of refined 4x4 CPU float tensors.  The views share one loss normaliser,
    so they run in one group: at most ops.MAX_V source frames."""
    assert len(src_frames) > 1  # should have more than one src view (:198)
    if len(src_frames) > ops.MAX_V:
        raise ValueError("local_BA_direct_parallel: %d source frames, at most %d (the views share one loss normaliser and "
                         "run in one group; local_BA_direct takes any number)" % (len(src_frames), ops.MAX_V))
    opt_R, opt_t = _flags(opt_vars, False, conf_map_ref, 'unit_quat', max_iter)
    levels, init = _prepare(ref_frame, src_frames, dmap_ref, conf_map_ref, cams_intrin, dw_scales, rel_pose_inits)
    state, log = _run(levels, init, int(max_iter), step, opt_R, opt_t, joint=True)
    _print_d_loss(log[0].cpu().numpy(), len(levels), int(max_iter))
    return _poses(state)


def local_BA_direct(ref_frame, src_frames, dmap_ref, conf_map_ref, cams_intrin, dw_scales, rel_pose_inits, max_iter, step,
                    opt_vars):
    """Optimise the pose of each source frame on its own (opt_pose_numerical.py:358-417); arguments and return value as
    local_BA_direct_parallel, any number of source frames (the driver passes 20).  Each view has its own normaliser 3 h w and
    its own Adam state, so the views run in groups of at most ops.MAX_V, each group's independent optimisations in the same
    launches; a view's result does not depend on its group (the grad kernel indexes views by blockIdx.y, the update reduces
    each view's rows on their own).  The d_loss lines are printed in view order after the last group."""
    opt_R, opt_t = _flags(opt_vars, False, conf_map_ref, 'unit_quat', max_iter)
    N = len(src_frames)
    if N < 1 or len(rel_pose_inits) != N:
        raise ValueError("local BA: %d source frames / %d initial poses (equal, at least 1)" % (N, len(rel_pose_inits)))
    poses, logs = [], []
    for g0 in range(0, N, ops.MAX_V):
        levels, init = _prepare(ref_frame, src_frames[g0:g0 + ops.MAX_V], dmap_ref, conf_map_ref, cams_intrin, dw_scales,
                                rel_pose_inits[g0:g0 + ops.MAX_V])
        state, log = _run(levels, init, int(max_iter), step, opt_R, opt_t, joint=False)
        poses += _poses(state)
        logs.append(log)
    log = torch.cat(logs).cpu().numpy()
    for i_src in range(log.shape[0]):
        _print_d_loss(log[i_src], len(levels), int(max_iter))
    return poses
