"""Record tests/golden/lba_step.npz: the UNMODIFIED reference on one LBA step (test_KVNet_LBA.py:408-511), on CPU.

    python tools/gen_lba_step_golden.py

Runs only where the reference project is present (oracle/ref_shim.py imports it with `.cuda()` as the identity).  Inputs come
from tests/lba_step_inputs.py (a rendered 6-frame video at 64 x 96, D = 16, t_win_r = 2, dat_indx_step = 1, a log-DPV peaked at
the rendered depth in place of the R-Net output).  The step is driven through the reference's own functions in the driver's
order: warping.homography.resample_vol_cuda + clamp, mutils.misc.depth_val_regression, torch.max, exp ** 2,
mutils.misc.get_twin_rel_pose, ICP.opt_pose_numerical.local_BA_direct / local_BA_direct_parallel, the trajectory updates.

Recorded (outputs only): the resampled volume and the four maps; the poses both optimisers return and the trajectory after
each update; get_twin_rel_pose's poses and index lists for every switch combination the driver reaches, at dat_indx_step 1 and
5; the same step with the reference run against ITSELF (1 / 8 threads, oneDNN on / off): `self_pose` / `self_traj` = the largest
difference of any returned pose / trajectory entry between those runs — what a pose gate on this input has to allow; checksums
of the inputs.  Fixed zip timestamps: a second run reproduces the file byte for byte."""
import contextlib
import io
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import ref_shim  # noqa: E402
import lba_step_inputs as li  # noqa: E402
from gen_lba_opt_golden import savez_fixed  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lba_step.npz")


def ref_step(ref, opn, sc, max_iter, step, opt_vars):
    """One driver step on the reference's functions; returns a dict of numpy outputs."""
    rmisc, rhomo = ref.misc, ref.homography
    cams = li.cams()
    traj = [t.copy() for t in sc["traj"]]
    frames = sc["frames"]
    BV = sc["BV"].clone()
    d_candi = li.D_CANDI
    ref_indx, idx_ref_ = li.REF, li.REF + 1
    out = {}
    pose_next = torch.FloatTensor(rhomo.get_rel_extrinsicM(traj[ref_indx], traj[idx_ref_]))
    with contextlib.redirect_stdout(io.StringIO()):
        BV_tmp = rhomo.resample_vol_cuda(src_vol=BV, rel_extM=pose_next.inverse(), cam_intrinsic=cams[2], d_candi=d_candi,
                                         d_candi_new=d_candi, padding_value=math.log(1. / float(len(d_candi)))
                                         ).clamp(max=0, min=-1000.)
        dmap_ref = rmisc.depth_val_regression(BV, d_candi, BV_log=True).squeeze()
        conf_ref, _ = torch.max(BV.squeeze(), dim=0)
        dmap_kf = rmisc.depth_val_regression(BV_tmp.unsqueeze(0), d_candi, BV_log=True).squeeze()
        conf_kf, _ = torch.max(BV_tmp.squeeze(), dim=0)
        conf_ref = torch.exp(conf_ref).squeeze() ** 2
        conf_kf = torch.exp(conf_kf).squeeze() ** 2
        out.update(pose_next=pose_next.numpy(), pose_next_inv=pose_next.inverse().numpy(), resampled=BV_tmp.numpy(),
                   dmap_ref=dmap_ref.numpy(), conf_ref=conf_ref.numpy(), dmap_kf=dmap_kf.numpy(), conf_kf=conf_kf.numpy())
        inits_all, idx_all = rmisc.get_twin_rel_pose(traj, ref_indx, li.T_WIN_R * li.STEP, 1, use_gt_R=False, use_gt_t=False,
                                                     dataset=frames)
        poses = opn.local_BA_direct(frames[ref_indx]["img"], [frames[i]["img"] for i in idx_all], dmap_ref[None, None],
                                    conf_ref[None, None], cams, li.DW_SCALES, inits_all, max_iter=max_iter, step=step,
                                    opt_vars=opt_vars)
        for idx, srcidx in enumerate(idx_all):
            traj[srcidx] = np.matmul(poses[idx].cpu().numpy(), traj[ref_indx])
        out.update(direct_idx=np.asarray(idx_all), direct_inits=np.stack([p.numpy() for p in inits_all]),
                   direct_poses=np.stack([p.detach().numpy() for p in poses]), traj_after_direct=np.stack(traj))
        inits, srcs_idx = rmisc.get_twin_rel_pose(traj, idx_ref_, li.T_WIN_R, li.STEP, use_gt_R=False, use_dso_R=False,
                                                  use_gt_t=False, use_dso_t=False, dataset=frames,
                                                  traj_extMs_dso=None, opt_next_frame=False)
        poses = opn.local_BA_direct_parallel(frames[idx_ref_]["img"], [frames[i]["img"] for i in srcs_idx], dmap_kf[None, None],
                                             conf_kf[None, None], cams, li.DW_SCALES, inits, max_iter=max_iter, step=step,
                                             opt_vars=opt_vars)
        for idx, srcidx in enumerate(srcs_idx):
            traj[srcidx] = np.matmul(poses[idx].cpu().numpy(), traj[idx_ref_])
        out.update(par_idx=np.asarray(srcs_idx), par_inits=np.stack([p.numpy() for p in inits]),
                   par_poses=np.stack([p.detach().numpy() for p in poses]), traj_after_par=np.stack(traj))
    return out


def twin_records(rmisc):
    traj, dso, dataset = li.index_traj()
    out = {}
    for n, (ref_indx, t_win_r, step, kw) in enumerate(li.twin_cases()):
        kw = dict(kw)
        if kw.pop("with_dso", False):
            kw["traj_extMs_dso"] = [d.copy() for d in dso]
        with contextlib.redirect_stdout(io.StringIO()):
            poses, idx = rmisc.get_twin_rel_pose([t.copy() for t in traj], ref_indx, t_win_r, step, dataset=dataset, **kw)
        out["twin_%03d_poses" % n] = np.stack([p.numpy() for p in poses])
        out["twin_%03d_idx" % n] = np.asarray(idx)
    out["twin_n"] = n + 1
    return out


def main():
    if not ref_shim.available():
        print("reference not present: nothing recorded")
        return 0
    ref = ref_shim.load()
    import ICP.opt_pose_numerical as opn
    sc = li.scene()
    out = {"H": li.H, "W": li.W, "D": li.D, "seed": li.SEED, "max_iter": li.MAX_ITER, "step": li.LBA_STEP}
    out.update(li.checksums(sc))
    torch.set_num_threads(1)
    base = ref_step(ref, opn, sc, li.MAX_ITER, li.LBA_STEP, [1, 1])
    out.update(base)
    # the reference against itself: only the execution changes
    self_pose, self_traj = 0.0, 0.0
    for threads, mkldnn in ((8, True), (1, False), (8, False)):
        torch.set_num_threads(threads)
        with torch.backends.mkldnn.flags(enabled=mkldnn):
            o = ref_step(ref, opn, sc, li.MAX_ITER, li.LBA_STEP, [1, 1])
        for k in ("direct_poses", "par_poses"):
            self_pose = max(self_pose, float(np.abs(o[k].astype(np.float64) - base[k]).max()))
        for k in ("traj_after_direct", "traj_after_par"):
            self_traj = max(self_traj, float(np.abs(o[k] - base[k]).max()))
        print("self-noise threads=%d oneDNN=%s: pose %.3e traj %.3e" % (threads, mkldnn, self_pose, self_traj))
    torch.set_num_threads(1)
    out["self_pose"], out["self_traj"] = self_pose, self_traj
    out.update(twin_records(ref.misc))
    savez_fixed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
