"""Record tests/golden/lba_opt_small.npz and tests/golden/lba_opt_wide.npz: the UNMODIFIED reference's local bundle adjustment
(ICP/opt_pose_numerical.py) on CPU.

    python tools/gen_lba_opt_golden.py

Runs only where the reference project is present (oracle/ref_shim.py imports it with `.cuda()` as the identity).  The inputs
come from tests/lba_fp64.py::inputs (a rendered 64 x 96 window, 4 sources, perturbed poses, dw_scales [4, 2, 1]).  For both
public forms and the three opt_vars it records, through recording stand-ins for torch.optim.Adam and nn.L1Loss placed in the
reference module's namespace (its file is not touched): the loss of every iteration, the gradients (g_t, g_uq) of every
iteration, the final (t, uq), the returned 4x4 poses and the printed d_loss lines; plus Rotation2UnitQ / UnitQ2Rotation on a set
of rotations and checksums of the inputs.

lba_opt_wide.npz (tests/lba_fp64.py WIDE_* / PAR16_*) holds outputs only: (a) local_BA_direct with the LBA driver's 20 sources
at 256 x 384, dw_scales [4, 2, 1], a confidence map built as the driver builds it, opt_vars [1, 1] and [0, 1]; (b)
local_BA_direct_parallel with 16 sources at 32 x 48.  Losses, gradients, final (t, uq), poses, prints, input checksums.

Both files are written with fixed zip timestamps, so a second run reproduces them byte for byte.
"""
import contextlib
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim  # noqa: E402
import lba_fp64 as lf  # noqa: E402
from neuralrgbd_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lba_opt_small.npz")
OUT_WIDE = os.path.join(ROOT, "tests", "golden", "lba_opt_wide.npz")


def savez_fixed(path, **arrays):
    """np.savez_compressed with a fixed timestamp on every member: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[name]), allow_pickle=False)


def _checksums(out, ref_frame, src_frames, dmap, conf, prefix=""):
    out[prefix + "cks_ref"] = float(ref_frame.double().sum())
    out[prefix + "cks_src"] = float(torch.cat(src_frames).double().sum())
    out[prefix + "cks_dmap"] = float(dmap.double().sum())
    out[prefix + "cks_conf"] = float(conf.double().sum())


def main():
    if not ref_shim.available():
        print("reference not present: nothing recorded")
        return 0
    torch.set_num_threads(1)
    ref_shim.load()
    import ICP.opt_pose_numerical as opn
    import mutils.misc as rmisc

    rec = {"loss": [], "grads": [], "params": []}

    class RecAdam(torch.optim.Adam):
        def step(self, closure=None):
            rec["grads"].append([p.grad.detach().clone() for g in self.param_groups for p in g["params"]])
            out = super().step(closure)
            rec["params"].append([p.detach().clone() for g in self.param_groups for p in g["params"]])
            return out

    class RecL1(torch.nn.L1Loss):
        def forward(self, a, b):
            out = super().forward(a, b)
            rec["loss"].append(float(out))
            return out

    opn.optim = types.SimpleNamespace(Adam=RecAdam)
    opn.nn = types.SimpleNamespace(L1Loss=RecL1)

    ref_frame, src_frames, dmap, conf, inits, true = lf.inputs()
    cams = lf.cams(lf.H, lf.W)
    out = {"H": lf.H, "W": lf.W, "seed": lf.SEED, "max_iter": lf.MAX_ITER, "step": lf.STEP,
           "dw_scales": np.asarray(lf.DW_SCALES), "inits": inits.numpy(), "true": true.numpy(),
           "cks_ref": float(ref_frame.double().sum()), "cks_src": float(torch.cat(src_frames).double().sum()),
           "cks_dmap": float(dmap.double().sum()), "cks_conf": float(conf.double().sum())}
    uq0 = torch.stack([rmisc.Rotation2UnitQ(inits[v, :3, :3].clone()) for v in range(lf.V)])
    out["uq0"] = uq0.numpy()
    for form in ("parallel", "single"):
        for ov in lf.OPT_VARS:
            tag = "%s_%d%d" % (form, ov[0], ov[1])
            rec["loss"].clear(); rec["grads"].clear()
            fn = opn.local_BA_direct_parallel if form == "parallel" else opn.local_BA_direct
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                poses = fn(ref_frame.clone(), [s.clone() for s in src_frames], dmap.clone(), conf.clone(), cams, lf.DW_SCALES,
                           [inits[v].numpy() for v in range(lf.V)], lf.MAX_ITER, lf.STEP, ov)
            nit = len(lf.DW_SCALES) * lf.MAX_ITER
            opt_R = ov[0] == 1
            opt_t = (not opt_R) or ov[1] == 1
            names = (["t"] if opt_t else []) + (["uq"] if opt_R else [])        # Adam([opt_t, opt_R]) / ([opt_R]) / ([opt_t])
            n_run = 1 if form == "parallel" else lf.V
            g_t = np.zeros((n_run, nit, lf.V if form == "parallel" else 1, 3), np.float32)
            g_uq = np.zeros_like(g_t)
            for r in range(n_run):
                for i in range(nit):
                    for name, g in zip(names, rec["grads"][r * nit + i]):
                        (g_t if name == "t" else g_uq)[r, i] = g.numpy().reshape(-1, 3)
            if form == "single":       # [view][iter][1][3] -> [iter][view][3]
                g_t = g_t[:, :, 0].transpose(1, 0, 2); g_uq = g_uq[:, :, 0].transpose(1, 0, 2)
                loss = np.asarray(rec["loss"], np.float32).reshape(lf.V, nit).T
            else:
                g_t = g_t[0]; g_uq = g_uq[0]
                loss = np.asarray(rec["loss"], np.float32).reshape(nit, 1)
            P = np.stack([p.numpy() for p in poses])
            out[tag + "_loss"] = loss
            out[tag + "_g_t"] = g_t
            out[tag + "_g_uq"] = g_uq
            out[tag + "_poses"] = P
            out[tag + "_prints"] = np.asarray(buf.getvalue().strip().split("\n"))
            print(tag, "loss", loss[0].tolist(), "->", loss[-1].tolist())
    # the final (t, uq) from the private forms, which return them
    for ov in lf.OPT_VARS:
        levels_ref = [rmisc.downsample_img(ref_frame, k) for k in lf.DW_SCALES]
        levels_d = [rmisc.downsample_img(dmap, k).squeeze() for k in lf.DW_SCALES]
        levels_c = [rmisc.downsample_img(conf, k).squeeze() for k in lf.DW_SCALES]
        srcs = torch.cat(src_frames, 0)
        levels_s = [rmisc.downsample_img(srcs, k) for k in lf.DW_SCALES]
        t0 = inits[:, :3, 3].clone()
        with contextlib.redirect_stdout(io.StringIO()):
            t, uq, _, ref_img = opn._opt_pose_warping_parallel(levels_ref, levels_d, levels_s, uq0.clone(), t0.clone(), cams,
                                                               max_iter=lf.MAX_ITER, LR=lf.STEP, opt_vars=ov,
                                                               conf_maps_ref=levels_c)
        tag = "parallel_%d%d" % (ov[0], ov[1])
        out[tag + "_t"] = t.detach().numpy().copy()
        out[tag + "_uq"] = uq.detach().numpy().copy()
        if ov == [1, 1]:
            out["ref_img"] = np.asarray(ref_img, np.float32)
        ts, uqs = [], []
        for v in range(lf.V):
            with contextlib.redirect_stdout(io.StringIO()):
                t, uq, _, _ = opn._opt_pose_warping(levels_ref, levels_d, [x[v:v + 1] for x in levels_s], uq0[v].clone(),
                                                    t0[v].clone(), cams, max_iter=lf.MAX_ITER, LR=lf.STEP, opt_vars=ov,
                                                    conf_maps_ref=levels_c)
            ts.append(t.detach().numpy().copy()); uqs.append(uq.detach().numpy().copy())
        tag = "single_%d%d" % (ov[0], ov[1])
        out[tag + "_t"] = np.stack(ts)
        out[tag + "_uq"] = np.stack(uqs)
    # Rotation2UnitQ / UnitQ2Rotation on a set of rotations (incl. the identity and larger angles)
    rng = np.random.RandomState(11)
    Rs = [np.eye(3)] + [synth.rotvec_to_R(rng.normal(0, s, 3)) for s in (0.01, 0.1, 0.5, 1.0) for _ in range(4)]
    Rs = np.stack(Rs).astype(np.float32)
    out["rot_R"] = Rs
    out["rot_uq"] = np.stack([rmisc.Rotation2UnitQ(torch.from_numpy(R.copy())).numpy() for R in Rs])
    out["rot_R_back"] = np.stack([rmisc.UnitQ2Rotation(torch.from_numpy(u.copy())).numpy() for u in out["rot_uq"]])
    savez_fixed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    wide(opn, rmisc, rec)
    return 0


def _record(opn, rec, fn, frames, cams, dw_scales, inits, ov, n_run, V):
    """One public-form call of the reference with the recorders cleared: (loss [iters, n_run], g_t / g_uq [iters, V, 3],
    final t / uq [V, 3] (uq: the initial unit quaternion when R is not optimised), poses [V, 4, 4], prints)."""
    ref_frame, src_frames, dmap, conf = frames
    rec["loss"].clear(); rec["grads"].clear(); rec["params"].clear()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        poses = fn(ref_frame.clone(), [s.clone() for s in src_frames], dmap.clone(), conf.clone(), cams, dw_scales,
                   [inits[v].numpy() for v in range(V)], lf.MAX_ITER, lf.STEP, ov)
    nit = len(dw_scales) * lf.MAX_ITER
    opt_R = ov[0] == 1
    opt_t = (not opt_R) or ov[1] == 1
    names = (["t"] if opt_t else []) + (["uq"] if opt_R else [])
    per = V // n_run
    g = {"t": np.zeros((nit, V, 3), np.float32), "uq": np.zeros((nit, V, 3), np.float32)}
    fin = {"t": np.full((V, 3), np.nan, np.float32), "uq": np.full((V, 3), np.nan, np.float32)}
    for r in range(n_run):
        for i in range(nit):
            for name, x in zip(names, rec["grads"][r * nit + i]):
                g[name][i, r * per:(r + 1) * per] = x.numpy().reshape(-1, 3)
        for name, x in zip(names, rec["params"][r * nit + nit - 1]):
            fin[name][r * per:(r + 1) * per] = x.numpy().reshape(-1, 3)
    loss = np.asarray(rec["loss"], np.float32).reshape(n_run, nit).T
    return {"loss": loss, "g_t": g["t"], "g_uq": g["uq"], "t": fin["t"], "uq": fin["uq"],
            "poses": np.stack([p.numpy() for p in poses]), "prints": np.asarray(buf.getvalue().strip().split("\n"))}


def wide(opn, rmisc, rec):
    out = {"max_iter": lf.MAX_ITER, "step": lf.STEP, "dw_scales": np.asarray(lf.DW_SCALES)}
    # (a) the driver's local_BA_direct window
    ref_frame, src_frames, dmap, conf, inits, true = lf.inputs(lf.WIDE_SEED, lf.WIDE_H, lf.WIDE_W, lf.WIDE_V,
                                                               conf_kind="driver")
    _checksums(out, ref_frame, src_frames, dmap, conf, "wide_")
    out["wide_inits"] = inits.numpy()
    out["wide_uq0"] = np.stack([rmisc.Rotation2UnitQ(inits[v, :3, :3].clone()).numpy() for v in range(lf.WIDE_V)])
    cams = lf.cams(lf.WIDE_H, lf.WIDE_W)
    for ov in lf.WIDE_OPT_VARS:
        r = _record(opn, rec, opn.local_BA_direct, (ref_frame, src_frames, dmap, conf), cams, lf.DW_SCALES, inits, ov,
                    lf.WIDE_V, lf.WIDE_V)
        if ov[0] != 1:
            r["uq"] = out["wide_uq0"].copy()
        for k, v in r.items():
            out["wide_%d%d_%s" % (ov[0], ov[1], k)] = v
        print("wide", ov, "loss", r["loss"][0, :3].tolist(), "->", r["loss"][-1, :3].tolist())
    # (b) local_BA_direct_parallel with 16 sources
    ref_frame, src_frames, dmap, conf, inits, true = lf.inputs(lf.PAR16_SEED, lf.PAR16_H, lf.PAR16_W, lf.PAR16_V)
    _checksums(out, ref_frame, src_frames, dmap, conf, "par16_")
    out["par16_inits"] = inits.numpy()
    out["par16_uq0"] = np.stack([rmisc.Rotation2UnitQ(inits[v, :3, :3].clone()).numpy() for v in range(lf.PAR16_V)])
    r = _record(opn, rec, opn.local_BA_direct_parallel, (ref_frame, src_frames, dmap, conf), lf.cams(lf.PAR16_H, lf.PAR16_W),
                lf.DW_SCALES, inits, [1, 1], 1, lf.PAR16_V)
    for k, v in r.items():
        out["par16_11_%s" % k] = v
    print("par16 loss", r["loss"][0].tolist(), "->", r["loss"][-1].tolist())
    savez_fixed(OUT_WIDE, **out)
    print("wrote", OUT_WIDE, os.path.getsize(OUT_WIDE), "bytes")


if __name__ == "__main__":
    sys.exit(main())
