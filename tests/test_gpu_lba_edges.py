"""Local bundle adjustment on the GPU at the driver's window and at its edge inputs: the fused loss + gradient pass against the
exact-position comparator (tests/lba_edges.py) over view counts 1 / 5 / 16, sizes from 7 x 9 to 256 x 384 and the edge contents;
exact ties (sign(0) = 0); the update kernel against torch.optim.Adam over every block of four views and workgroup counts up to
the cap; the pyramid against F.avg_pool2d in float64; local_BA_direct with the driver's 20 sources and local_BA_direct_parallel
with 16 against the unmodified reference's recorded runs (tests/golden/lba_opt_wide.npz)."""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lba_edges as le
import lba_fp64 as lf
from conftest import GOLDEN
from neuralrgbd_amd import misc, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _kernel_sums(level):
    """lba_grad at the level's poses -> the unnormalised sums over the workgroup partials [N, 13] in float64."""
    ref, src, dmap, conf, K, rays, R, t = level
    N, _, H, W = src.shape
    state = torch.zeros((N, ops.LBA_STATE))
    state[:, 3:6] = torch.from_numpy(t)
    state[:, 6:15] = torch.from_numpy(R).reshape(N, 9)
    nwg = ops.lba_workgroups(H, W)
    partial = torch.full((N * nwg * 13,), float("nan"), device=DEV)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    ops.lba_grad(d(ref), d(src), d(dmap), d(conf), d(K), d(rays), state.to(DEV), partial)
    p = partial.view(N, nwg, 13).double().cpu().numpy()
    assert np.isfinite(p).all()
    return p.sum(1)


def _check_exact(level, tag):
    e = le.exact_sums(level)
    s = _kernel_sums(level)
    d_g = np.abs(s[:, :12] - e["g"])
    d_L = np.abs(s[:, 12] - e["loss"])
    worst = (d_g / e["g_bound"]).max()
    print("[parity] lba_grad %s vs exact-position comparator: |dg| / bound %.2f  |dL| / bound %.2f  (ties %d, masked %d, "
          "partly out %d)" % (tag, worst, (d_L / e["loss_bound"]).max(), e["ties"], e["masked"], e["partial_taps"]))
    assert (d_g <= e["g_bound"]).all(), (tag, np.argwhere(d_g > e["g_bound"])[:5])
    assert (d_L <= e["loss_bound"]).all(), tag
    return s


@pytest.mark.parametrize("N", [1, 5, 16])
@pytest.mark.parametrize("H,W", le.SIZES, ids=lambda v: str(v))
def test_fused_pass_vs_exact_comparator(H, W, N):
    """Every size (nwg 1; 25; exactly 256; 256 with a grid-stride remainder; 384 pixels per lane row) x view count with the mixed
    content: zero borders, one zeroed channel, confidence zeros, small / large / behind-the-camera / true poses in turn."""
    _check_exact(le.edge_level(H, W, N, "mixed"), "%dx%d N=%d mixed" % (H, W, N))


@pytest.mark.parametrize("content", ["small", "zeros", "conf0", "large", "behind", "true"])
@pytest.mark.parametrize("H,W", [(65, 97), (256, 257)], ids=lambda v: str(v))
def test_fused_pass_edge_contents(H, W, content):
    """Each content alone with 5 views (two blocks of the update's reduction).  Where the poses are perturbed by 0.01 rad / 0.02
    (small, zeros, conf0) the existing gate against the float64 restatement holds as well: 1e-4 of max |g|.  Host-measured spread
    of the fp32 positions (the C oracle) against float64 on these inputs: at most 6.0e-5 (256 x 256, conf0); at large
    perturbations, behind the camera and at the true pose it reaches 5.4e-4, 3.9e-4 and 2.9e-3, where only the exact comparator
    gates.  No GPU number existed for these cases when the gates were set."""
    level = le.edge_level(H, W, 5, content)
    s = _check_exact(level, "%dx%d N=5 %s" % (H, W, content))
    if content in ("small", "zeros", "conf0"):
        N = 5
        L, gR, gt = lf.loss_and_grad(le.fp64_level(level), torch.from_numpy(level[6]), torch.from_numpy(level[7]), joint=True,
                                     param="R")
        g64 = np.concatenate([gR.reshape(N, 9), gt], 1)
        got = s[:, :12] / (N * 3.0 * H * W)
        e_g = np.abs(got - g64).max() / np.abs(g64).max()
        e_L = abs(s[:, 12].sum() / (N * 3.0 * H * W) - L) / L
        print("[parity] lba_grad %dx%d %s vs fp64: loss rel %.2e  g %.2e (of max |g|)" % (H, W, content, e_L, e_g))
        assert e_L < 1e-5 and e_g <= 1e-4


def test_exact_ties_give_zero():
    """Every sample lands exactly on a pixel centre (power-of-two size, unit focal length, identity pose) of a source equal to
    the reference: r = 0 exactly everywhere, and sign(0) = 0 makes every partial exactly 0."""
    H, W, N = 64, 64, 5
    rng = np.random.RandomState(3)
    ref = rng.standard_normal((3, H, W)).astype(np.float32)
    src = np.repeat(ref[None], N, 0)
    K = np.array([[1, 0, W / 2], [0, 1, H / 2], [0, 0, 1]], np.float32)
    ys, xs = np.meshgrid(np.arange(H) + 0.5 - H / 2, np.arange(W) + 0.5 - W / 2, indexing="ij")
    rays = np.stack([xs.reshape(-1), ys.reshape(-1), np.ones(H * W)]).astype(np.float32)
    R = np.repeat(np.eye(3, dtype=np.float32)[None], N, 0)
    t = np.zeros((N, 3), np.float32)
    conf = (0.2 + 0.8 * rng.rand(H, W)).astype(np.float32)
    level = (ref, src, np.ones((H, W), np.float32), conf, K, rays, R, t)
    w = le.co.warp_depth_fwd(src, level[2], K, R, t, rays)
    assert np.array_equal(w, src)                       # the positions are exact: the test's premise
    assert np.array_equal(_kernel_sums(level), np.zeros((N, 13)))


def _uq_to_R_f32(uq):
    q = torch.zeros(4)
    misc.unitQ_to_quat(uq, q)
    return misc.quaternion2Rotation(q)


def _adam_run(N, nwg, joint, opt_R, opt_t, steps, lr_of, seed):
    """The update kernel for `steps` steps on synthetic partials [N, nwg, 13] vs torch.optim.Adam (CPU, fp32) fed the same
    gradients (d/d uq through the reference's quaternion chain by fp32 autograd); returns (kernel state, torch uq, torch t,
    loss_log, expected losses)."""
    rng = np.random.RandomState(seed)
    H, W = 1, 256 * nwg                     # lba_workgroups(1, 256 nwg) = nwg: the update reads exactly nwg rows per view
    assert ops.lba_workgroups(H, W) == nwg
    uq0 = (0.05 * rng.standard_normal((N, 3))).astype(np.float32)
    t0 = (0.1 * rng.standard_normal((N, 3))).astype(np.float32)
    state = torch.empty((N, ops.LBA_STATE), device=DEV)
    ops.lba_init(torch.from_numpy(np.concatenate([uq0, t0], 1)).to(DEV), state)
    uq = torch.from_numpy(uq0.copy()).requires_grad_(True)
    t = torch.from_numpy(t0.copy()).requires_grad_(True)
    opt = torch.optim.Adam(([uq] if opt_R else []) + ([t] if opt_t else []), lr=0.01, betas=(.9, .999))
    slots = steps + 7                       # log_stride larger than the slots used
    SENT = -777.25
    log = torch.full((1 if joint else N, slots), SENT, device=DEV)
    norm = 3.0 * H * W * (N if joint else 1)
    want = np.full((1 if joint else N, slots), SENT, np.float32)
    for step in range(1, steps + 1):
        lr = lr_of(step)
        for g in opt.param_groups:
            g["lr"] = lr
        part = (rng.standard_normal((N, nwg, 13)) * 50).astype(np.float32)
        slot = step + 2
        ops.lba_update(torch.from_numpy(part).to(DEV), state, log, slot, H, W, joint, step, lr, opt_R, opt_t)
        S = part.astype(np.float64).sum(1)
        want[:, slot] = S[:, 12].sum() / norm if joint else S[:, 12] / norm
        G = torch.from_numpy(S / norm)
        opt.zero_grad()
        if opt_R:
            Rm = torch.stack([_uq_to_R_f32(uq[n]) for n in range(N)])
            (Rm * G[:, :9].float().view(N, 3, 3)).sum().backward()
        if opt_t:
            t.grad = G[:, 9:12].float().clone()
        opt.step()
    return state.cpu(), uq.detach(), t.detach(), log.cpu().numpy(), want, SENT


@pytest.mark.parametrize("nwg", [1, 63, 64, 65, 200, 256])
@pytest.mark.parametrize("N", [1, 4, 5, 8, 13, 16])
def test_update_kernel_vs_torch_adam_all_view_blocks(N, nwg):
    """Every block of four views of the reduction, workgroup counts around a wave and at the cap; both forms; 60 steps (bias
    correction close to 1) with the lr halved at 20 and 40 as at the scale changes.  Gates: |uq|, |t| <= 1e-6, the existing
    test's (host-measured spread of an fp32 against a float64 Adam on such gradient sequences: 7.5e-8 after 60 steps); no GPU
    number existed for N > 4, nwg > 1 or 60 steps when the gate was set."""
    for joint in (True, False):
        st, uq, t, log, want, SENT = _adam_run(N, nwg, joint, True, True, 60, lambda s: 0.01 / 2 ** ((s - 1) // 20),
                                               1000 * N + nwg + joint)
        e_uq = (st[:, 0:3] - uq).abs().max().item()
        e_t = (st[:, 3:6] - t).abs().max().item()
        print("[parity] lba_update N=%d nwg=%d %s vs torch.optim.Adam (60 steps): |uq| %.2e  |t| %.2e"
              % (N, nwg, "joint" if joint else "per-view", e_uq, e_t))
        assert e_uq <= 1e-6 and e_t <= 1e-6
        written = want != SENT
        assert (log[~written] == SENT).all()                      # only [0, slot] / [n, slot] is written
        assert (np.abs(log[written] - want[written]) <= 1e-6 * np.abs(want[written])).all()
        for n in range(N):
            assert torch.equal(st[n, 6:15].view(3, 3), misc.UnitQ2Rotation(st[n, 0:3]))


@pytest.mark.parametrize("opt_R,opt_t", [(True, False), (False, True)])
@pytest.mark.parametrize("N,nwg", [(5, 65), (16, 256)])
def test_update_kernel_one_parameter(N, nwg, opt_R, opt_t):
    """opt_R only / opt_t only: the other parameter is unchanged bit for bit."""
    for joint in (True, False):
        st, uq, t, _, _, _ = _adam_run(N, nwg, joint, opt_R, opt_t, 12, lambda s: 0.01, 7 * N + nwg)
        assert (st[:, 0:3] - uq).abs().max().item() <= 1e-6 and (st[:, 3:6] - t).abs().max().item() <= 1e-6
        rng = np.random.RandomState(7 * N + nwg)
        uq0 = torch.from_numpy((0.05 * rng.standard_normal((N, 3))).astype(np.float32))
        t0 = torch.from_numpy((0.1 * rng.standard_normal((N, 3))).astype(np.float32))
        assert torch.equal(st[:, 0:3], uq0) if not opt_R else torch.equal(st[:, 3:6], t0)


def test_update_kernel_lr_zero_leaves_the_pose_unchanged():
    for joint in (True, False):
        st, _, _, _, _, _ = _adam_run(13, 200, joint, True, True, 5, lambda s: 0.0, 5)
        rng = np.random.RandomState(5)
        uq0 = torch.from_numpy((0.05 * rng.standard_normal((13, 3))).astype(np.float32))
        t0 = torch.from_numpy((0.1 * rng.standard_normal((13, 3))).astype(np.float32))
        assert torch.equal(st[:, 0:3], uq0) and torch.equal(st[:, 3:6], t0)
        for n in range(13):
            assert torch.equal(st[n, 6:15].view(3, 3), misc.UnitQ2Rotation(uq0[n]))


@pytest.mark.parametrize("ks", [[8, 4, 2, 1], [3], [5, 3], [1]], ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("nplanes", [1, 7, 5 + 3 * ops.MAX_V])
@pytest.mark.parametrize("H,W", [(257, 383), (375, 1242)], ids=lambda v: str(v))
def test_pyramid_vs_avg_pool2d(H, W, nplanes, ks):
    """Every plane and level against F.avg_pool2d in float64 of the full-resolution plane (sizes no level divides): the k x k fp32
    sum and the division round at most k^2 + 1 times, each relative to the window's absolute sum.  k = 1 copies bit for bit."""
    rng = np.random.RandomState(nplanes + H)
    x = torch.from_numpy(rng.standard_normal((nplanes, H, W)).astype(np.float32) * 3 + 1)
    xd = x.to(DEV)
    levels = ops.lba_pyramid([xd[i] for i in range(nplanes)], ks)
    assert len(levels) == len(ks)
    for k, lv in zip(ks, levels):
        got = lv.cpu()
        assert got.shape == (nplanes, H // k, W // k)
        if k == 1:
            assert torch.equal(got, x)
            continue
        want = F.avg_pool2d(x.double()[None], k)[0]
        mag = F.avg_pool2d(x.double().abs()[None], k)[0]
        err = (got.double() - want).abs()
        print("[parity] lba_pyramid %dx%d P=%d k=%d: max |d| / bound %.3f" % (H, W, nplanes, k, (err / ((k * k + 1) * U * mag)).max()))
        assert (err <= (k * k + 1) * U * mag).all()


def test_pyramid_levels_come_from_full_resolution_and_bad_arguments_raise():
    x = torch.randn(3, 64, 96, device=DEV)
    a, b = ops.lba_pyramid([x[i] for i in range(3)], [5, 3])
    assert torch.equal(b, ops.lba_pyramid([x[i] for i in range(3)], [3])[0])      # not pooled from the 5-level
    assert torch.equal(a, ops.lba_pyramid([x[i] for i in range(3)], [5])[0])
    with pytest.raises(ValueError, match="54 planes"):
        ops.lba_pyramid([x[0]] * (5 + 3 * ops.MAX_V + 1), [2])
    with pytest.raises(ValueError, match="kernel sizes"):
        ops.lba_pyramid([x[0]], [1] * (ops.LBA_MAX_LEVELS + 1))
    with pytest.raises(ValueError, match="kernel sizes"):
        ops.lba_pyramid([x[0]], [65])


@pytest.mark.parametrize("k", [1, 2, 3, 4, 7])
def test_downsample_img_vs_avg_pool2d(k):
    x = torch.randn(5, 3, 61, 93)
    got = misc.downsample_img(x.to(DEV), k).cpu()
    if k == 1:
        assert torch.equal(got, x)
        return
    want = F.avg_pool2d(x.double(), k)
    mag = F.avg_pool2d(x.double().abs(), k)
    assert got.shape == want.shape and ((got.double() - want).abs() <= (k * k + 1) * U * mag).all()


# ----------------------------------------------------------------------------- end to end against the reference's recording

@pytest.fixture(scope="module")
def wide():
    return dict(np.load(os.path.join(GOLDEN, "lba_opt_wide.npz")))


def _call(fn, frames, cams, inits, ov):
    ref_frame, src_frames, dmap, conf = frames
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        poses = fn(ref_frame.to(DEV), [s.to(DEV) for s in src_frames], dmap.to(DEV), conf.to(DEV), cams, lf.DW_SCALES,
                   [inits[v].numpy() for v in range(len(src_frames))], lf.MAX_ITER, lf.STEP, ov)
    return poses, buf.getvalue().strip().split("\n")


def _d_losses(lines):
    return [(m.group(1), float(m.group(2))) for m in (re.match(r"(opt_pose\(\): scale=\d+, iter \d+/\d+), d_loss = (-?\d+\.\d{6})$", s)
                                                       for s in lines)]


# The reference's loss is discontinuous where a sample leaves the frame: a channel whose warped value goes from 0 (masked) to a
# sliver of one tap adds |ref c| / (3 h w).  Poses within a few 1e-6 of the recording flip a handful of such pixels over the 20
# driver views at 256 x 384, so the loss of that run is gated at 1e-3 relative (the float64 restatement sits 9.0e-4 from the
# same recording on the host; the GPU measured 3.8e-4 with opt_vars [1, 1]); the poses keep the 1e-4 of the existing test.
# d_loss is 100 x a difference of two losses, so its gate is 200 x the loss gate x the largest loss (the existing test's 2e-3
# for losses ~0.1 at 1e-4).
LOSS_GATE = {"wide": 1e-3, "par16": 1e-4}


def _vs_golden(wide, tag, poses, lines, state_uq, state_t, log):
    e_P = np.abs(np.stack([p.numpy() for p in poses]) - wide[tag + "_poses"]).max()
    e_t = np.abs(state_t - wide[tag + "_t"]).max()
    e_uq = np.abs(state_uq - wide[tag + "_uq"]).max()
    e_loss = (np.abs(log - wide[tag + "_loss"]) / np.abs(wide[tag + "_loss"])).max()
    got_d, want_d = _d_losses(lines), _d_losses(list(wide[tag + "_prints"]))
    e_d = max(abs(a[1] - b[1]) for a, b in zip(got_d, want_d))
    print("[parity] LBA %s GPU vs reference: loss rel %.2e  |t| %.2e  |uq| %.2e  |pose| %.2e  d_loss %.1e"
          % (tag, e_loss, e_t, e_uq, e_P, e_d))
    gate = LOSS_GATE[tag.split("_")[0]]
    assert e_loss <= gate and e_t <= 1e-4 and e_uq <= 1e-4 and e_P <= 1e-4
    assert len(got_d) == len(want_d) == len(lines) and [a[0] for a in got_d] == [b[0] for b in want_d]
    assert e_d <= 200 * gate * np.abs(wide[tag + "_loss"]).max()


@pytest.mark.parametrize("ov", lf.WIDE_OPT_VARS, ids=lambda v: "%d%d" % tuple(v))
def test_local_BA_direct_driver_window_vs_reference(wide, ov):
    """The LBA driver's first window: 20 sources (t_win 2, dat_indx_step 5) at 256 x 384, the driver's confidence map."""
    from neuralrgbd_amd import opt_pose
    tag = "wide_%d%d" % tuple(ov)
    ref_frame, src_frames, dmap, conf, inits, _ = lf.inputs(lf.WIDE_SEED, lf.WIDE_H, lf.WIDE_W, lf.WIDE_V, conf_kind="driver")
    cams = lf.cams(lf.WIDE_H, lf.WIDE_W)
    poses, lines = _call(opt_pose.local_BA_direct, (ref_frame, src_frames, dmap, conf), cams, inits, ov)
    assert len(poses) == lf.WIDE_V
    opt_R, opt_t = opt_pose._flags(ov, False, conf, 'unit_quat', lf.MAX_ITER)
    sts, logs = [], []
    for g0 in range(0, lf.WIDE_V, ops.MAX_V):            # the parameters behind the poses, group by group
        levels, init = opt_pose._prepare(ref_frame, src_frames[g0:g0 + ops.MAX_V], dmap, conf, cams, lf.DW_SCALES,
                                         [inits[v].numpy() for v in range(g0, min(lf.WIDE_V, g0 + ops.MAX_V))])
        st, lg = opt_pose._run(levels, init, lf.MAX_ITER, lf.STEP, opt_R, opt_t, joint=False)
        sts.append(st.cpu().numpy()); logs.append(lg.cpu().numpy())
    st, log = np.concatenate(sts), np.concatenate(logs).T
    _vs_golden(wide, tag, poses, lines, st[:, 0:3], st[:, 3:6], log)
    # each view's result is the same bits whether it runs alone, in a group of 5 or in the 20-view call
    for v in range(lf.WIDE_V):
        one, one_lines = _call(opt_pose.local_BA_direct, (ref_frame, src_frames[v:v + 1], dmap, conf), cams, inits[v:v + 1], ov)
        assert torch.equal(one[0], poses[v]), v
        assert one_lines == lines[3 * v:3 * v + 3]
    five, _ = _call(opt_pose.local_BA_direct, (ref_frame, src_frames[15:20], dmap, conf), cams, inits[15:20], ov)
    assert all(torch.equal(a, b) for a, b in zip(five, poses[15:20]))


def test_local_BA_direct_parallel_16_views_vs_reference(wide):
    from neuralrgbd_amd import opt_pose
    tag = "par16_11"
    ref_frame, src_frames, dmap, conf, inits, _ = lf.inputs(lf.PAR16_SEED, lf.PAR16_H, lf.PAR16_W, lf.PAR16_V)
    cams = lf.cams(lf.PAR16_H, lf.PAR16_W)
    poses, lines = _call(opt_pose.local_BA_direct_parallel, (ref_frame, src_frames, dmap, conf), cams, inits, [1, 1])
    levels, init = opt_pose._prepare(ref_frame, src_frames, dmap, conf, cams, lf.DW_SCALES, [inits[v].numpy() for v in range(16)])
    st, lg = opt_pose._run(levels, init, lf.MAX_ITER, lf.STEP, True, True, joint=True)
    st = st.cpu().numpy()
    _vs_golden(wide, tag, poses, lines, st[:, 0:3], st[:, 3:6], lg.cpu().numpy().T)
    with pytest.raises(ValueError, match="at most 16"):
        _call(opt_pose.local_BA_direct_parallel, (ref_frame, src_frames + src_frames[:1], dmap, conf), cams,
              torch.cat([inits, inits[:1]]), [1, 1])
