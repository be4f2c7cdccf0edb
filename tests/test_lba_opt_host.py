"""Local bundle adjustment (neuralrgbd_amd/opt_pose.py), host side: the float64 restatement (tests/lba_fp64.py) against the
unmodified reference's recorded run (tests/golden/lba_opt_small.npz, tools/gen_lba_opt_golden.py), the host pose helpers bit
for bit, the argument errors, and convergence of the algorithm on the rendered scene the GPU test then runs."""
import os

import numpy as np
import pytest
import torch

import lba_fp64 as lf
from conftest import GOLDEN

ENVELOPE = 2.5e-5


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "lba_opt_small.npz")))


@pytest.fixture(scope="module")
def scene():
    ref_frame, src_frames, dmap, conf, inits, true = lf.inputs()
    return ref_frame, src_frames, dmap, conf, inits, true, lf.level_inputs(ref_frame, src_frames, dmap, conf, lf.cams(lf.H, lf.W))


def test_fixture_inputs_and_gradients_are_well_conditioned(golden, scene):
    ref_frame, src_frames, dmap, conf, inits, _, _ = scene
    assert abs(float(ref_frame.double().sum()) - float(golden["cks_ref"])) < 1e-6
    assert abs(float(torch.cat(src_frames).double().sum()) - float(golden["cks_src"])) < 1e-6
    assert abs(float(dmap.double().sum()) - float(golden["cks_dmap"])) < 1e-6
    assert abs(float(conf.double().sum()) - float(golden["cks_conf"])) < 1e-6
    assert np.array_equal(inits.numpy(), golden["inits"])
    # Adam's first steps are +-lr sign(g): a component near zero would flip the trajectory on rounding alone
    for form in ("parallel", "single"):
        for ov in lf.OPT_VARS:
            tag = "%s_%d%d" % (form, ov[0], ov[1])
            opt_R = ov[0] == 1
            opt_t = (not opt_R) or ov[1] == 1
            gs = ([golden[tag + "_g_t"]] if opt_t else []) + ([golden[tag + "_g_uq"]] if opt_R else [])
            for i in range(gs[0].shape[0]):
                rows = [slice(None)] if form == "parallel" else list(range(gs[0].shape[1]))   # single: per view (own run)
                for r in rows:
                    a = np.concatenate([np.abs(g[i][r]).reshape(-1) for g in gs])
                    assert a.min() / a.max() >= 1e-3, (tag, i, r)


@pytest.mark.parametrize("form", ["parallel", "single"])
@pytest.mark.parametrize("ov", lf.OPT_VARS, ids=lambda v: "%d%d" % tuple(v))
def test_fp64_restatement_vs_reference_golden(golden, scene, form, ov):
    _, _, _, _, inits, _, levels = scene
    tag = "%s_%d%d" % (form, ov[0], ov[1])
    t0 = inits[:, :3, 3].numpy()
    r = lf.run(levels, golden["uq0"], t0, lf.MAX_ITER, lf.STEP, ov, joint=(form == "parallel"))
    opt_R = ov[0] == 1
    opt_t = (not opt_R) or ov[1] == 1
    e_loss = np.abs(r["loss"] - golden[tag + "_loss"]).max() / np.abs(golden[tag + "_loss"]).max()
    e_gt = np.abs(r["g_t"] - golden[tag + "_g_t"]).max() / np.abs(golden[tag + "_g_t"]).max() if opt_t else 0.0
    e_guq = np.abs(r["g_uq"] - golden[tag + "_g_uq"]).max() / np.abs(golden[tag + "_g_uq"]).max() if opt_R else 0.0
    e_t = np.abs(r["t"] - golden[tag + "_t"]).max()
    e_uq = np.abs(r["uq"] - golden[tag + "_uq"]).max()
    P = np.stack(lf.uq_to_pose(r["uq"], r["t"]))
    e_P = np.abs(P - golden[tag + "_poses"]).max()
    print("[parity] LBA %s fp32 reference vs fp64: loss rel %.2e  g_t rel %.2e  g_uq rel %.2e  |t| %.2e  |uq| %.2e  |pose| %.2e"
          % (tag, e_loss, e_gt, e_guq, e_t, e_uq, e_P))
    assert e_loss < 2e-5 and e_gt < 5e-4 and e_guq < 5e-4   # fp32 tap selection vs fp64
    assert max(e_t, e_uq, e_P) <= ENVELOPE


def test_host_pose_helpers_are_bit_equal_to_the_reference(golden):
    from neuralrgbd_amd import misc
    for R, uq, Rb in zip(golden["rot_R"], golden["rot_uq"], golden["rot_R_back"]):
        got = misc.Rotation2UnitQ(torch.from_numpy(R.copy())).numpy()
        assert np.array_equal(got, uq) or (np.isnan(got).all() and np.isnan(uq).all())
        if np.isfinite(uq).all():
            assert np.array_equal(misc.UnitQ2Rotation(torch.from_numpy(uq.copy())).numpy(), Rb)
    for v in range(golden["inits"].shape[0]):
        assert np.array_equal(misc.Rotation2UnitQ(torch.from_numpy(golden["inits"][v, :3, :3].copy())).numpy(), golden["uq0"][v])
    # the returned poses carry UnitQ2Rotation of the final parameters bit for bit
    for n in range(4):
        P = golden["parallel_11_poses"][n]
        assert np.array_equal(misc.UnitQ2Rotation(torch.from_numpy(golden["parallel_11_uq"][n].copy())).numpy(), P[:3, :3])


def test_argument_errors_raise_before_device_work_with_20_views_allowed(scene, monkeypatch):
    """The errors raise before device work; local_BA_direct accepts the driver's 20 views (it runs them in groups of at most
    ops.MAX_V), the joint form keeps the limit."""
    from neuralrgbd_amd import opt_pose, ops
    ref_frame, src_frames, dmap, conf, inits, _, _ = scene
    cams = lf.cams(lf.H, lf.W)
    poses = [inits[v].numpy() for v in range(4)]

    def boom(*a, **k):
        raise AssertionError("device work started")
    for name in ("lba_pyramid", "lba_init", "lba_grad", "lba_update"):
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.setattr(opt_pose, "_device", boom)
    for fn in (opt_pose.local_BA_direct, opt_pose.local_BA_direct_parallel):
        with pytest.raises(ValueError, match="conf_maps_ref"):
            fn(ref_frame, src_frames, dmap, None, cams, [4, 2, 1], poses, 3, 0.01, [1, 1])
        with pytest.raises(ValueError, match="max_iter"):
            fn(ref_frame, src_frames, dmap, conf, cams, [4, 2, 1], poses, 0, 0.01, [1, 1])
        with pytest.raises(ValueError, match="rays"):
            fn(ref_frame, src_frames, dmap, conf, lf.cams(lf.H, lf.W, [2, 2, 1]), [4, 2, 1], poses, 3, 0.01, [1, 1])
        with pytest.raises(ValueError, match="initial poses"):
            fn(ref_frame, src_frames * 2, dmap, conf, cams, [4, 2, 1], poses, 3, 0.01, [1, 1])
        with pytest.raises(Exception, match="undefined optmization variable option"):
            fn(ref_frame, src_frames, dmap, conf, cams, [4, 2, 1], poses, 3, 0.01, [1, 2])
    # the joint form couples the views through one normaliser: one group, at most ops.MAX_V (local_BA_direct takes any number)
    with pytest.raises(ValueError, match="at most"):
        opt_pose.local_BA_direct_parallel(ref_frame, src_frames * 5, dmap, conf, cams, [4, 2, 1], poses * 5, 3, 0.01, [1, 1])
    with pytest.raises(AssertionError, match="device work started"):      # valid: the checks pass, the first group starts
        opt_pose.local_BA_direct(ref_frame, src_frames * 5, dmap, conf, cams, [4, 2, 1], poses * 5, 3, 0.01, [1, 1])
    with pytest.raises(ValueError, match="local_BA_direct_parallel: 17 source frames, at most 16"):
        opt_pose.local_BA_direct_parallel(ref_frame, (src_frames * 5)[:17], dmap, conf, cams, [4, 2, 1], (poses * 5)[:17], 3,
                                          0.01, [1, 1])
    levels = [[x] for x in (ref_frame, dmap[0, 0], torch.cat(src_frames), conf[0, 0])]
    uq = torch.zeros(4, 3)
    t = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="bi_direct_warp"):
        opt_pose._opt_pose_warping_parallel(levels[0], levels[1], levels[2], uq, t, cams[-1:], conf_maps_ref=levels[3],
                                            bi_direct_warp=True)
    with pytest.raises(NotImplementedError, match="r_para"):
        opt_pose._opt_pose_warping(levels[0], levels[1], [x[:1] for x in levels[2]], uq[0], t[0], cams[-1:],
                                   conf_maps_ref=levels[3], r_para="log_quat")
    with pytest.raises(ValueError, match="conf_maps_ref"):
        opt_pose._opt_pose_warping(levels[0], levels[1], [x[:1] for x in levels[2]], uq[0], t[0], cams[-1:])


def test_restatement_converges_on_the_rendered_scene(scene):
    """3 x 20 iterations at lr 0.01 (the driver's settings) bring the poses closer to the truth than the initial ones."""
    from neuralrgbd_amd import misc
    _, _, _, _, inits, true, levels = scene
    uq0 = np.stack([misc.Rotation2UnitQ(inits[v, :3, :3]).numpy() for v in range(4)])
    r = lf.run(levels, uq0, inits[:, :3, 3].numpy(), 20, 0.01, [1, 1], joint=True)
    e0 = lf.pose_error(inits.numpy(), true.numpy())
    e1 = lf.pose_error(lf.uq_to_pose(r["uq"], r["t"]), true.numpy())
    print("[lba] rendered scene: pose error (t, rad) %.4f %.4f -> %.4f %.4f; loss %.4f -> %.4f"
          % (e0[0], e0[1], e1[0], e1[1], r["loss"][0][0], r["loss"][-1][0]))
    assert e1[0] < e0[0] and e1[1] < e0[1]


@pytest.fixture(scope="module")
def wide():
    return dict(np.load(os.path.join(GOLDEN, "lba_opt_wide.npz")))


def _wide_inputs(which):
    if which == "wide":
        return lf.inputs(lf.WIDE_SEED, lf.WIDE_H, lf.WIDE_W, lf.WIDE_V, conf_kind="driver"), lf.cams(lf.WIDE_H, lf.WIDE_W)
    return lf.inputs(lf.PAR16_SEED, lf.PAR16_H, lf.PAR16_W, lf.PAR16_V), lf.cams(lf.PAR16_H, lf.PAR16_W)


# The float64 restatement against the reference's recorded wide runs.  Measured spreads (fp32 reference vs float64): the
# driver's 20-view local_BA_direct (a), opt_vars [1, 1]: loss 9.0e-4 rel, g_t 2.5e-3 rel, |t| 5.3e-5, |uq| 2.3e-5, |pose| 5.3e-5;
# [0, 1]: loss 4.8e-5, g_t 4.1e-4, |t| 4.8e-6.  The 16-view local_BA_direct_parallel (b): loss 1.2e-6, g_t 3.7e-4, g_uq 7.5e-4,
# |t| 8.6e-7, |uq| 1.4e-6, |pose| 2.7e-6.  At 256 x 384 with 20 views more pixels sit where fp32 and fp64 select different taps
# (partly out of frame, confidence down to 1e-2) than in the 4-view 64 x 96 fixture, hence the wider gates of (a).
WIDE_GATES = {"wide": (2e-3, 5e-3, 1e-4), "par16": (2e-5, 2e-3, 1e-5)}      # loss rel, gradient rel, |t| |uq| |pose|


@pytest.mark.parametrize("tag", ["wide_11", "wide_01", "par16_11"])
def test_fp64_restatement_vs_reference_wide_golden(wide, tag):
    which = tag.split("_")[0]
    (ref_frame, src_frames, dmap, conf, inits, _), cams = _wide_inputs(which)
    assert abs(float(ref_frame.double().sum()) - float(wide[which + "_cks_ref"])) < 1e-6
    assert abs(float(torch.cat(src_frames).double().sum()) - float(wide[which + "_cks_src"])) < 1e-6
    assert abs(float(dmap.double().sum()) - float(wide[which + "_cks_dmap"])) < 1e-6
    assert abs(float(conf.double().sum()) - float(wide[which + "_cks_conf"])) < 1e-6
    assert np.array_equal(inits.numpy(), wide[which + "_inits"])
    if which == "wide":                      # the driver's confidence exp(max log-prob)^2: in (0, 1]
        assert float(conf.min()) > 0 and float(conf.max()) <= 1 and float(conf.min()) < 0.02
    ov = [int(tag[-2]), int(tag[-1])]
    levels = lf.level_inputs(ref_frame, src_frames, dmap, conf, cams)
    r = lf.run(levels, wide[which + "_uq0"], inits[:, :3, 3].numpy(), lf.MAX_ITER, lf.STEP, ov, joint=(which == "par16"))
    g_loss, g_grad, g_pose = WIDE_GATES[which]
    e_loss = np.abs(r["loss"] - wide[tag + "_loss"]).max() / np.abs(wide[tag + "_loss"]).max()
    e_gt = np.abs(r["g_t"] - wide[tag + "_g_t"]).max() / np.abs(wide[tag + "_g_t"]).max()
    e_guq = np.abs(r["g_uq"] - wide[tag + "_g_uq"]).max() / np.abs(wide[tag + "_g_uq"]).max() if ov[0] == 1 else 0.0
    e_t = np.abs(r["t"] - wide[tag + "_t"]).max()
    e_uq = np.abs(r["uq"] - wide[tag + "_uq"]).max()
    e_P = np.abs(np.stack(lf.uq_to_pose(r["uq"], r["t"])) - wide[tag + "_poses"]).max()
    print("[parity] LBA %s fp32 reference vs fp64: loss rel %.2e  g_t rel %.2e  g_uq rel %.2e  |t| %.2e  |uq| %.2e  |pose| %.2e"
          % (tag, e_loss, e_gt, e_guq, e_t, e_uq, e_P))
    assert e_loss < g_loss and e_gt < g_grad and e_guq < g_grad
    assert max(e_t, e_uq, e_P) <= g_pose
    nv = wide[tag + "_poses"].shape[0]
    assert len(wide[tag + "_prints"]) == len(lf.DW_SCALES) * (nv if which == "wide" else 1)


def test_lba_pyramid_rejects_bad_arguments_before_device_work():
    """ops.lba_pyramid checks the plane count and the kernel sizes before it touches a tensor's device: these raise on CPU
    tensors with ValueError, not with the no-CPU-fallback error."""
    from neuralrgbd_amd import ops
    x = torch.zeros(64, 96)
    with pytest.raises(ValueError, match="54 planes"):
        ops.lba_pyramid([x] * (5 + 3 * ops.MAX_V + 1), [2])
    with pytest.raises(ValueError, match="0 planes"):
        ops.lba_pyramid([], [2])
    with pytest.raises(ValueError, match="kernel sizes"):
        ops.lba_pyramid([x], [1] * (ops.LBA_MAX_LEVELS + 1))
    with pytest.raises(ValueError, match="kernel sizes"):
        ops.lba_pyramid([x], [65])                          # a level of 0 rows
    with pytest.raises(ValueError, match="kernel sizes"):
        ops.lba_pyramid([x], [4, 0])


def test_lba_pyramid_c_abi_rejects_bad_shapes_before_device_work():
    """nrgbd_lba_pyramid checks its arguments before any launch: 54 planes (> 5 + 3 MAX_V), 9 levels, a level of size 0."""
    import ctypes
    from neuralrgbd_amd import _lib, ops
    lib = _lib.load()
    fake = (ctypes.c_void_p * 64)(*([16] * 64))            # never dereferenced: the calls must return before a launch
    out = ctypes.c_void_p(16)

    def call(nplanes, H, W, ks):
        k = (ctypes.c_int * max(1, len(ks)))(*ks)
        return lib.nrgbd_lba_pyramid(fake, nplanes, H, W, k, len(ks), out, None)
    e_shape = call(5 + 3 * ops.MAX_V + 1, 64, 96, [4])
    assert e_shape == -2                                     # NRGBD_E_SHAPE
    assert call(1, 64, 96, [1] * (ops.LBA_MAX_LEVELS + 1)) == e_shape
    assert call(1, 64, 96, [65]) == e_shape                 # 64 // 65 = 0 rows
    assert call(1, 64, 96, [0]) == e_shape
    assert call(0, 64, 96, [2]) == e_shape
