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


def test_argument_errors_raise_before_device_work(scene, monkeypatch):
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
        with pytest.raises(ValueError, match="at most"):
            fn(ref_frame, src_frames * 5, dmap, conf, cams, [4, 2, 1], poses * 5, 3, 0.01, [1, 1])
        with pytest.raises(Exception, match="undefined optmization variable option"):
            fn(ref_frame, src_frames, dmap, conf, cams, [4, 2, 1], poses, 3, 0.01, [1, 2])
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
