"""Oracle vs the reference's own outputs on fresh seeds and shapes beyond the other golden vectors: the reference's functions
were run once on these inputs by oracle/gen_golden.py live, which stored inputs and outputs in tests/golden/ref_live.npz
(and the D = 64 state-dict keys in tests/golden/state_keys_D64.json)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, report
from neuralrgbd_amd import camera
from oracle import cpu_oracle as co
from oracle.gen_golden import LIVE_OPS_SHAPES, LIVE_PREDICT_SUB, LIVE_RAY_GRIDS, checksum


@pytest.fixture(scope="module")
def live():
    return dict(np.load(os.path.join(GOLDEN, "ref_live.npz")))


@pytest.mark.parametrize("h,w,D,V,C,seed", list(LIVE_OPS_SHAPES))
def test_ops_fresh_shapes(h, w, D, V, C, seed, live):
    p = "ops%d_" % LIVE_OPS_SHAPES.index((h, w, D, V, C, seed))
    cam = camera.scannet_intrinsics(w, h)
    rng = np.random.RandomState(seed)
    feat_ref = torch.from_numpy(rng.standard_normal((1, C, h, w)).astype(np.float32))
    feat_src = torch.from_numpy(rng.standard_normal((1, V, C, h, w)).astype(np.float32))
    want_sum = float(live[p + "feat_checksum"])
    assert abs(checksum([feat_ref, feat_src]) - want_sum) < 1e-6 * want_sum      # the features the reference was run on
    poses = torch.from_numpy(live[p + "poses"])
    d_candi = np.linspace(0.3, 8, D)
    R, t = poses[:, :3, :3].contiguous(), poses[:, :3, 3].contiguous()
    want = live[p + "cost"]
    K = cam["intrinsic_M_cuda"]
    KR = torch.stack([K.matmul(R[v]) for v in range(V)]).reshape(V, 9).numpy()
    Kt = torch.stack([K.matmul(t[v]) for v in range(V)]).numpy()
    got = co.costvol(feat_ref[0].numpy(), feat_src[0].numpy(), KR, Kt, cam["unit_ray_array_2D"].numpy(), d_candi,
                     cam["intrinsic_M"][0, 2], cam["intrinsic_M"][1, 2], 3.0)
    mx, _, _ = report("oracle vs ref costvol", -got, -want)
    assert mx < 1e-4 * max(1.0, float(np.abs(want).max()))

    dpv, T = live[p + "dpv"], live[p + "T"]
    pad = math.log(1. / D)
    want = live[p + "pred"]
    got = co.dpv_resample(dpv, T, cam["unit_ray_array_2D"].numpy(), d_candi,
                          math.tan(math.radians(cam["hfov"]) * .5), math.tan(math.radians(cam["vfov"]) * .5), pad)
    assert np.array_equal(got, want)


def test_camera_dict_matches_reference_loop(live):
    for (w, h) in LIVE_RAY_GRIDS:
        cam = camera.scannet_intrinsics(w, h)
        rays = live["rays_%dx%d" % (w, h)]
        assert np.array_equal(rays, cam["unit_ray_array"])


def test_state_dict_keys_match_live_reference():
    import neuralrgbd_amd
    cam = camera.scannet_intrinsics(96, 64)
    d = np.linspace(.1, 5, 64)
    mine = neuralrgbd_amd.KVNET(64, cam, d, 10., 64, None, if_refined=True, refineNet_name="DPV", t_win_r=2)
    with open(os.path.join(GOLDEN, "state_keys_D64.json")) as f:
        a = {k: tuple(v) for k, v in json.load(f).items()}
    b = {k: tuple(v.shape) for k, v in mine.state_dict().items()}
    assert a == b and len(a) == 459


def test_homography_terms_order_is_what_torch_cpu_executes_here(live):
    """oracle_homography_terms / csrc/geom.hip write out the order torch's CPU kernels used for IntM.matmul(R_v) and
    IntM.matmul(t_v) where the golden vectors were generated (their products are stored in ref_live.npz).  Other hosts' BLAS
    kernels may order a K=3 contraction differently (the MI355X node's does), which is why the order is pinned in code rather
    than delegated."""
    cam = camera.scannet_intrinsics(96, 64)
    K = cam["intrinsic_M_cuda"]
    for n in range(50):
        poses = live["hterms_poses"][n]
        KR, Kt = co.homography_terms(K.numpy(), poses[:, :3, :3], poses[:, :3, 3])
        want_KR, want_Kt = live["hterms_KR"][n], live["hterms_Kt"][n]
        assert np.array_equal(KR, want_KR) and np.array_equal(Kt, want_Kt)


def test_pose_inverse_vs_live_reference_inverse(live):
    """test_utils/test_KVNet.py:50 `Src_CamPoses[ibatch, t_win_r].inverse()` runs on the host LAPACK (MKL sgetrf + sgetrs of
    the transposed matrix under torch 2.10: its LU is reproducible — right-looking fma chain, reciprocal scaling — its
    triangular solves are not), so unlike K.R_v it cannot be pinned bit for bit.  What is pinned: the path's inverse
    (oracle_pose_inverse == nrgbd_pose_inverse, fp64 Gauss-Jordan rounded to fp32) is within the reference's OWN rounding
    error of the reference's result, and closer to the exact inverse than the reference is.  The reference's inverses are the
    ones torch computed where the golden vectors were generated (ref_live.npz)."""
    worst_ours, worst_ref, worst_gap = 0.0, 0.0, 0.0
    for T, ref in zip(live["inv_poses"], live["inv_ref"]):
        ours = co.pose_inverse(T)
        ex = np.linalg.inv(T.astype(np.float64))
        e_ref, e_ours = np.abs(ref - ex).max(), np.abs(ours - ex).max()
        worst_ours, worst_ref = max(worst_ours, e_ours), max(worst_ref, e_ref)
        worst_gap = max(worst_gap, np.abs(ours - ref).max())
        assert np.abs(ours - ref).max() <= e_ref + e_ours + 1e-12
    print("[parity] pose inverse: |ours - exact| max %.2e, |reference - exact| max %.2e, |ours - reference| max %.2e" %
          (worst_ours, worst_ref, worst_gap))
    assert worst_ours <= worst_ref and worst_gap < 4e-6


def test_predict_with_path_inverse_vs_live_reference_predict(live):
    """The whole PREDICT step (inverse + resample + clamp) of the oracle against the reference's, on a peaked DPV: the two
    differ ONLY through the last bits of the inverse (the resample itself is bit-identical given T, test_ops_fresh_shapes).
    Mean stays far below 1e-4; the max is the DPV's slope times ~1e-7 of coordinate and is printed.
    The reference's whole output volume is rebuilt from the inverse it used (its resample = the oracle's given the matrix) and
    must reproduce the reference's own stored output at every LIVE_PREDICT_SUB-th pixel before the gates are applied to it."""
    h, w, D = 48, 64, 64
    cam = camera.scannet_intrinsics(w, h)
    d_candi = np.linspace(0.1, 5, D)
    rng = np.random.RandomState(31)
    dpv = torch.log_softmax(torch.from_numpy(rng.standard_normal((1, D, h, w)).astype(np.float32)) * 6, 1)[0].numpy()
    assert abs(dpv.astype(np.float64).sum() - float(live["predict_dpv_sum"])) < 1e-6 * abs(float(live["predict_dpv_sum"]))
    pad = math.log(1. / D)
    rays, tx, ty = cam["unit_ray_array_2D"].numpy(), math.tan(math.radians(cam["hfov"]) * .5), math.tan(math.radians(cam["vfov"]) * .5)
    worst = 0.0
    st = LIVE_PREDICT_SUB
    for pose, inv_ref, want_sub in zip(live["predict_poses"], live["predict_inv_ref"], live["predict_ref_sub"]):
        want = co.dpv_resample(dpv, inv_ref, rays, d_candi, tx, ty, pad)
        assert want.shape == (D, h, w)
        assert np.all(np.abs(want[:, ::st, ::st] - want_sub) <= 1e-6 * np.maximum(1.0, np.abs(want_sub)))
        got = co.dpv_resample(dpv, co.pose_inverse(pose), rays, d_candi, tx, ty, pad)
        mx, mean, _ = report("oracle PREDICT (own inverse) vs ref", got, want)
        worst = max(worst, mx)
        assert mean < 1e-4 and mx < 2e-2


def test_resample_with_new_candidates_vs_live_reference(live):
    """resample_vol_cuda(..., d_candi_new=...) — the LBA driver's form (test_KVNet_LBA.py:414-417): output planes at the NEW
    candidates, z normalised by the source candidates' float64 range.  Bit-identical like the d_candi_new=None form."""
    h, w, D, Dn = 20, 28, 12, 9
    cam = camera.scannet_intrinsics(w, h)
    d_candi, d_new = np.linspace(0.3, 8, D), np.linspace(0.5, 6.5, Dn)
    dpv, T = live["newcand_dpv"], live["newcand_T"]
    pad = math.log(1. / D)
    want = live["newcand_new"]
    # the reference allocates D point planes and fills the first Dn: the rest sample the origin (d = 0)
    d_pad = np.concatenate([d_new, np.zeros(D - Dn)])
    got = co.dpv_resample(dpv, T, cam["unit_ray_array_2D"].numpy(), d_candi,
                          math.tan(math.radians(cam["hfov"]) * .5), math.tan(math.radians(cam["vfov"]) * .5), pad,
                          clamp=None, d_candi_new=d_pad)
    assert got.shape == (D, h, w) and np.array_equal(got, want)
    # the LBA call itself: d_candi_new = d_candi (same planes, but the float64 z range)
    want = live["newcand_same"]
    got = co.dpv_resample(dpv, T, cam["unit_ray_array_2D"].numpy(), d_candi,
                          math.tan(math.radians(cam["hfov"]) * .5), math.tan(math.radians(cam["vfov"]) * .5), pad,
                          clamp=None, d_candi_new=d_candi)
    assert np.array_equal(got, want)


def test_oracle_on_a_static_window_vs_live_reference():
    """A camera standing still: five identical images (ordinary poses, so depth is defined).  The SPP 64-window BatchNorm then sees
    five equal values per channel.  The oracle's feature CNN and two frames of step() against the UNMODIFIED reference run here
    (oracle/ref_shim.py), with the gates of test_oracle_golden.py::test_whole_path_two_frames (the path's own pose inverse): the
    checker of tests/test_gpu_static_window.py is valid on such windows, and the reference's outputs there are finite."""
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip("the unmodified reference is not present on this machine")
    from neuralrgbd_amd import synth
    from oracle import gen_golden
    from oracle import kvnet_oracle as ko
    ref = ref_shim.load()
    H, W, D = 256, 256, 16
    cam = camera.scannet_intrinsics(W // 4, H // 4)
    d_candi = np.linspace(0.1, 5.0, D)
    with ref_shim.quiet():
        model = ref.KVNET.KVNET(64, cam, d_candi, 10.0, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=2)
    sd = synth.seeded_state_dict(model, 0)
    model.load_state_dict(sd)
    rng = np.random.RandomState(11)
    img = torch.from_numpy(synth.smooth_texture(rng, 3, H, W))[None]
    src = img[None].expand(1, 4, 3, H, W).contiguous()
    poses = torch.from_numpy(synth.random_poses(rng, 4)[None])
    x = torch.cat((src[0], img), 0)
    with torch.no_grad():
        l1_ref, f_ref = model.feature_extractor(x)
        l1_o, f_o = ko.feature_cnn(sd, "feature_extractor.feature_extraction", x)
    assert torch.isfinite(f_ref).all()
    for name, got, want in (("layer1", l1_o, l1_ref), ("feature", f_o, f_ref)):
        mx, _, _ = report("static window oracle vs reference " + name, got.numpy(), want.numpy())
        assert mx < 1e-4 * max(1.0, float(want.abs().max()))
    (dpv1, pred1, _), (dpv2, pred2, _) = gen_golden.run_stream(ref, model, cam, d_candi, [(img, src, poses)] * 2)
    o1 = ko.step(sd, img, src, poses, cam, d_candi, 10.0, None)
    o2 = ko.step(sd, img, src, poses, cam, d_candi, 10.0, o1[3])
    for name, got, want, tol in (("BV_cur f1", o1[2], dpv1, 2e-4), ("BV_predict f1", o1[3], pred1, 1e-3), ("DPV f2", o2[1], dpv2, 1e-3),
                                 ("BV_predict f2", o2[3], pred2, 1e-3)):
        assert torch.isfinite(want).all(), name
        mx, mean, _ = report("static window oracle vs reference " + name, got[0].numpy(), want[0].numpy())
        assert mx < tol and mean < 1e-4, name
    assert (o1[2][0].argmax(0) != dpv1[0].argmax(0)).sum() == 0
    assert (o2[1][0].argmax(0) != dpv2[0].argmax(0)).sum() == 0
