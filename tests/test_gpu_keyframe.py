"""nrgbd_dpv_keyframe_maps (keyframe.hip) against the composition it replaces, bit for bit: the LBA driver's
resample_vol_cuda(..., d_candi_new=d_candi).clamp(-1000, 0) -> depth_val_regression / exp(max) ** 2 (test_KVNet_LBA.py:414-423,
:455, :495) on this path's own operators.  No tolerance anywhere: the fused kernel samples with resample.hip's own body
(resample.hpp), adds the candidates in depth_regress_kernel's order and squares export_depth_u16's exponential."""
import math

import numpy as np
import pytest
import torch

from neuralrgbd_amd import camera, homography, lba_step, misc, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _motion(kind):
    T = np.eye(4)
    if kind == "small":
        T[:3, :3] = synth.rotvec_to_R([0.01, -0.02, 0.005])
        T[:3, 3] = [0.03, -0.02, 0.05]
    elif kind == "outside":          # a third of the grid leaves the source frustum: border taps, clipped coordinates
        T[:3, :3] = synth.rotvec_to_R([0.05, 0.35, -0.1])
        T[:3, 3] = [0.4, -0.3, 0.6]
    elif kind == "behind":           # the candidates nearer than 1.5 end up behind the source camera (z <= 0)
        T[:3, :3] = synth.rotvec_to_R([0.0, 0.1, 0.0])
        T[:3, 3] = [0.0, 0.0, 1.5]
    else:
        assert kind == "identity"
    return torch.from_numpy(T.astype(np.float32))


def _volume(D, H, W, seed, kind="peaked"):
    g = torch.Generator().manual_seed(seed)
    logits = 4.0 * torch.randn(D, H, W, generator=g)
    bv = torch.log_softmax(logits, 0)
    if kind == "floor":              # entries at the clamp's lower bound (an invalidated region) and below it
        bv[:, : H // 2, : W // 3] = -1000.0
        bv[D // 2, H // 2:, :] = -1200.0
    elif kind == "ties":             # the maximum is reached by several candidates, in different parts of the 4-way split
        bv[:] = torch.minimum(bv, torch.tensor(-3.0))
        bv[1::3] = -0.5
    return bv.contiguous()


def _composition(bv, T, cam, d_candi, d_candi_new):
    """(dmap_ref, conf_ref, dmap_kf, conf_kf) from the separate operators, as the reference driver composes them."""
    D = bv.shape[0]
    pad = math.log(1. / float(D))
    res = homography.resample_vol_cuda(bv[None], T, cam_intrinsic=cam, d_candi=d_candi, d_candi_new=d_candi_new,
                                       padding_value=pad, clamp=(-1000., 0.))
    d_out = np.concatenate([np.asarray(d_candi_new, np.float64), np.zeros(D - len(d_candi_new))])
    dmap_kf = misc.depth_val_regression(res.unsqueeze(0), d_out)[0]
    c = ops.export_depth_u16(res, homography._d_candi_dev(d_out, res.device))[1]
    dmap_ref = misc.depth_val_regression(bv[None], d_candi)[0]
    c_ref = ops.export_depth_u16(bv, homography._d_candi_dev(d_candi, bv.device))[1]
    return dmap_ref, c_ref * c_ref, dmap_kf, c * c, res


def _equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


SIZES = [(7, 9), (64, 96), (256, 384), (480, 640)]


@pytest.mark.parametrize("D", [8, 64, 128])
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("motion", ["identity", "small", "outside", "behind"])
def test_maps_equal_the_composition_bit_for_bit(D, H, W, motion):
    cam = camera.scannet_intrinsics(W, H)
    d_candi = np.linspace(0.5, 5.0, D)
    bv = _volume(D, H, W, 3 + D + H).to(DEV)
    pose_next = _motion(motion)
    T = ops.pose_inverse(pose_next.to(DEV))
    want = _composition(bv, T, cam, d_candi, d_candi)
    got = lba_step.keyframe_maps(bv[None], pose_next, cam, d_candi)
    for name, g, w_ in zip(("dmap_ref", "conf_ref", "dmap_kf", "conf_kf"), got, want):
        assert g.shape == (H, W)
        assert _equal(g, w_), "%s differs: max|d| = %g" % (name, float((g - w_).abs().max()))
    if motion in ("outside", "behind"):
        # the case exercises what it names: a good part of the samples lands on the bordered faces (value pad)
        assert float(((want[4] - math.log(1. / D)).abs() < 1e-5).float().mean()) > 0.05


@pytest.mark.parametrize("kind", ["floor", "ties"])
@pytest.mark.parametrize("H,W", [(7, 9), (64, 96)])
def test_floor_entries_and_tied_maxima(kind, H, W):
    D = 64
    cam = camera.scannet_intrinsics(W, H)
    d_candi = np.linspace(0.5, 5.0, D)
    bv = _volume(D, H, W, 11, kind).to(DEV)
    pose_next = _motion("small")
    want = _composition(bv, ops.pose_inverse(pose_next.to(DEV)), cam, d_candi, d_candi)
    got = lba_step.keyframe_maps(bv[None], pose_next, cam, d_candi)
    for name, g, w_ in zip(("dmap_ref", "conf_ref", "dmap_kf", "conf_kf"), got, want):
        assert _equal(g, w_), name


@pytest.mark.parametrize("H,W,D,Dn", [(64, 96, 64, 40), (7, 9, 8, 3), (256, 384, 128, 127)])
def test_fewer_new_candidates_than_planes(H, W, D, Dn):
    """resample_vol_cuda pads the new candidates with zeros to the volume's D planes (the reference leaves those point planes at
    the origin): the kernel gets the padded list, as homography.resample_vol_cuda passes it to nrgbd_dpv_resample_to."""
    cam = camera.scannet_intrinsics(W, H)
    d_candi = np.linspace(0.5, 5.0, D)
    d_new = np.linspace(0.7, 3.0, Dn)
    bv = _volume(D, H, W, 17).to(DEV)
    T = ops.pose_inverse(_motion("small").to(DEV))
    want = _composition(bv, T, cam, d_candi, d_new)
    d_out = homography._d_candi_dev(np.concatenate([d_new, np.zeros(D - Dn)]), DEV)
    z_half, z_radius = homography.z_range_f64(d_candi)
    _, rays = homography._cam_dev(cam, DEV)
    got = ops.dpv_keyframe_maps(bv, T, rays, d_out, homography._d_candi_dev(d_candi, DEV),
                                math.tan(math.radians(cam['hfov']) * .5), math.tan(math.radians(cam['vfov']) * .5),
                                z_half, z_radius, math.log(1. / D))
    for name, g, w_ in zip(("dmap_ref", "conf_ref", "dmap_kf", "conf_kf"), got, want):
        assert _equal(g, w_), name
    # a SHORTER output list (D_out < D_src at the C-ABI): the first Dn planes alone
    res = ops.dpv_resample(bv, T, rays, d_out[:Dn].contiguous(), math.tan(math.radians(cam['hfov']) * .5),
                           math.tan(math.radians(cam['vfov']) * .5), z_half, z_radius, math.log(1. / D), new_candi=True)
    got = ops.dpv_keyframe_maps(bv, T, rays, d_out[:Dn].contiguous(), None, math.tan(math.radians(cam['hfov']) * .5),
                                math.tan(math.radians(cam['vfov']) * .5), z_half, z_radius, math.log(1. / D), want_ref=False)
    assert got[0] is None and got[1] is None
    assert _equal(got[2], ops.depth_regress(res, d_out[:Dn].contiguous(), want_conf=False)[0])
    c = ops.export_depth_u16(res, d_out[:Dn].contiguous())[1]
    assert _equal(got[3], c * c)


def test_want_ref_false_leaves_the_reference_outputs_untouched():
    H, W, D = 64, 96, 64
    cam = camera.scannet_intrinsics(W, H)
    d_candi = np.linspace(0.5, 5.0, D)
    bv = _volume(D, H, W, 5).to(DEV)
    full = lba_step.keyframe_maps(bv[None], _motion("small"), cam, d_candi)
    out = tuple(torch.full((H, W), -7.0, device=DEV) for _ in range(4))
    got = lba_step.keyframe_maps(bv[None], _motion("small"), cam, d_candi, want_ref=False, out=out)
    torch.cuda.synchronize()
    assert got[0] is out[0] and got[2] is out[2]
    assert bool((out[0] == -7.0).all()) and bool((out[1] == -7.0).all())
    assert _equal(out[2], full[2]) and _equal(out[3], full[3])
    none = lba_step.keyframe_maps(bv[None], _motion("small"), cam, d_candi, want_ref=False)
    assert none[0] is None and none[1] is None and _equal(none[2], full[2])


def test_argument_checks():
    from neuralrgbd_amd import _lib
    H, W, D = 8, 8, 8
    cam = camera.scannet_intrinsics(W, H)
    bv = _volume(D, H, W, 1)
    with pytest.raises(_lib.NrgbdError):
        lba_step.keyframe_maps(bv[None], _motion("small"), cam, np.linspace(1, 2, D))      # CPU volume: no fallback
    with pytest.raises(ValueError):
        lba_step.keyframe_maps(bv[None].to(DEV), _motion("small"), cam, np.linspace(1, 2, D + 1))
    lib = _lib.load()
    z = ops._p(None)
    assert lib.nrgbd_dpv_keyframe_maps(z, z, z, z, z, 1., 1., 1., 1., 0., 0, 0., 0., z, z, z, z, D, D, H, W, z) == -1
    p = ops._p(bv.to(DEV))
    assert lib.nrgbd_dpv_keyframe_maps(p, p, p, p, p, 1., 1., 1., 1., 0., 0, 0., 0., p, p, p, p, 0, D, H, W, z) == -2


def test_capture_and_replay_give_the_same_bits():
    H, W, D = 64, 96, 64
    cam = camera.scannet_intrinsics(W, H)
    d_candi = np.linspace(0.5, 5.0, D)
    bv = _volume(D, H, W, 23).to(DEV)
    pose = _motion("small").to(DEV)
    eager = lba_step.keyframe_maps(bv[None], pose, cam, d_candi)
    st_bv, st_pose = bv.clone(), pose.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = lba_step.keyframe_maps(st_bv[None], st_pose, cam, d_candi)
    for o in out:
        o.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    for e, o in zip(eager, out):
        assert _equal(e, o)
    # new inputs through the static buffers: the pose is read from device memory at replay time
    bv2, pose2 = _volume(D, H, W, 24).to(DEV), _motion("outside").to(DEV)
    st_bv.copy_(bv2); st_pose.copy_(pose2)
    g.replay()
    torch.cuda.synchronize()
    for e, o in zip(lba_step.keyframe_maps(bv2[None], pose2, cam, d_candi), out):
        assert _equal(e, o)
