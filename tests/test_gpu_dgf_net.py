"""KVNET(refineNet_name='DGF') on the GPU at the shape of the twin fixtures (256 x 256, D = 8), every comparison bit for bit:
the volumes against KVNET(if_refined=False) with the same weights, the refined maps against ops.dgf_refine on the regressed depth
(with the existing DPV parity and tests/test_gpu_dgf.py this is the end-to-end argument: no numeric gate against the reference's
end-to-end fp32 map is set, its guided filter cancels in fp32), and test_step.test / DepthStream (eager, hipGraph, pipelined) /
VideoDepthStream against a loop written out by hand."""
import math

import numpy as np
import pytest
import torch

import gen_dgf_golden as gg
import video_ref as vr
import neuralrgbd_amd
from neuralrgbd_amd import homography, misc, ops, synth, video
from neuralrgbd_amd._lib import NrgbdError
from neuralrgbd_amd.streaming import DepthStream
from neuralrgbd_amd.test_step import test as step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = gg.MODEL["r"]
H, W = gg.MODEL["H"], gg.MODEL["W"]
N_FRAMES = 2 * R + 5            # five windows: the first-frame branch, then four updates (the pipelined stream captures at the fifth)


def _models():
    m = gg.MODEL
    cam, d_candi = gg.model_setup()
    dgf = neuralrgbd_amd.KVNET(64, cam, d_candi, m["sigma"], 64, None, if_refined=True, refineNet_name="DGF", t_win_r=R)
    sd = synth.seeded_state_dict(dgf, m["weight_seed"])
    dgf.load_state_dict(sd)
    plain = neuralrgbd_amd.KVNET(64, cam, d_candi, m["sigma"], 64, None, if_refined=False, t_win_r=R)
    plain.load_state_dict({k: v for k, v in sd.items() if not k.startswith("r_net.")})
    return dgf.to(DEV), plain.to(DEV), cam, d_candi


def _predict(dpv, pose_next, cam, d_candi):
    inv = ops.pose_inverse(pose_next.to(dtype=torch.float32).contiguous())
    return homography.resample_vol_cuda(src_vol=dpv, rel_extM=inv, cam_intrinsic=cam, d_candi=d_candi,
                                        padding_value=math.log(1. / len(d_candi)), clamp=(-1000., 0.)).unsqueeze(0)


def _loop(model, cam, d_candi, windows):
    """KVNET.forward + PREDICT per window, written out: [(dmap_cur_refined, dmap_refined, BV_cur, DPV)] per window."""
    pred, outs = None, []
    with torch.no_grad():
        for ref, src, poses in windows:
            res = model(ref, src, poses, torch.zeros(1), cam_intrinsics=[cam], BV_predict=pred)
            outs.append(tuple(t.clone() if isinstance(t, torch.Tensor) else t for t in res))
            pred = _predict(res[3], poses[0, R], cam, d_candi)
    torch.cuda.synchronize()
    return outs


@pytest.fixture(scope="module")
def hand():
    frames = vr.noise_frames(931, N_FRAMES, H, W)
    images = [vr.normalise(f) for f in frames]
    extMs = vr.trajectory(932, N_FRAMES)
    loop = [(c, ref[None].to(DEV), torch.stack(src)[None].to(DEV), torch.from_numpy(poses)[None].to(DEV))
            for c, valid, ref, src, poses, _ in vr.driver_loop(images, extMs, R)]
    assert len(loop) == 5
    dgf, plain, cam, d_candi = _models()
    windows = [w[1:] for w in loop]
    return dict(frames=frames, extMs=extMs, index=[w[0] for w in loop], windows=windows, dgf=dgf, cam=cam, d_candi=d_candi,
                outs=_loop(dgf, cam, d_candi, windows), plain=_loop(plain, cam, d_candi, windows))


def test_volumes_equal_the_unrefined_model_and_maps_equal_the_kernel(hand):
    g = np.load(gg.model_path())
    net = hand["dgf"].r_net.feature_ext
    params = (net[0].weight, net[0].bias, net[2].weight, net[2].bias)
    for f, (got, plain, (ref, _, _)) in enumerate(zip(hand["outs"], hand["plain"], hand["windows"])):
        assert [",".join(str(n) for n in t.shape) for t in got] == [str(s) for s in g["shapes_f1" if f == 0 else "shapes_f2"]]
        assert plain[0] == -1 and plain[1] == -1
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
        assert torch.equal(got[2], plain[2]) and torch.equal(got[3], plain[3]), "frame %d: the volumes differ" % f
        with torch.no_grad():
            for refined, volume in ((got[0], got[2]), (got[1], got[3])):
                low = misc.depth_val_regression(volume, hand["d_candi"], BV_log=True)
                assert torch.equal(refined, ops.dgf_refine(low, ref, *params)), "frame %d: a refined map differs" % f
        if f == 0:
            assert torch.equal(got[0], got[1]) and torch.equal(got[2], got[3])
        else:
            assert not torch.equal(got[0], got[1])
    # the refined map is a depth map in metres: inside the candidates' range up to the filter's overshoot
    assert 0.0 < float(hand["outs"][-1][1].mean()) < 5.0


def test_test_step_returns_the_loop_maps(hand):
    pred = None
    for (ref, src, poses), want in zip(hand["windows"], hand["outs"]):
        dmap, pred = step(hand["dgf"], hand["d_candi"], [hand["cam"]], R, [{"img": ref}], [[{"img": src[0, v:v + 1]} for v in range(2 * R)]],
                          poses, pred, R_net=True)
        assert torch.equal(dmap, want[1])


@pytest.mark.parametrize("mode", ["eager", "graph", "pipeline"])
def test_depth_stream_returns_the_loop_maps(hand, mode):
    ds = DepthStream(hand["dgf"], hand["cam"], hand["d_candi"], t_win_r=R, use_graph=mode != "eager", copy_outputs=True,
                     pipeline=mode == "pipeline")
    outs = [ds.step(*w) for w in hand["windows"]]
    if mode == "pipeline":
        assert outs[1] is None
        outs = [outs[0]] + outs[2:] + [ds.flush()]
    torch.cuda.synchronize()
    ds.check()
    if mode != "eager":
        assert ds._graph is not None, ds.graph_error
    assert len(outs) == len(hand["outs"])
    for f, (got, want) in enumerate(zip(outs, hand["outs"])):
        assert torch.equal(got[0], want[1]) and torch.equal(got[1], want[3]), "frame %d" % f


def test_video_stream_returns_the_loop_maps(hand):
    vs = video.VideoDepthStream(hand["dgf"], hand["cam"], hand["d_candi"], t_win_r=R, copy_outputs=True, use_graph=True)
    returned = [vs.push(f, e) for f, e in zip(hand["frames"], hand["extMs"])]
    assert vs.flush() is None
    torch.cuda.synchronize()
    vs.check()
    got = {o[0]: o[1:] for o in returned if o is not None}
    assert sorted(got) == hand["index"]
    for c, want in zip(hand["index"], hand["outs"]):
        assert torch.equal(got[c][0], want[1]) and torch.equal(got[c][1], want[3]), "frame %d" % c


def test_frame_launches_no_kernel_of_another_library(hand):
    """Every kernel of an update frame of the DGF model is a kernel of the library (nrgbd::) or one the frame of the unrefined model
    launches as well."""
    from torch.profiler import ProfilerActivity, profile
    _, plain, cam, d_candi = _models()
    ref, src, poses = hand["windows"][1]
    pred = _predict(hand["outs"][0][3], hand["windows"][0][2][0, R], cam, d_candi)
    names = {}
    for key, model in (("plain", plain), ("dgf", hand["dgf"])):
        with torch.no_grad():
            model(ref, src, poses, torch.zeros(1), cam_intrinsics=[cam], BV_predict=pred, dpv_valid=True)       # caches warm
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                model(ref, src, poses, torch.zeros(1), cam_intrinsics=[cam], BV_predict=pred, dpv_valid=True)
                torch.cuda.synchronize()
        names[key] = {e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                      and "memset" not in e.name.lower()}
    assert any("dgf_refine_kernel" in n for n in names["dgf"]) and len(names["plain"]) > 5
    extra = sorted(n for n in names["dgf"] - names["plain"] if "nrgbd::" not in n)
    assert not extra, extra


def test_gradients_enabled_is_refused(hand):
    ref, src, poses = hand["windows"][0]
    with pytest.raises(NrgbdError, match="inference only"):
        hand["dgf"](ref, src, poses, torch.zeros(1), cam_intrinsics=[hand["cam"]], BV_predict=None)
