"""TrainVideoStream (neuralrgbd_amd/train_video.py) on the GPU against a hand-built loop: the loop calls train() / TrainGraph.step on
windows the comparator prepared on the CPU (tests/train_video_ref.py: real Pillow resizes, np.digitize, the reference's driver loop) and
uploaded, the stream gets raw uint8 frames, uint16 depth frames and extrinsics.  With deterministic=True the two runs must agree bit
for bit: losses, BV_predict, every state-dict tensor and every Adam moment.  The shape of tests/test_gpu_train_det.py: 256 x 256
images, D = 8, seeded state dict, FusedAdam."""
import numpy as np
import pytest
import torch

import neuralrgbd_amd
import train_video_ref as tr
import video_ref as vr
from neuralrgbd_amd import camera, synth
from neuralrgbd_amd.optim import FusedAdam
from neuralrgbd_amd.train_step import TrainGraph, train
from neuralrgbd_amd.train_video import TrainVideoStream, run_training_sequence

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R_WIN = 2
SHAPES = {"plain": dict(H=256, W=256, D=8, Hf=300, Wf=300, Hd=160, Wd=160, dup=False),
          "dup": dict(H=256, W=256, D=32, Hf=300, Wf=300, Hd=160, Wd=160, dup=True)}


def _setup(shape):
    s = SHAPES[shape]
    cam = camera.scannet_intrinsics(s["W"] // 4, s["H"] // 4)
    d_candi = np.linspace(0.1, 5, s["D"])
    return s, cam, d_candi


def _model(cam, d_candi, dup):
    kw = {"if_upsample_d": True} if dup else {}
    m = neuralrgbd_amd.KVNET(64, cam, d_candi, 10.0, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=R_WIN, **kw)
    m.load_state_dict(synth.seeded_state_dict(m, 0))
    return m.to(DEV)


def _state(model, opt):
    out = {"model." + k: v.detach().clone() for k, v in model.state_dict().items()}
    names = {p: n for n, p in model.named_parameters()}
    for p, st in opt.state.items():
        for key in ("exp_avg", "exp_avg_sq", "step"):
            if key in st and isinstance(st[key], torch.Tensor):
                out["adam.%s.%s" % (names[p], key)] = st[key].detach().clone()
    return out


def _assert_same(tag, a, b):
    assert list(a) == list(b), tag
    bad = [(k, int((a[k] != b[k]).sum()), a[k].numel()) for k in a if not torch.equal(a[k], b[k])]
    print("[train_video] %s: %d tensors compared, %d differ%s" % (tag, len(a), len(bad), "".join("\n      %s: %d of %d" % x for x in bad[:8])))
    assert not bad, "%s: first differing tensor %s (%d differ)" % (tag, bad[0][0], len(bad))


def _sequence(shape, n, seed, missing_depth=None, nan_pose=None):
    s, cam, d_candi = _setup(shape)
    frames, extMs = vr.noise_frames(seed, n, s["Hf"], s["Wf"]), vr.trajectory(seed + 1, n)
    depths = tr.depth_frames(seed + 2, n, s["Hd"], s["Wd"])
    if nan_pose is not None:
        extMs[nan_pose] = np.full((4, 4), np.nan)
    if missing_depth is not None:
        depths[missing_depth] = -1
    return frames, depths, extMs


def _hand_built(shape, frames, depths, extMs, use_graph):
    """The reference's driver loop over items prepared on the CPU; train() per valid window (TrainGraph.step for update-branch windows
    with use_graph).  Returns ({name: tensor} of losses and predictions, the final state, [(ref index, ran without BV_predict)])."""
    s, cam, d_candi = _setup(shape)
    H, W = s["H"], s["W"]
    full_key = "dmap_up4_imgsize_digit" if s["dup"] else "dmap_imgsize_digit"
    items = []
    for i, (f, d, e) in enumerate(zip(frames, depths, extMs)):
        lab = -1 if isinstance(d, int) else tr.prepare_depth(d, (H, W), (H // 4, W // 4), d_candi)
        items.append({"img": vr.normalise(vr.resize_nearest(f, H, W))[None], "dmap": lab if isinstance(lab, int) else lab["dmap"], "lab": lab,
                      "extM": e, "idx": i})
    model = _model(cam, d_candi, s["dup"])
    opt = FusedAdam(model.parameters(), lr=1e-4)
    tg = TrainGraph(model, opt, R_WIN, d_candi, cam, deterministic=True, refine_dup=s["dup"]) if use_graph else None
    trace, schedule, bv = {}, [], None
    for c, valid, first, poses, src_idx in tr.driver_loop(items, R_WIN):
        if not valid:
            continue
        ref = items[c]
        poses = torch.from_numpy(poses)[None].to(DEV)
        dmap, dmap_full = ref["lab"]["dmap"].to(DEV), ref["lab"][full_key].to(DEV)
        if tg is not None and not first:
            src = torch.stack([items[i]["img"][0] for i in src_idx])[None].to(DEV)
            loss, bv = tg.step(ref["img"].to(DEV), src, poses, dmap, dmap_full, bv)
        else:
            _, bv, loss, _, _ = train(1, model, opt, R_WIN, d_candi, [{"img": ref["img"].to(DEV), "dmap": dmap, full_key: dmap_full}],
                                      [[{"img": items[i]["img"].to(DEV)} for i in src_idx]], poses, None if first else bv, [cam],
                                      refine_dup=s["dup"], deterministic=True)
        trace["loss@%d" % c], trace["bv@%d" % c] = loss.clone(), bv.clone()
        schedule.append((c, first))
    torch.cuda.synchronize()
    return trace, _state(model, opt), schedule


def _streamed(shape, frames, depths, extMs, use_graph, device_inputs=False):
    s, cam, d_candi = _setup(shape)
    model = _model(cam, d_candi, s["dup"])
    opt = FusedAdam(model.parameters(), lr=1e-4)
    stream = TrainVideoStream(model, opt, cam, d_candi, t_win_r=R_WIN, use_graph=use_graph, refine_dup=s["dup"], deterministic=True)
    assert (stream.H, stream.W) == (s["H"], s["W"])
    if device_inputs:
        frames = [torch.from_numpy(f).to(DEV) for f in frames]
        depths = [d if isinstance(d, int) else torch.from_numpy(d).to(DEV) for d in depths]
    trace, schedule = {}, []
    for i, (f, d, e) in enumerate(zip(frames, depths, extMs)):
        was_first = stream.bv_predict is None
        out = stream.push(f, d, e)
        if out is None:
            continue
        c, loss = out[0], out[1]
        assert c == i - R_WIN and all(isinstance(t, torch.Tensor) and t.is_cuda for t in out[1:] if t is not None)
        if not (use_graph and not was_first):
            assert all(t is not None for t in out[2:]) and out[2].shape[1] == (4 if s["dup"] else 1) * s["D"]
        trace["loss@%d" % c], trace["bv@%d" % c] = loss.clone(), stream.bv_predict.clone()
        schedule.append((c, was_first))
    torch.cuda.synchronize()
    return trace, _state(model, opt), schedule, stream


def _compare(shape, frames, depths, extMs, use_graph, want_schedule, **kw):
    t1, s1, sched1 = _hand_built(shape, frames, depths, extMs, use_graph)
    t2, s2, sched2, stream = _streamed(shape, frames, depths, extMs, use_graph, **kw)
    assert sched1 == sched2 == want_schedule
    print("[train_video] %s graph=%s: losses %s" % (shape, use_graph, [float(v) for k, v in t1.items() if k.startswith("loss")]))
    assert all(bool(torch.isfinite(v).all()) for v in t1.values())
    _assert_same("losses and BV_predict", t1, t2)
    _assert_same("weights, BN statistics, Adam moments", s1, s2)
    n_adam = sum(1 for k in s1 if k.endswith(".exp_avg"))
    assert n_adam == len(list(stream.model.parameters()))
    return stream


def test_image_sizes_are_where_the_integer_rule_is_pillows():
    """The uint8 frame ingest keeps the integer rule; the frames of this file are resized at pairs where it equals Pillow."""
    assert np.array_equal(tr.integer_nearest_index(300, 256), tr.pil_nearest_index(300, 256))


@pytest.mark.parametrize("use_graph", [False, True])
def test_stream_equals_the_hand_built_loop(use_graph):
    frames, depths, extMs = _sequence("plain", 8, 11)
    stream = _compare("plain", frames, depths, extMs, use_graph, [(2, True), (3, False), (4, False), (5, False)], device_inputs=use_graph)
    if use_graph:
        assert stream.graph._graph is not None                         # eager warm-up, then capture: the last two windows replayed


@pytest.mark.parametrize("kind,bad,n,want", [("depth", 4, 11, [(7, True), (8, False)]), ("pose", 4, 11, [(7, True), (8, False)]),
                                             ("pose", 6, 13, [(2, True), (3, False), (9, True), (10, False)])])
def test_invalid_windows_are_skipped_and_the_next_starts_over(kind, bad, n, want):
    frames, depths, extMs = _sequence("plain", n, 23, **({"missing_depth": bad} if kind == "depth" else {"nan_pose": bad}))
    _compare("plain", frames, depths, extMs, False, want)


def test_refine_dup_stream_equals_the_hand_built_loop():
    """KVNET(if_upsample_d=True), D = 32: the image-size label is dmap_up4_imgsize_digit (128 bins).  At 256 x 256 images, the shape
    of tests/test_gpu_rnet_dup.py (the feature CNN does not take 64 x 64 images); a first-frame and an update-branch step."""
    frames, depths, extMs = _sequence("dup", 6, 31)
    stream = _compare("dup", frames, depths, extMs, False, [(2, True), (3, False)])
    assert stream.labeler.full_key == "dmap_up4_imgsize_digit" and int(stream.labels_full.max()) > 31


def test_reset_and_generator_form():
    frames, depths, extMs = _sequence("plain", 6, 41)
    s, cam, d_candi = _setup("plain")
    model = _model(cam, d_candi, False)
    stream = TrainVideoStream(model, FusedAdam(model.parameters(), lr=1e-4), cam, d_candi, t_win_r=R_WIN, deterministic=True)
    outs = list(run_training_sequence(stream, frames, depths, extMs))
    assert [o[0] for o in outs] == [2, 3] and stream.bv_predict is not None
    stream.reset()
    assert stream.bv_predict is None and stream.n_pushed == 0
    assert all(stream.push(f, d, e) is None for f, d, e in zip(frames[:4], depths[:4], extMs[:4]))
