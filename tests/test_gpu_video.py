"""The video stream on the GPU (neuralrgbd_amd/video.py, csrc/ingest.hip), every comparison bit for bit: nrgbd_frame_ingest_u8 against
ToTensor + Normalize on the CPU (every byte value, row tails, padded rows, both layouts, the integer nearest resize, a slot between
sentinels), nrgbd_window_gather against torch.stack, and VideoDepthStream against a DepthStream fed by the reference's driver loop
written out on the host (tests/video_ref.py) — eager, hipGraph, pipelined, across a NaN pose, from uint8 and from prepared fp32
frames.  The model is the small one of tests/test_gpu_twin.py (256 x 256: the smallest image the SPP branch takes)."""
import numpy as np
import pytest
import torch

import gen_twin_golden as gt
import video_ref as vr
import neuralrgbd_amd
from neuralrgbd_amd import ops, synth, video
from neuralrgbd_amd._lib import NrgbdError
from neuralrgbd_amd.streaming import DepthStream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.5


# ---- 1. frame ingest ------------------------------------------------------------------------------------------------------------

def _device_frame(hwc, layout, extra_pitch):
    """The uint8 frame on the device as the wrapper takes it: interleaved or planar, rows `extra_pitch` bytes longer than needed."""
    Hin, Win, _ = hwc.shape
    rows = hwc.reshape(Hin, 3 * Win) if layout == "hwc" else hwc.transpose(2, 0, 1).reshape(3 * Hin, Win)
    buf = np.full((rows.shape[0], rows.shape[1] + extra_pitch), 201, np.uint8)
    buf[:, :rows.shape[1]] = rows
    t = torch.from_numpy(buf).to(DEV)[:, :rows.shape[1]]
    return t.unflatten(1, (Win, 3)) if layout == "hwc" else t.unflatten(0, (3, Hin))


def _ingest_between_sentinels(hwc, Hout, Wout, layout, extra_pitch=0, mean=vr.MEAN, std=vr.STD):
    """Ingest into the middle slot of a three-slot ring whose every other float holds a sentinel; returns the slot (CPU)."""
    n = 3 * Hout * Wout
    stride = (n + 3) // 4 * 4 + 4                                   # a gap behind every slot
    buf = torch.full((3 * stride,), SENTINEL, device=DEV)
    slot = buf[stride:stride + n].view(3, Hout, Wout)
    frame = _device_frame(hwc, layout, extra_pitch)
    assert frame.is_contiguous() == (extra_pitch == 0)
    assert ops.frame_ingest(frame, slot, mean, std, layout) is slot
    torch.cuda.synchronize()
    out = buf.cpu()
    assert bool((out[:stride] == SENTINEL).all()) and bool((out[stride + n:] == SENTINEL).all()), "a neighbour of the slot was written"
    return out[stride:stride + n].view(3, Hout, Wout)


def _all_bytes_frame():
    u = np.arange(256, dtype=np.uint8)
    return np.stack((u, u[::-1], np.roll(u, 77)), axis=-1).reshape(16, 16, 3)


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("extra_pitch", [0, 5])
@pytest.mark.parametrize("H,W", [(16, 16), (5, 7), (33, 50), (64, 96)])
def test_ingest_is_totensor_normalize(H, W, extra_pitch, layout):
    hwc = _all_bytes_frame() if (H, W) == (16, 16) else vr.noise_frames(H * W, 1, H, W)[0]
    got = _ingest_between_sentinels(hwc, H, W, layout, extra_pitch)
    assert torch.equal(got, vr.normalise(hwc))
    other = ((0.1, 0.55, 0.9), (0.31, 1.7, 0.052))                  # custom statistics
    assert torch.equal(_ingest_between_sentinels(hwc, H, W, layout, extra_pitch, *other), vr.normalise(hwc, *other))


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("size_in,size_out", [((13, 17), (5, 7)), ((7, 5), (13, 17)), ((121, 162), (64, 96))])       # (H, W)
def test_ingest_resizes_nearest_by_the_integer_rule(size_in, size_out, layout):
    hwc = vr.noise_frames(size_in[0], 1, *size_in)[0]
    want = vr.normalise(vr.resize_nearest(hwc, *size_out))
    assert torch.equal(_ingest_between_sentinels(hwc, size_out[0], size_out[1], layout), want)
    assert torch.equal(_ingest_between_sentinels(hwc, size_out[0], size_out[1], layout, 5), want)


def test_ingest_wrapper_refusals_on_the_device():
    ring = torch.zeros(2, 3, 5, 7, device=DEV)                      # 105 floats per slot: slot 1 starts 4 bytes off a 16-byte word
    u8 = torch.zeros(5, 7, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(NrgbdError, match="code -3"):
        ops.frame_ingest(u8, ring[1], vr.MEAN, vr.STD)
    with pytest.raises(NrgbdError, match="code -4"):
        ops.frame_ingest(u8, ring[0], vr.MEAN, (0.2, 0.0, 0.2))
    with pytest.raises(ValueError):
        ops.frame_ingest(u8, ring[0], vr.MEAN, vr.STD, layout="chw")
    with pytest.raises(TypeError):
        ops.frame_ingest(u8.float(), ring[0], vr.MEAN, vr.STD)
    torch.cuda.synchronize()
    assert not ring.any()


# ---- 2. window gather -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,pad", [(8, 12, 0), (8, 12, 2), (5, 7, 3), (5, 7, 0)])      # 16 bytes per lane; the rest: one element per lane
@pytest.mark.parametrize("r", [1, 2, 3])
def test_gather_is_torch_stack(r, H, W, pad):
    R, n = 2 * r + 1, 3 * H * W
    buf = torch.randn(R * (n + pad), device=DEV)
    ring = buf.as_strided((R, 3, H, W), (n + pad, H * W, W, 1))
    for pushed in range(R, 2 * R + 1):                               # every rotation of the ring, wrapped ones included
        src_slots, ref_slot, _ = video.window_slots(pushed, r)
        src = torch.full((1, 2 * r, 3, H, W), SENTINEL, device=DEV)
        ref = torch.full((1, 3, H, W), SENTINEL, device=DEV)
        ops.window_gather(ring, src_slots + [ref_slot], src, ref)
        assert torch.equal(src[0], torch.stack([ring[s] for s in src_slots])) and torch.equal(ref[0], ring[ref_slot])
    a, b = ops.window_gather(ring, src_slots + [ref_slot])           # outputs of its own
    assert torch.equal(a, src[0]) and torch.equal(b, ref[0])
    with pytest.raises(ValueError):
        ops.window_gather(ring, [0] * (2 * r) + [R])


# ---- 3. the stream against the hand-built loop ----------------------------------------------------------------------------------

H, W = gt.TWIN["H"], gt.TWIN["W"]
FRAME_SIZE = {1: (H, W), 2: (300, 281)}           # r = 2: camera frames of another size, resized on the way in


def _model(r):
    cam, d_candi = gt.setup()
    m = neuralrgbd_amd.KVNET(64, cam, d_candi, gt.TWIN["sigma"], 64, None, if_refined=True, refineNet_name="DPV", t_win_r=r)
    m.load_state_dict(synth.seeded_state_dict(m, gt.TWIN["weight_seed"]))
    return m.to(DEV), cam, d_candi


def _sequence(r):
    n = 2 * r + 5
    frames = vr.noise_frames(900 + r, n, *FRAME_SIZE[r])
    images = [vr.normalise(vr.resize_nearest(f, H, W)) for f in frames]
    return frames, images, vr.trajectory(910 + r, n)


def _hand_built(r, images, extMs):
    """{reference index: (refined, dpv)} of an eager DepthStream over the windows of the reference's loop, assembled in torch."""
    model, cam, d_candi = _model(r)
    ds = DepthStream(model, cam, d_candi, t_win_r=r, use_graph=False, copy_outputs=True)
    outs = {}
    for c, valid, ref, src, poses, _ in vr.driver_loop(images, extMs, r):
        if not valid:
            ds.reset()
            continue
        o = ds.step(ref[None].to(DEV), torch.stack(src)[None].to(DEV), torch.from_numpy(poses)[None].to(DEV))
        outs[c] = (o[0].clone(), o[1].clone())
    torch.cuda.synchronize()
    ds.check()
    return outs


@pytest.fixture(scope="module", params=[1, 2])
def hand(request):
    r = request.param
    frames, images, extMs = _sequence(r)
    return r, frames, images, extMs, _hand_built(r, images, extMs)


def _as_pushed(frame, i):
    """The accepted uint8 forms in turn: host numpy HWC, device tensor CHW, host tensor HWC, device tensor HWC."""
    t = torch.from_numpy(frame)
    return [frame, t.permute(2, 0, 1).contiguous().to(DEV), t, t.to(DEV)][i % 4]


def _video(r, frames, extMs, **kw):
    model, cam, d_candi = _model(r)
    vs = video.VideoDepthStream(model, cam, d_candi, t_win_r=r, copy_outputs=True, **kw)
    assert (vs.H, vs.W) == (H, W)
    returned = [vs.push(f, e) for f, e in zip(frames, extMs)]
    last = vs.flush()
    torch.cuda.synchronize()
    vs.check()
    return vs, returned, last


def _same(outs, want):
    assert sorted(outs) == sorted(want)
    for c in want:
        assert torch.isfinite(outs[c][0]).all() and torch.isfinite(outs[c][1]).all()
        assert torch.equal(outs[c][0], want[c][0]) and torch.equal(outs[c][1], want[c][1]), "maps of frame %d differ" % c


@pytest.mark.parametrize("use_graph", [False, True])
def test_stream_equals_the_hand_built_loop(hand, use_graph):
    r, frames, _, extMs, want = hand
    vs, returned, last = _video(r, [_as_pushed(f, i) for i, f in enumerate(frames)], extMs, use_graph=use_graph)
    if use_graph:
        assert vs.stream._graph is not None, vs.stream.graph_error
    assert last is None and all(o is None for o in returned[:2 * r])
    assert [o[0] for o in returned[2 * r:]] == [i - r for i in range(2 * r, len(frames))]       # a latency of r frames
    _same({o[0]: o[1:] for o in returned[2 * r:]}, want)
    assert not torch.equal(want[r][1], want[r + 1][1])


def test_pipelined_stream_equals_the_hand_built_loop(hand):
    r, frames, _, extMs, want = hand
    vs, returned, last = _video(r, [_as_pushed(f, i + 1) for i, f in enumerate(frames)], extMs, use_graph=True, pipeline=True)
    # the first window answers at once (first-frame branch), the next call owes its frame, then one more frame of latency
    assert [None if o is None else o[0] for o in returned[2 * r:]] == [r, None] + [i - r - 1 for i in range(2 * r + 2, len(frames))]
    assert last is not None and last[0] == len(frames) - 1 - r
    outs = {o[0]: o[1:] for o in returned if o is not None}
    outs[last[0]] = last[1:]
    _same(outs, want)
    assert vs.flush() is None


def test_prepared_fp32_frames_give_the_uint8_stream(hand):
    r, _, images, extMs, want = hand
    pushed = [img.to(DEV) if i % 2 else img[None].to(DEV) for i, img in enumerate(images)]
    vs, returned, _ = _video(r, pushed, extMs, use_graph=False)
    _same({o[0]: o[1:] for o in returned if o is not None}, want)
    with pytest.raises(ValueError, match="network size"):
        vs.push(torch.zeros(3, H // 2, W, device=DEV), extMs[0])


def test_nan_pose_resets_the_filter():
    """A NaN extrinsic in the middle: its windows return None, the first clean window is a first frame again — the maps of a fresh
    DepthStream on that window."""
    r = 1
    frames, images, extMs = _sequence(r)
    bad = 3
    extMs[bad] = np.full((4, 4), np.nan)
    want = _hand_built(r, images, extMs)                         # the loop resets at every invalid window, as the reference's
    vs, returned, _ = _video(r, frames, extMs, use_graph=False)
    assert [o is None for o in returned] == [True, True, False, True, True, True, False]
    assert sorted(want) == [1, 5]
    _same({o[0]: o[1:] for o in returned if o is not None}, want)
    model, cam, d_candi = _model(r)
    fresh = DepthStream(model, cam, d_candi, t_win_r=r, use_graph=False)
    poses = np.stack([neuralrgbd_amd.homography.get_rel_extrinsicM(extMs[5], extMs[i]).astype(np.float32) for i in (4, 6)])
    o = fresh.step(images[5][None].to(DEV), torch.stack([images[4], images[6]])[None].to(DEV), torch.from_numpy(poses)[None].to(DEV))
    assert returned[6][0] == 5 and torch.equal(o[0], returned[6][1]) and torch.equal(o[1], returned[6][2])
