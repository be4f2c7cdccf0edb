"""The video stream (neuralrgbd_amd/video.py), host side: the ring indexing against a list that slides, the two new entries in the
header and the ctypes table, their refusals (no launch: no GPU needed), the integer nearest-resize rule against Pillow, the torch-CPU
normalisation against true fp32 divisions, and the driver logic of VideoDepthStream against the reference loop with the inner
DepthStream and the two kernels replaced by CPU recorders."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import video_ref as vr
from conftest import ROOT
from neuralrgbd_amd import _lib, camera, misc, ops, video
from neuralrgbd_amd._lib import NrgbdError


# ---- 1. window indexing ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 2, 3])
def test_window_slots_follow_the_sliding_list(r):
    R = 2 * r + 1
    window = []                                            # (frame index, ring slot) of the frames in the window, oldest first
    for i in range(3 * R):
        if len(window) == R:
            window.pop(0)
        window.append((i, i % R))
        if len(window) < R:
            with pytest.raises(ValueError):
                video.window_slots(i + 1, r)
            continue
        ref, src = misc.split_frame_list(window, r)
        got = video.window_slots(i + 1, r)
        assert got == ([s for _, s in src], ref[1], ref[0]), (r, i)
        assert got[2] == i - r and sorted(got[0] + [got[1]]) == list(range(R))


# ---- 2. symbols -----------------------------------------------------------------------------------------------------------------

def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    for name in ("nrgbd_frame_ingest_u8", "nrgbd_window_gather"):
        assert name + "(" in header and name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert "mdataloader/scanNet.py:368-369,429-430" in header and "test_KVNet.py:195,213" in header
    assert header.count('#define NRGBD_INTERFACE_VERSION "0.10"') == 1
    assert len(_lib.SIGNATURES["nrgbd_frame_ingest_u8"][1]) == 15 and len(_lib.SIGNATURES["nrgbd_window_gather"][1]) == 10
    assert ctypes.sizeof(_lib.WindowSlots) == 4 * (_lib.GATHER_MAX_V + 1)
    import neuralrgbd_amd
    assert neuralrgbd_amd.video is video and neuralrgbd_amd.VideoDepthStream is video.VideoDepthStream


# ---- 3. refused calls -----------------------------------------------------------------------------------------------------------

E_NULL, E_SHAPE, E_ALIGN, E_ARG = -1, -2, -3, -4


def _ingest(src=16, Hin=8, Win=8, pitch=24, layout=0, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25), dst=32, Hout=8, Wout=8):
    """nrgbd_frame_ingest_u8 on fake pointers: never dereferenced, every call here must return before a launch."""
    return _lib.load().nrgbd_frame_ingest_u8(ctypes.c_void_p(src), Hin, Win, pitch, layout, *mean, *std, ctypes.c_void_p(dst), Hout, Wout,
                                             None)


def test_frame_ingest_refusals_need_no_gpu():
    assert _ingest(src=None) == E_NULL and _ingest(dst=None) == E_NULL
    for dim in ("Hin", "Win", "Hout", "Wout"):
        for bad in (0, -1, 16385):
            kw = {dim: bad}
            if dim == "Win":
                kw["pitch"] = 3 * 16385                 # only the dimension is at fault
            assert _ingest(**kw) == E_SHAPE, kw
    assert _ingest(pitch=23) == E_SHAPE                                    # HWC rows need 3 Win bytes
    assert _ingest(layout=1, pitch=7) == E_SHAPE                           # CHW rows need Win bytes
    assert _ingest(dst=36) == E_ALIGN and _ingest(dst=40) == E_ALIGN
    assert _ingest(layout=2) == E_ARG and _ingest(layout=-1) == E_ARG
    for bad in (0.0, float("inf"), float("nan")):
        for c in range(3):
            std = [0.25, 0.25, 0.25]
            std[c] = bad
            assert _ingest(std=std) == E_ARG, (bad, c)
    assert _ingest(mean=(0.5, float("nan"), 0.5)) == E_ARG


def _gather(ring=16, R=5, stride=3 * 8 * 12, slots=(0, 1, 3, 4, 2), V=4, src=32, ref=48, H=8, W=12):
    st = _lib.WindowSlots()
    for i, s in enumerate(slots):
        st.idx[i] = s
    return _lib.load().nrgbd_window_gather(ctypes.c_void_p(ring), R, stride, st, V, ctypes.c_void_p(src), ctypes.c_void_p(ref), H, W, None)


def test_window_gather_refusals_need_no_gpu():
    assert _gather(ring=None) == E_NULL and _gather(src=None) == E_NULL and _gather(ref=None) == E_NULL
    assert _gather(V=0) == E_SHAPE and _gather(V=7) == E_SHAPE and _gather(V=-1) == E_SHAPE
    assert _gather(slots=(0, 1, 3, 5, 2)) == E_SHAPE and _gather(slots=(0, 1, 3, 4, -1)) == E_SHAPE      # outside [0, R)
    assert _gather(V=6, slots=(0, 1, 3, 4, 2, 9, 0)) == E_SHAPE and _gather(V=6, R=7, slots=(0, 1, 3, 4, 2, 5, 7)) == E_SHAPE
    assert _gather(stride=3 * 8 * 12 - 1) == E_SHAPE and _gather(H=0) == E_SHAPE and _gather(W=16385) == E_SHAPE and _gather(R=0) == E_SHAPE


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    u8, slot = torch.zeros(4, 6, 3, dtype=torch.uint8), torch.zeros(3, 4, 6)
    with pytest.raises(NrgbdError):
        ops.frame_ingest(u8, slot, vr.MEAN, vr.STD)
    with pytest.raises(NrgbdError):
        ops.window_gather(torch.zeros(3, 3, 4, 6), [0, 2, 1])
    with pytest.raises(ValueError):
        ops.frame_ingest(u8, slot, vr.MEAN, vr.STD, layout="nhwc")
    with pytest.raises(TypeError):
        ops.frame_ingest(u8.numpy(), slot, vr.MEAN, vr.STD)


# ---- 4. the arithmetic the kernel is specified by -------------------------------------------------------------------------------

PIL_SIZES = [((1296, 968), (384, 256)), ((640, 480), (384, 256)), ((1242, 375), (768, 256)), ((1296, 968), (1024, 768)),
             ((320, 240), (1024, 768)), ((17, 13), (7, 5)), ((5, 7), (17, 13)), ((3, 1), (2, 5)), ((1, 1), (3, 3))]       # (W, H)


@pytest.mark.parametrize("size_in,size_out", PIL_SIZES)
def test_integer_resize_rule_is_pillow_nearest(size_in, size_out):
    Image = pytest.importorskip("PIL.Image")
    (Win, Hin), (Wout, Hout) = size_in, size_out
    y, x = np.mgrid[0:Hin, 0:Win]
    img = np.stack((x & 255, y & 255, ((x >> 8) << 4) | (y >> 8)), axis=-1).astype(np.uint8)      # a pixel names its own position
    want = np.asarray(Image.fromarray(img).resize((Wout, Hout), Image.NEAREST))
    got = vr.resize_nearest(img, Hout, Wout)
    assert got.shape == want.shape and int((got != want).any(axis=-1).sum()) == 0


def test_torch_cpu_normalisation_is_two_true_fp32_divisions():
    """The formula the kernel implements, ((float)u / 255.0f - mean) / std with IEEE divisions, against ToTensor + Normalize as torch
    computes them on the CPU (the reference of tests/test_gpu_video.py), over every byte value."""
    u = np.arange(256, dtype=np.uint8)
    img = np.stack((u, u[::-1], np.roll(u, 77)), axis=-1).reshape(16, 16, 3)
    got = vr.normalise(img).numpy()
    f = img.transpose(2, 0, 1).astype(np.float32)
    want = (f / np.float32(255.0) - np.asarray(vr.MEAN, np.float32)[:, None, None]) / np.asarray(vr.STD, np.float32)[:, None, None]
    assert want.dtype == np.float32 and np.array_equal(got, want)


# ---- 5. the driver logic --------------------------------------------------------------------------------------------------------

class RecorderStream:
    """Stands in for DepthStream: records what step is handed and answers like the real one (at once on a first frame; with
    pipeline=True otherwise one call late), with (reference image, source images) as the 'maps' so that a test can tell whose they are."""
    made = []

    def __init__(self, model, cam_intrinsics, d_candi, t_win_r=2, device=None, pipeline=False, **kw):
        self.kw = dict(kw, pipeline=pipeline, t_win_r=t_win_r)
        self.pipeline = pipeline
        self.bv_predict = None
        self.pending = None
        self.steps, self.resets, self.first_frames = [], 0, 0
        RecorderStream.made.append(self)

    def reset(self):
        self.resets += 1
        self.bv_predict = None
        self.pending = None

    def step(self, ref, src, poses):
        self.steps.append((ref.clone(), src.clone(), poses.clone()))
        own = (ref.clone(), src.clone())
        if self.bv_predict is None:
            self.bv_predict = True
            self.first_frames += 1
            return own
        if not self.pipeline:
            return own
        out, self.pending = self.pending, own
        return out

    def flush(self):
        out, self.pending = self.pending, None
        return out

    def check(self):
        pass


def _cpu_ingest(frame, dst, mean, std, layout="hwc"):
    hwc = frame.numpy() if layout == "hwc" else frame.permute(1, 2, 0).numpy()
    dst.copy_(vr.normalise(vr.resize_nearest(hwc, dst.shape[1], dst.shape[2]), mean, std))
    return dst


def _cpu_gather(ring, slots, src=None, ref=None):
    src.view(len(slots) - 1, *ring.shape[1:]).copy_(torch.stack([ring[s] for s in slots[:-1]]))
    ref.view(*ring.shape[1:]).copy_(ring[slots[-1]])
    return src, ref


@pytest.fixture
def recorders(monkeypatch):
    monkeypatch.setattr(video, "DepthStream", RecorderStream)
    monkeypatch.setattr(ops, "frame_ingest", _cpu_ingest)
    monkeypatch.setattr(ops, "window_gather", _cpu_gather)
    RecorderStream.made = []


H, W, N = 12, 16, 12


def _stream(r, **kw):
    s = video.VideoDepthStream(types.SimpleNamespace(t_win_r=r), camera.scannet_intrinsics(W // 4, H // 4), np.linspace(.5, 5, 4),
                               t_win_r=r, device="cpu", **kw)
    assert (s.H, s.W) == (H, W) and tuple(s.ring.shape) == (2 * r + 1, 3, H, W)
    return s, RecorderStream.made[-1]


@pytest.mark.parametrize("pipeline", [False, True])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_windows_and_poses_are_the_reference_loops(recorders, r, pipeline):
    frames, extMs = vr.noise_frames(40 + r, N, H, W), vr.trajectory(50 + r, N)
    images = [vr.normalise(f) for f in frames]
    want = vr.driver_loop(images, extMs, r)
    s, rec = _stream(r, pipeline=pipeline, use_graph=False, copy_outputs=True)
    assert rec.kw == dict(pipeline=pipeline, use_graph=False, copy_outputs=True, t_win_r=r)
    # frames in every accepted form: uint8 numpy HWC, uint8 tensor CHW, prepared fp32 [3,H,W] / [1,3,H,W]
    forms = [lambda i: frames[i], lambda i: torch.from_numpy(frames[i]).permute(2, 0, 1).contiguous(), lambda i: images[i],
             lambda i: images[i][None]]
    outs = list(video.run_sequence(s, [forms[i % 4](i) for i in range(N)], extMs))
    assert len(rec.steps) == len(want) == N - 2 * r and rec.first_frames == 1
    for (ref, src, poses), (c, valid, w_ref, w_src, w_poses, _) in zip(rec.steps, want):
        assert valid and torch.equal(ref, w_ref[None]) and torch.equal(src, torch.stack(w_src)[None])
        assert poses.dtype == torch.float32 and tuple(poses.shape) == (1, 2 * r, 4, 4) and np.array_equal(poses[0].numpy(), w_poses)
    # every window's maps come out once, in order, under the index of the frame they belong to (the last through flush())
    assert [o[0] for o in outs] == [w[0] for w in want] == list(range(r, N - r))
    for (c, ref, src) in outs:
        assert torch.equal(ref[0], images[c])


@pytest.mark.parametrize("r", [1, 2, 3])
def test_a_nan_pose_skips_every_window_that_holds_it(recorders, r):
    R, bad = 2 * r + 1, 6
    frames, extMs = vr.noise_frames(60 + r, N, H, W), vr.trajectory(70 + r, N)
    extMs[bad] = np.full((4, 4), np.nan)
    want = vr.driver_loop([vr.normalise(f) for f in frames], extMs, r)
    s, rec = _stream(r)
    resets0 = rec.resets
    results, reset_at = [], []
    for i in range(N):
        before = rec.resets
        results.append(s.push(frames[i], extMs[i]))
        if rec.resets != before:
            assert rec.resets == before + 1
            reset_at.append(i)
    holds = [i for i in range(R - 1, N) if i - R < bad <= i]             # pushes whose window holds the bad frame
    assert [i for i in range(R - 1, N) if results[i] is None] == holds == reset_at
    assert all(o is None for o in results[:R - 1]) and rec.resets - resets0 == len(holds)
    if r < 3:
        assert len(holds) == R                                            # 12 frames: the bad frame's R windows all complete
    assert [not w[1] for w in want] == [i in holds for i in range(R - 1, N)]
    valid = [w for w in want if w[1]]
    assert len(rec.steps) == len(valid)
    for (ref, src, poses), w in zip(rec.steps, valid):
        assert torch.equal(ref, w[2][None]) and np.array_equal(poses[0].numpy(), w[4])
    assert rec.first_frames == int(R - 1 < holds[0]) + int(holds[-1] < N - 1)      # the first clean window starts over
    assert [o[0] for o in results if o is not None] == [w[0] for w in valid]
    # a loader's missing pose (an int) counts as invalid too (test_KVNet.py:37)
    s.reset()
    before = rec.resets
    assert all(s.push(frames[i], -1 if i == 0 else extMs[0]) is None for i in range(R)) and rec.resets == before + 1


def test_refused_input_raises_before_any_launch(recorders, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work started")
    with pytest.raises(ValueError, match="t_win_r"):
        video.VideoDepthStream(types.SimpleNamespace(t_win_r=1), camera.scannet_intrinsics(4, 3), np.linspace(.5, 5, 4), t_win_r=2, device="cpu")
    with pytest.raises(ValueError, match="t_win_r"):
        _stream(4)
    with pytest.raises(ValueError, match="std"):
        _stream(2, std=(0.2, 0.0, 0.2))
    s, rec = _stream(2)
    monkeypatch.setattr(ops, "frame_ingest", boom)
    monkeypatch.setattr(ops, "window_gather", boom)
    E = np.eye(4)
    for bad in (torch.zeros(3, H + 1, W), torch.zeros(2, 3, H, W), np.zeros((H, W, 3), np.float32), np.zeros((H, W, 4), np.uint8),
                torch.zeros(H, W, dtype=torch.uint8), torch.zeros(3, H, W, dtype=torch.float64), None):
        with pytest.raises(ValueError):
            s.push(bad, E)
    with pytest.raises(ValueError, match="4 x 4"):
        s.push(torch.zeros(3, H, W), np.eye(3))
    assert s.n_pushed == 0 and not rec.steps
