"""The training video stream (neuralrgbd_amd/train_video.py), host side: Pillow's NEAREST index rule and the label thresholds against
the real thing, the new entry in the header and the ctypes table, its refusals (no launch: no GPU needed), the label tables against
the PIL comparator through a numpy statement of the kernel's contract, and the driver logic of TrainVideoStream against the
reference's training loop with train(), TrainGraph and the kernels replaced by CPU recorders."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import train_video_ref as tr
import video_ref as vr
from conftest import ROOT
from neuralrgbd_amd import _lib, camera, ops, train_video
from neuralrgbd_amd._lib import NrgbdError


# ---- 1. Pillow's NEAREST ----------------------------------------------------------------------------------------------------------

PAIRS = [(640, 96), (480, 64), (1308, 234), (152, 546), (1296, 384), (968, 256), (640, 384), (480, 256), (1242, 768), (375, 256),
         (300, 256), (160, 64), (160, 256), (37, 64), (53, 96), (37, 16), (53, 24), (30, 18), (41, 27), (30, 9), (41, 13), (7, 7), (1, 5),
         (5, 1)]
IMAGE_PAIRS = [(1296, 384), (968, 256), (640, 384), (480, 256), (1242, 768), (375, 256)]       # where the reference resizes images


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_pillow_nearest_index_is_pillow(n_in, n_out):
    want = tr.pil_nearest_index(n_in, n_out, "I")
    assert np.array_equal(train_video.pillow_nearest_index(n_in, n_out), want)
    assert np.array_equal(tr.pil_nearest_index(n_in, n_out, "F"), want)                          # the mask's and the frame's modes agree
    if n_in <= 256:
        assert np.array_equal(tr.pil_nearest_index(n_in, n_out, "L"), want)
    if (n_in, n_out) in IMAGE_PAIRS:
        assert np.array_equal(tr.integer_nearest_index(n_in, n_out), want)


def test_the_integer_rule_is_not_pillow_at_scannets_depth_width():
    want = tr.pil_nearest_index(640, 96)
    diff = np.nonzero(tr.integer_nearest_index(640, 96) != want)[0]
    assert diff.tolist() == [25, 28, 31, 34, 37, 40, 43, 94]
    assert np.array_equal(tr.integer_nearest_index(640, 96)[diff] - want[diff], np.ones(8, dtype=np.int64))
    assert not np.array_equal(tr.integer_nearest_index(1308, 234), tr.pil_nearest_index(1308, 234))


def test_the_twice_resized_mask_is_not_the_direct_one():
    lab = train_video.DepthLabeler(np.linspace(.1, 5, 8), (256, 384), (64, 96), device="cpu")
    _, _, rows_q, cols_q, mrows, mcols = lab.host_tables(480, 640)
    assert int((rows_q != mrows).sum()) == 64 and int((cols_q != mcols).sum()) == 72             # of 64 rows, of 96 columns
    assert int((tr.integer_nearest_index(640, 96) != mcols).sum()) == 64                         # (against the integer rule's direct columns)
    assert np.array_equal(mrows, tr.pil_nearest_index(480, 256)[tr.pil_nearest_index(256, 64)])
    assert np.array_equal(mcols, tr.pil_nearest_index(640, 384)[tr.pil_nearest_index(384, 96)])


# ---- 2. thresholds ----------------------------------------------------------------------------------------------------------------

CANDI = {"s8": np.linspace(.1, 5, 8), "s32": np.linspace(.1, 5, 32), "s64": np.linspace(.1, 5, 64), "s128": np.linspace(.1, 5, 128),
         "k64": np.linspace(1, 60, 64)}
CANDI.update({k + "_up4": tr.up4(v) for k, v in list(CANDI.items())})


@pytest.mark.parametrize("name", sorted(CANDI))
def test_label_thresholds_reproduce_digitize_on_every_value(name):
    d = CANDI[name]
    T = train_video.label_thresholds(d)
    assert T.dtype == np.int32 and T.shape == d.shape and np.all(np.diff(T) >= 0) and T.min() >= 0 and T.max() <= 65536
    u = np.arange(65536)
    metres = (torch.from_numpy(u.astype(np.int32)).float() * .001).numpy()                       # the loaders' product
    want = np.digitize(metres, d)
    got = (T[None, :] <= u[:, None]).sum(axis=1)
    assert np.array_equal(got, want)


def test_fp32_candidates_would_give_a_wrong_label():
    d = CANDI["s64_up4"]
    assert len(d) == 256
    u = np.arange(65536)
    metres = u.astype(np.float32) * np.float32(.001)
    assert int((np.digitize(metres, d) != np.digitize(metres, d.astype(np.float32))).sum()) == 1


def test_label_thresholds_refuse_bad_candidates():
    for bad in ([1.0, 1.0, 2.0], [2.0, 1.0], [1.0, float("nan")], [1.0, float("inf")], []):
        with pytest.raises(ValueError):
            train_video.label_thresholds(np.asarray(bad))
    with pytest.raises(ValueError):
        train_video.label_thresholds(np.linspace(1, 2, 4), depth_scale=0.0)


# ---- 3. symbols and refusals ------------------------------------------------------------------------------------------------------

def test_new_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    assert "nrgbd_depth_ingest_u16(" in header and "nrgbd_depth_ingest_u16" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "nrgbd_depth_ingest_u16")
    assert "mdataloader/scanNet.py:372-422" in header and "mdataloader/misc.py:13-36" in header
    assert header.count('#define NRGBD_INTERFACE_VERSION "0.10"') == 1
    assert "#define NRGBD_DEPTH_MAX_THRESHOLDS %d" % _lib.DEPTH_MAX_THRESHOLDS in header
    decl = header[header.index("int nrgbd_depth_ingest_u16("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") + 1 == len(_lib.SIGNATURES["nrgbd_depth_ingest_u16"][1]) == 24
    import neuralrgbd_amd
    assert neuralrgbd_amd.train_video is train_video
    for name in ("TrainVideoStream", "DepthLabeler", "run_training_sequence", "pillow_nearest_index", "label_thresholds"):
        assert getattr(neuralrgbd_amd, name) is getattr(train_video, name)


E_ARG = -4
_THR = (ctypes.c_int * 4)(100, 200, 300, 65536)


def _entry(depth=16, Hin=8, Win=8, pitch=8, tables=(32, 48, 64, 80, 96, 112), scale=.001, thr_q=_THR, n_q=4, thr_full=_THR, n_full=4,
           outs=(128, 144, 160, 176), H=8, W=8, h=2, w=2):
    """nrgbd_depth_ingest_u16 on fake device pointers: never dereferenced, every call here must return before a launch."""
    vp = lambda a: a if isinstance(a, ctypes.Array) else ctypes.c_void_p(a)
    return _lib.load().nrgbd_depth_ingest_u16(vp(depth), Hin, Win, pitch, *(vp(t) for t in tables), scale, vp(thr_q), n_q, vp(thr_full),
                                              n_full, *(vp(o) for o in outs), H, W, h, w, None)


def test_depth_ingest_refusals_need_no_gpu():
    assert _entry(depth=None) == E_ARG
    for i in range(6):
        t = [32, 48, 64, 80, 96, 112]
        t[i] = None
        assert _entry(tables=t) == E_ARG, i
    assert _entry(thr_q=None) == E_ARG and _entry(thr_full=None) == E_ARG
    assert _entry(outs=(None, None, None, None)) == E_ARG
    for dim in ("Hin", "Win", "H", "W", "h", "w"):
        for bad in (0, -1, 16385):
            kw = {dim: bad}
            if dim == "Win":
                kw["pitch"] = 16385
            assert _entry(**kw) == E_ARG, kw
    assert _entry(pitch=7) == E_ARG
    for n in (0, -1, 513):
        assert _entry(n_q=n) == E_ARG and _entry(n_full=n) == E_ARG
    assert _entry(thr_q=(ctypes.c_int * 4)(100, 99, 300, 400)) == E_ARG                          # decreasing
    assert _entry(thr_full=(ctypes.c_int * 4)(100, 200, 300, 299)) == E_ARG
    assert _entry(thr_q=(ctypes.c_int * 4)(-1, 200, 300, 400)) == E_ARG and _entry(thr_q=(ctypes.c_int * 4)(1, 2, 3, 65537)) == E_ARG
    for bad in (0.0, -0.001, float("inf"), float("nan")):
        assert _entry(scale=bad) == E_ARG


def test_wrapper_refuses_cpu_tensors_and_bad_arguments():
    lab = train_video.DepthLabeler(np.linspace(.1, 5, 8), (8, 12), (2, 3), device="cpu")
    frame = np.ones((6, 9), np.uint16)
    with pytest.raises(NrgbdError):
        lab(frame)                                                                               # no CPU path behind the wrapper
    with pytest.raises(ValueError):
        lab(frame.astype(np.float32))
    with pytest.raises(ValueError):
        lab(np.ones((2, 6, 9), np.uint16))
    with pytest.raises(ValueError):
        lab(frame, out={"dmap_up4_imgsize_digit": torch.zeros(1, 8, 12, dtype=torch.int64)})     # not this labeler's key
    with pytest.raises(ValueError):
        train_video.DepthLabeler(np.linspace(.1, 5, 129), (8, 12), (2, 3), refine_dup=True, device="cpu")     # 516 thresholds
    with pytest.raises(TypeError):
        ops.depth_ingest(frame, lab.tables(6, 9), .001, lab.thr_q, lab.thr_full)


# ---- 4. tables and thresholds together: a numpy statement of the kernel's contract against the PIL comparator ---------------------

def _cpu_depth_ingest(depth, tables, depth_scale, thr_q, thr_full, labels_q=None, labels_full=None, dmap_raw=None, dmap_imgsize=None):
    u = depth.numpy().view(np.uint16).astype(np.int64)
    rf, cf, rq, cq, mr, mc = (t.numpy() for t in tables)
    full, q = u[rf][:, cf], u[rq][:, cq]
    q = np.where(u[mr][:, mc] == 0, 0, q)
    for x, thr, lab, met in ((q, thr_q, labels_q, dmap_raw), (full, thr_full, labels_full, dmap_imgsize)):
        if lab is not None:
            lab.view(x.shape).copy_(torch.from_numpy(np.minimum((thr[None, None, :] <= x[..., None]).sum(-1), len(thr) - 1)))
        if met is not None:
            met.view(x.shape).copy_(torch.from_numpy(x.astype(np.float32) * np.float32(depth_scale)))
    return labels_q, labels_full, dmap_raw, dmap_imgsize


@pytest.mark.parametrize("sizes", [((480, 640), (256, 384), (64, 96)), ((37, 53), (64, 96), (16, 24)), ((30, 41), (18, 27), (9, 13))])
@pytest.mark.parametrize("dup", [False, True])
def test_tables_and_thresholds_give_the_loaders_maps(monkeypatch, sizes, dup):
    monkeypatch.setattr(ops, "depth_ingest", _cpu_depth_ingest)
    (Hin, Win), net, grid = sizes
    d_candi = np.linspace(.1, 5, 16)
    frame = tr.depth_frames(3, 1, Hin, Win)[0]
    assert 0.2 < float((frame == 0).mean()) < 0.5
    want = tr.prepare_depth(frame, net, grid, d_candi)
    lab = train_video.DepthLabeler(d_candi, net, grid, refine_dup=dup, device="cpu")
    got = lab(frame)
    assert sorted(got) == sorted(["dmap", lab.full_key, "dmap_raw", "dmap_imgsize"])
    assert lab.full_key == ("dmap_up4_imgsize_digit" if dup else "dmap_imgsize_digit")
    for k, v in got.items():
        assert v.dtype == want[k].dtype and torch.equal(v, want[k]), k
    assert int((got["dmap"] == 0).sum()) > 0 and int(got[lab.full_key].max()) == (64 if dup else 16) - 1


# ---- 5. the driver logic ----------------------------------------------------------------------------------------------------------

class Recorder:
    """Stands in for train() and TrainGraph.step: records what it is handed and answers with a BV_predict that names the window."""

    def __init__(self):
        self.calls = []

    def train(self, nGPU, model, opt, r, d_candi, Ref_Dats, Src_Dats, poses, bv, cams, **kw):
        assert nGPU == 1 and len(Ref_Dats) == 1 and len(Src_Dats) == 1 and len(Src_Dats[0]) == 2 * r
        ref = Ref_Dats[0]
        full = [k for k in ref if k.endswith("imgsize_digit")]
        assert len(full) == 1
        self.calls.append(dict(how="train", ref=ref["img"].clone(), src=torch.cat([s["img"] for s in Src_Dats[0]]).clone(), poses=poses.clone(),
                               dmap=ref["dmap"].clone(), full_key=full[0], dmap_full=ref[full[0]].clone(), bv=bv, kw=kw))
        n = float(len(self.calls))
        self.calls[-1]["out_bv"] = torch.tensor(n)
        return torch.tensor(n + .1), self.calls[-1]["out_bv"], torch.tensor(n + .2), torch.tensor(n + .3), torch.tensor(n + .4)

    def graph(self, model, opt, r, d_candi, cam, **kw):
        self.graph_kw = kw
        return types.SimpleNamespace(step=self.step)

    def step(self, ref, src, poses, dmap, dmap_full, bv):
        assert bv is not None
        self.calls.append(dict(how="graph", ref=ref.clone(), src=src[0].clone(), poses=poses.clone(), dmap=dmap.clone(), full_key=None,
                               dmap_full=dmap_full.clone(), bv=bv, kw={}))
        n = float(len(self.calls))
        self.calls[-1]["out_bv"] = torch.tensor(n)
        return torch.tensor(n + .2), self.calls[-1]["out_bv"]


def _cpu_ingest(frame, dst, mean, std, layout="hwc"):
    hwc = frame.numpy() if layout == "hwc" else frame.permute(1, 2, 0).numpy()
    dst.copy_(vr.normalise(vr.resize_nearest(hwc, dst.shape[1], dst.shape[2]), mean, std))
    return dst


def _cpu_gather(ring, slots, src=None, ref=None):
    src.view(len(slots) - 1, *ring.shape[1:]).copy_(torch.stack([ring[s] for s in slots[:-1]]))
    ref.view(*ring.shape[1:]).copy_(ring[slots[-1]])
    return src, ref


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(train_video, "train", r.train)
    monkeypatch.setattr(train_video, "TrainGraph", r.graph)
    monkeypatch.setattr(ops, "frame_ingest", _cpu_ingest)
    monkeypatch.setattr(ops, "window_gather", _cpu_gather)
    monkeypatch.setattr(ops, "depth_ingest", _cpu_depth_ingest)
    return r


H, W, N = 12, 16, 16
D_CANDI = np.linspace(.5, 5, 4)


def _stream(r, model=None, **kw):
    model = model or types.SimpleNamespace(t_win_r=r)
    return train_video.TrainVideoStream(model, None, camera.scannet_intrinsics(W // 4, H // 4), D_CANDI, t_win_r=r, device="cpu", **kw)


def _sequence(seed, r, missing_depth=(), nan_pose=()):
    frames, extMs = vr.noise_frames(seed, N, H + 3, W + 5), vr.trajectory(seed + 1, N)
    depths = tr.depth_frames(seed + 2, N, 10, 13)
    for i in nan_pose:
        extMs[i] = np.full((4, 4), np.nan)
    depths = [-1 if i in missing_depth else d for i, d in enumerate(depths)]
    images = [vr.normalise(vr.resize_nearest(f, H, W)) for f in frames]
    labels = [None if isinstance(d, int) else tr.prepare_depth(d, (H, W), (H // 4, W // 4), D_CANDI) for d in depths]
    items = [{"dmap": -1 if lab is None else lab["dmap"], "extM": extMs[i], "idx": i} for i, lab in enumerate(labels)]
    return frames, depths, extMs, images, labels, tr.driver_loop(items, r)


def _check_calls(rec, want, images, labels, r, full_key, results, use_graph=False):
    valid = [w for w in want if w[1]]
    assert len(rec.calls) == len(valid) and any(w[2] for w in valid)
    prev = None
    for call, (c, _, first, poses, src_idx) in zip(rec.calls, valid):
        assert call["how"] == ("graph" if use_graph and not first else "train")
        assert torch.equal(call["ref"], images[c][None]) and torch.equal(call["src"], torch.stack([images[i] for i in src_idx]))
        assert call["poses"].dtype == torch.float32 and np.array_equal(call["poses"][0].numpy(), poses)
        assert torch.equal(call["dmap"], labels[c]["dmap"]) and torch.equal(call["dmap_full"], labels[c][full_key])
        assert call["full_key"] in (None, full_key)
        if first:
            assert call["bv"] is None
        else:
            assert call["bv"] is prev                      # what the previous step predicted, handed on as it is
        prev = call["out_bv"]
    got = [o for o in results if o is not None]
    assert [o[0] for o in got] == [w[0] for w in valid] and all(len(o) == 5 for o in got)
    # a push answers None exactly for the windows the reference's loop skips
    R = 2 * r + 1
    assert [o is None for o in results] == [True] * (R - 1) + [not w[1] for w in want]


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_windows_labels_and_poses_are_the_reference_loops(rec, monkeypatch, r, use_graph):
    frames, depths, extMs, images, labels, want = _sequence(100 + r, r)
    s = _stream(r, use_graph=use_graph, deterministic=True, grad_clip_max=2.0)
    # frames and depth maps in every accepted form
    fforms = [lambda i: frames[i], lambda i: torch.from_numpy(frames[i]).permute(2, 0, 1).contiguous(), lambda i: images[i]]
    dforms = [lambda i: depths[i], lambda i: torch.from_numpy(depths[i]), lambda i: torch.from_numpy(depths[i].view(np.int16))[None]]
    results = [s.push(fforms[i % 3](i), dforms[i % 3](i), extMs[i] if i % 2 else torch.from_numpy(extMs[i])) for i in range(N)]
    assert all(w[1] for w in want) and [w[2] for w in want] == [True] + [False] * (N - 2 * r - 1)
    _check_calls(rec, want, images, labels, r, "dmap_imgsize_digit", results, use_graph)
    assert rec.calls[0]["kw"] == dict(refine_dup=False, deterministic=True, grad_clip_max=2.0, skip_nonfinite=False)
    if use_graph:
        assert rec.graph_kw == dict(deterministic=True, refine_dup=False, grad_clip_max=2.0, skip_nonfinite=False)
        assert results[-1][2:] == (None, None, None)
    # the generator form gives the same answers
    rec2 = Recorder()
    monkeypatch.setattr(train_video, "train", rec2.train)
    monkeypatch.setattr(train_video, "TrainGraph", rec2.graph)
    s2 = _stream(r, use_graph=use_graph)
    outs = list(train_video.run_training_sequence(s2, frames, depths, extMs))
    assert [o[0] for o in outs] == [o[0] for o in results if o is not None] == list(range(r, N - r))


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("kind", ["depth", "pose"])
@pytest.mark.parametrize("r,bad", [(1, 5), (2, 6), (2, 4), (3, 7)])
def test_prev_invalid_rule(rec, r, bad, kind, use_graph):
    kw = {"missing_depth": (bad,)} if kind == "depth" else {"nan_pose": (bad,)}
    frames, depths, extMs, images, labels, want = _sequence(200 + r, r, **kw)
    s = _stream(r, use_graph=use_graph)
    results = [s.push(frames[i], depths[i], extMs[i]) for i in range(N)]
    R = 2 * r + 1
    assert [not w[1] for w in want] == [i - R < bad <= i for i in range(R - 1, N)]                # the windows that hold the bad frame
    firsts = [w[0] for w in want if w[2]]
    assert firsts[-1] == bad + r + 1 and len(firsts) == (2 if bad >= R else 1)                   # the first clean window starts over
    _check_calls(rec, want, images, labels, r, "dmap_imgsize_digit", results, use_graph)


def test_missing_depth_and_pose_forms(rec):
    frames, depths, extMs, images, labels, _ = _sequence(300, 1)
    s = _stream(1)
    for bad_depth, bad_pose in ((None, extMs[1]), (-1, extMs[1]), (depths[1], None), (depths[1], -1)):
        s.reset()
        outs = [s.push(frames[i], bad_depth if i == 1 else depths[i], bad_pose if i == 1 else extMs[i]) for i in range(5)]
        assert [o is None for o in outs] == [True, True, True, True, False] and len(rec.calls) == 1 and rec.calls[0]["bv"] is None
        rec.calls.clear()


def test_reset_starts_a_new_trajectory(rec):
    frames, depths, extMs, images, labels, want = _sequence(400, 2)
    s = _stream(2)
    for i in range(7):
        s.push(frames[i], depths[i], extMs[i])
    assert len(rec.calls) == 3 and rec.calls[0]["bv"] is None and rec.calls[2]["bv"] is not None and s.bv_predict is not None
    s.reset()
    assert s.n_pushed == 0 and s.bv_predict is None
    rec.calls.clear()
    results = [s.push(frames[i], depths[i], extMs[i]) for i in range(N)]
    _check_calls(rec, want, images, labels, 2, "dmap_imgsize_digit", results)


def test_refine_dup_hands_the_up4_label(rec):
    frames, depths, extMs, images, labels, want = _sequence(500, 2)
    s = _stream(2, model=types.SimpleNamespace(t_win_r=2, if_upsample_d=True), refine_dup=True)
    results = [s.push(frames[i], depths[i], extMs[i]) for i in range(N)]
    _check_calls(rec, want, images, labels, 2, "dmap_up4_imgsize_digit", results)
    assert rec.calls[0]["full_key"] == "dmap_up4_imgsize_digit" and rec.calls[0]["kw"]["refine_dup"] is True
    assert int(rec.calls[0]["dmap_full"].max()) > len(D_CANDI) - 1


def test_refusals_raise_before_any_launch(rec, monkeypatch):
    with pytest.raises(ValueError, match="t_win_r"):
        _stream(2, model=types.SimpleNamespace(t_win_r=1))
    with pytest.raises(ValueError, match="t_win_r"):
        _stream(4)
    with pytest.raises(ValueError, match="refine_dup"):
        _stream(2, refine_dup=True)
    with pytest.raises(ValueError, match="refine_dup"):
        _stream(2, model=types.SimpleNamespace(t_win_r=2, if_upsample_d=True))
    with pytest.raises(ValueError, match="grad_reducer"):
        _stream(2, grad_reducer=lambda: None)
    with pytest.raises(ValueError, match="std"):
        _stream(2, std=(0.2, 0.0, 0.2))
    with pytest.raises(ValueError):
        _stream(2, skip_nonfinite=True)                                                          # needs FusedAdam
    s = _stream(2)

    def boom(*a, **k):
        raise AssertionError("device work started")
    for name in ("frame_ingest", "window_gather", "depth_ingest"):
        monkeypatch.setattr(ops, name, boom)
    frame, depth, E = np.zeros((H, W, 3), np.uint8), np.ones((5, 6), np.uint16), np.eye(4)
    for bad in (np.ones((5, 6), np.int32), np.ones((5, 6), np.float32), torch.ones(5, 6), np.ones((2, 5, 6), np.uint16), "depth.pgm"):
        with pytest.raises(ValueError):
            s.push(frame, bad, E)
    with pytest.raises(ValueError, match="4 x 4"):
        s.push(frame, depth, np.eye(3))
    with pytest.raises(ValueError):
        s.push(np.zeros((H, W, 4), np.uint8), depth, E)
    assert s.n_pushed == 0 and not rec.calls
