"""DepthStream at its edges: a capture that fails half way, reset() with a frame in flight, and the K-Net's co-resident passes
as an argument.  Shapes of tests/test_gpu_nhwc_act_lean.py::_run_stream (256 x 256, 16 candidates); every comparison is bit for
bit against a sequential eager stream (DepthStream(pipeline=False, use_graph=False)) with a seeded model of its own."""
import weakref

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, D = 256, 256, 16
_REF = {}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _stream(**kw):
    import neuralrgbd_amd
    from neuralrgbd_amd import camera, streaming, synth
    cam = camera.scannet_intrinsics(W // 4, H // 4)
    d_candi = np.linspace(0.1, 5.0, D)
    m = neuralrgbd_amd.KVNET(64, cam, d_candi, 10.0, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=2)
    m.load_state_dict(synth.seeded_state_dict(m, 0))
    return streaming.DepthStream(m.to(DEV), cam, d_candi, t_win_r=2, copy_outputs=True, **kw)


def _run(stream, seeds, flush=True):
    """step() over the windows of `seeds` (+ flush()): the frames that came out, in order."""
    from neuralrgbd_amd import synth
    outs = []
    for s in seeds:
        r, sr, p = synth.noise_window(s, H, W)
        o = stream.step(r.to(DEV), sr.to(DEV), p.to(DEV))
        if o is not None:
            outs.append(o)
    if flush:
        o = stream.flush()
        if o is not None:
            outs.append(o)
    return outs


def _reference(seeds):
    """(frames, final bv_predict) of a fresh sequential eager stream over the windows: computed once, never written."""
    if seeds not in _REF:
        st = _stream(pipeline=False, use_graph=False)
        outs = _run(st, seeds)
        torch.cuda.synchronize()
        st.check()
        assert len(outs) == len(seeds) and st._graph is None
        _REF[seeds] = (outs, st.bv_predict.clone())
    return _REF[seeds]


def _assert_frames(got, stream, seeds):
    want, bv = _reference(seeds)
    torch.cuda.synchronize()
    stream.check()
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert _same(a[0], b[0]) and _same(a[1], b[1]), "frame %d" % i
    assert _same(stream.bv_predict, bv)


def _fail_third_graph(monkeypatch, stream):
    """The stream's third hipGraph (slot 1's front half) raises before any capture is opened."""
    real, n = stream._record, [0]

    def record(fn):
        n[0] += 1
        if n[0] == 3:
            raise RuntimeError("injected: no graph for the front half of slot 1")
        return real(fn)
    monkeypatch.setattr(stream, "_record", record)
    return n


@pytest.fixture
def alone(monkeypatch):
    from neuralrgbd_amd import streaming
    monkeypatch.setattr(streaming, "_PIPELINED", weakref.WeakSet())       # streams other tests may still hold do not count here


SEEDS8 = tuple(range(40, 48))


def test_failed_capture_leaves_one_consistent_eager_stream(monkeypatch, alone, capsys):
    stream = _stream(pipeline=True, allow_eager_fallback=True)
    n = _fail_third_graph(monkeypatch, stream)
    outs = _run(stream, SEEDS8)
    assert n[0] == 3                                         # one attempt, given up at the third graph
    assert stream.graph_error is not None and "injected" in stream.graph_error
    assert "staying eager" in capsys.readouterr().out
    assert stream._graph is None
    assert len(stream._slots) == 2 and all(sl.gf is None and sl.gb is None for sl in stream._slots)
    _assert_frames(outs, stream, SEEDS8)


def test_failed_capture_raises_without_the_fallback_and_leaves_no_graph(monkeypatch, alone):
    stream = _stream(pipeline=True)
    _fail_third_graph(monkeypatch, stream)
    with pytest.raises(RuntimeError, match="injected"):
        _run(stream, SEEDS8)
    assert stream.graph_error is not None and stream._graph is None
    assert all(sl.gf is None and sl.gb is None for sl in stream._slots)
    torch.cuda.synchronize()


@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "sequential-graph"])
def test_reset_with_a_frame_in_flight(pipeline, alone):
    stream = _stream(pipeline=pipeline)
    _run(stream, range(40, 46), flush=False)
    assert stream._graph is not None, stream.graph_error
    assert (stream._pending is not None) == pipeline         # the sixth window's front half is queued on the side stream
    stream.reset()
    assert stream._pending is None and stream.bv_predict is None
    after = tuple(range(46, 51))
    outs = _run(stream, after)
    assert stream._graph is not None
    _assert_frames(outs, stream, after)


def test_lean_form_reaches_the_knet_as_an_argument(monkeypatch):
    from neuralrgbd_amd import nets, ops
    torch.manual_seed(0)
    net = nets.KalmanGainNet(16, feature_dim=64).to(DEV)
    vol = torch.randn(8, 16, 32, 16, device=DEV)
    calls = []
    lean = ops.nhwc_act_lean
    monkeypatch.setattr(ops, "nhwc_act_lean", lambda *a, **kw: (calls.append(kw.get("wg_per_cu")), lean(*a, **kw))[1])
    with torch.no_grad():
        assert net.lean_passes == 0
        want = net.forward_channels_last(vol)
        assert not calls
        got = net.forward_channels_last(vol, lean_passes=1)
        assert calls == [1, 1, 1, 1]
        net.lean_passes = 1
        got0 = net.forward_channels_last(vol, lean_passes=0)
        assert calls == [1, 1, 1, 1]                         # lean_passes=0 overrides the attribute: no further call
    assert net.__dict__["lean_passes"] == 1
    assert bool(torch.isfinite(want).all())
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(got0), _bits(want))
