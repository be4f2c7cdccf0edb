"""The co-resident form of the channels-last activation pass (nrgbd_nhwc_act_lean, conv2d.hip) against the plain one
(nrgbd_nhwc_act), bit for bit: same fma, max and add in the same order, so not one bit may differ — NaN, infinities and
signed zeros included.  The shapes are the smallest at which a grid-stride streaming kernel with two slots in flight can go
wrong; the kernel's step is 256 / (C / 4) pixels per workgroup, its grid at most wg_per_cu workgroups per CU."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (C, P, ldy): fewer steps than CUs (the grid shrinks to 7 workgroups, the last one partial, and every second slot stays empty);
# a partial last step one word past a multiple of everything; the output inside a wider buffer; and enough pixels for whole
# rounds of both slots plus a partial one at wg_per_cu = 1 and at 8 on a 256-CU device (4096 and 32768 pixels per step)
SHAPES = [(64, 3 * 5 * 7, None), (64, 4 * 16 * 32 + 1, None), (32, 4 * 16 * 32 + 1, 320), (64, 37 * 4096 + 3, None)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _operands(C, P):
    g = torch.Generator().manual_seed(C * 7 + P)
    x = torch.randn(P, C, generator=g) * 3
    r = torch.randn(P, C, generator=g)
    for t, k in ((x, 0), (r, 5)):           # values whose handling the two kernels must share
        flat = t.view(-1)
        flat[k::997] = float("nan")
        flat[k + 1::997] = float("inf")
        flat[k + 2::997] = float("-inf")
        flat[k + 3::997] = -0.0
    ss = torch.randn(C, 2, generator=g)
    rs = torch.randn(C, 2, generator=g)
    return x.to(DEV), r.to(DEV), ss.to(DEV), rs.to(DEV)


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("C,P,ldy", SHAPES)
def test_lean_equals_plain_bit_for_bit(C, P, ldy, k):
    from neuralrgbd_amd import ops
    x, r, ss, rs = _operands(C, P)
    forms = {"x only": dict(),
             "relu(bn(x))": dict(x_ss=ss, x_relu=True),
             "x + res": dict(res=r),
             "bn(x) + relu(bn(res))": dict(x_ss=ss, res=r, res_ss=rs, res_relu=True)}      # the lazy-c0 site, dres2.0
    for name, kw in forms.items():
        if ldy is None:
            want = ops.nhwc_act(x, **kw)
            got = ops.nhwc_act_lean(x, wg_per_cu=k, **kw)
            assert torch.equal(_bits(got), _bits(want)), (name, int((_bits(got) != _bits(want)).sum()))
        else:
            want = torch.full((P, ldy), float("nan"), device=DEV)
            got = want.clone()
            ops.nhwc_act(x, out=want[:, 8:], ldy=ldy, **kw)          # lands at channels 8 .. 8 + C - 1 of the wider buffer
            ops.nhwc_act_lean(x, out=got[:, 8:], ldy=ldy, wg_per_cu=k, **kw)
            assert torch.equal(_bits(got[:, 8:8 + C]), _bits(want[:, 8:8 + C])), name
            rest = torch.cat([got[:, :8], got[:, 8 + C:]], 1)
            assert rest.shape[1] == ldy - C == 288 and bool(torch.isnan(rest).all()), name      # the other channels: untouched
            assert torch.equal(_bits(got), _bits(want)), name


def test_lean_refuses_what_it_cannot_walk():
    from neuralrgbd_amd import _lib, ops
    x = torch.zeros(16, 24, device=DEV)                 # C / 4 = 6 does not divide 256
    with pytest.raises(_lib.NrgbdError):
        ops.nhwc_act_lean(x)
    for k in (0, 9):
        with pytest.raises(_lib.NrgbdError):
            ops.nhwc_act_lean(torch.zeros(16, 64, device=DEV), wg_per_cu=k)


def test_knet_gain_same_bits_with_lean_passes(monkeypatch):
    """forward_channels_last with the four residual passes in the co-resident form (what a pipelined DepthStream captures into
    its back half) against the plain passes: equal bits in the gain."""
    from neuralrgbd_amd import nets, ops
    torch.manual_seed(0)
    net = nets.KalmanGainNet(16, feature_dim=64).to(DEV)
    vol = torch.randn(8, 16, 32, 16, device=DEV)
    calls = []
    lean = ops.nhwc_act_lean
    monkeypatch.setattr(ops, "nhwc_act_lean", lambda *a, **kw: (calls.append(kw.get("wg_per_cu")), lean(*a, **kw))[1])
    with torch.no_grad():
        want = net.forward_channels_last(vol)
        assert not calls
        net.lean_passes = 1
        got = net.forward_channels_last(vol)
    assert calls == [1, 1, 1, 1]
    assert bool(torch.isfinite(want).all())
    assert torch.equal(_bits(got), _bits(want))


# ---- the plumbing: which form a pipelined DepthStream captures ----------------------------------------------------------------

def _run_stream(monkeypatch, neighbours=0, knet_attr=None):
    """A pipelined DepthStream over six small windows (its four graphs are captured on the way): (the wg_per_cu of every
    nhwc_act_lean call, its outputs, its model).  `neighbours` further pipelined streams are alive on the device meanwhile."""
    import weakref
    import numpy as np
    import neuralrgbd_amd
    from neuralrgbd_amd import camera, ops, streaming, synth
    H, W, D = 256, 256, 16
    cam = camera.scannet_intrinsics(W // 4, H // 4)
    d_candi = np.linspace(0.1, 5.0, D)

    def model():
        m = neuralrgbd_amd.KVNET(64, cam, d_candi, 10.0, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=2)
        m.load_state_dict(synth.seeded_state_dict(m, 0))
        return m.to(DEV)
    monkeypatch.setattr(streaming, "_PIPELINED", weakref.WeakSet())       # streams other tests may still hold do not count here
    calls = []
    lean = ops.nhwc_act_lean
    monkeypatch.setattr(ops, "nhwc_act_lean", lambda *a, **kw: (calls.append(kw.get("wg_per_cu")), lean(*a, **kw))[1])
    m = model()
    if knet_attr is not None:
        m.kv_net.lean_passes = knet_attr
    others = [streaming.DepthStream(m, cam, d_candi, t_win_r=2, pipeline=True) for _ in range(neighbours)]
    stream = streaming.DepthStream(m, cam, d_candi, t_win_r=2, copy_outputs=True, pipeline=True)
    outs = []
    for i in range(6):
        r, s, p = synth.noise_window(40 + i, H, W)
        o = stream.step(r.to(DEV), s.to(DEV), p.to(DEV))
        if o is not None:
            outs.append(o)
    outs.append(stream.flush())
    torch.cuda.synchronize()
    stream.check()
    assert stream._graph is not None, stream.graph_error
    del others
    return calls, outs, m


def test_lone_pipelined_stream_captures_the_lean_passes(monkeypatch):
    """Four passes per slot go into the two back-half graphs in the co-resident form at one workgroup per CU; the K-Net is left as
    it was; the frames equal those of the same stream captured with the plain pass, bit for bit."""
    from neuralrgbd_amd import streaming
    calls, outs, m = _run_stream(monkeypatch)
    assert calls == [1] * 8, calls
    assert "lean_passes" not in m.kv_net.__dict__ and m.kv_net.lean_passes == 0
    monkeypatch.setattr(streaming.DepthStream, "lean_passes", 0)
    calls0, outs0, _ = _run_stream(monkeypatch)
    assert calls0 == []
    assert len(outs) == len(outs0) >= 5
    for a, b in zip(outs, outs0):
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


def test_pipelined_streams_that_share_a_device_keep_the_plain_pass(monkeypatch):
    """With a second pipelined video on the device (bench.py --streams N) no capture uses the co-resident form, and what the
    caller set on the K-Net itself survives the capture."""
    calls, _, m = _run_stream(monkeypatch, neighbours=1, knet_attr=0)
    assert calls == [], calls
    assert m.kv_net.__dict__.get("lean_passes") == 0
