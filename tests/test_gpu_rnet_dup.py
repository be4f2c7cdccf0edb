"""The R-Net with candidate up-sampling (KVNET(if_upsample_d=True); Refine.py:44-49: 4 D candidates at full resolution) on the GPU:
the 256-channel rows log-softmax, the depth regression / export epilogue on channels-last rows, the wide layers by themselves, the
whole up-sampler against the float64 module graph, whole frames and one training iteration against the UNMODIFIED reference
(tests/golden/rnet_dup_d32.npz, tests/gen_rnet_dup_golden.py), the stream forms against each other, and the shapes that keep raising."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_rnet_dup_golden as gd
import neuralrgbd_amd
from neuralrgbd_amd import _lib, misc, nets, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, D, R = gd.DUP["H"], gd.DUP["W"], gd.DUP["D"], gd.DUP["r"]


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


# ---- 1. log-softmax over 256-channel rows -------------------------------------------------------------------------------------

@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("rows", [1, 4, 5, 960])
def test_logsoftmax_rows_256_forward_and_backward(rows, inplace):
    """One wave per row, four rows per workgroup: a partial workgroup, a whole one, a partial last one, many.  Against float64
    log_softmax and its analytic gradient g - softmax(x) sum(g) at 1e-6; one row holds a -1e30 entry (no fp32 number lies within 1e-6
    of its log-probability: that one entry is held to the input's own value instead), one is constant."""
    C = 256
    x = _rand(rows, C, seed=rows)
    x[0, 7] = -1e30
    if rows > 1:
        x[rows - 1, :] = 0.375
    g = _rand(rows, C, seed=rows + 100)
    x64, g64 = x.double(), g.double()
    want = torch.log_softmax(x64, dim=1)
    want_g = g64 - torch.softmax(x64, dim=1) * g64.sum(1, keepdim=True)
    src = x.clone()
    y = ops.logsoftmax_rows(src, inplace=inplace)
    assert (y.data_ptr() == src.data_ptr()) == inplace
    if not inplace:
        assert torch.equal(src, x)
    gx = ops.logsoftmax_rows_bwd(y, g)
    torch.cuda.synchronize()
    d_f = (y.double() - want).abs()
    d_f[0, 7] = 0.0                                    # the -1e30 entry: checked by itself below
    e_f, e_b = d_f.max().item(), (gx.double() - want_g).abs().max().item()
    print("[parity] logsoftmax_rows C=256 rows %d inplace %d: forward max|d| %.2e, backward max|d| %.2e (|log p| max %.1f)"
          % (rows, inplace, e_f, e_b, want[want > -1e20].abs().max().item()))
    assert e_f < 1e-6 and e_b < 1e-6
    assert float(y[0, 7]) == float(x[0, 7]) and float(gx[0, 7]) == float(g[0, 7])   # -1e30 - (m + log s) rounds to -1e30; exp of it is 0: the gradient passes through
    if rows > 1:
        assert torch.equal(y[rows - 1], torch.full((C,), float(y[rows - 1, 0]), device=DEV))      # a constant row stays constant


def test_logsoftmax_rows_widths():
    for C in (64, 128, 256):
        x = _rand(7, C, seed=C)
        assert (ops.logsoftmax_rows(x, inplace=False).double() - torch.log_softmax(x.double(), 1)).abs().max().item() < 5e-6
    with pytest.raises(_lib.NrgbdError):
        ops.logsoftmax_rows(_rand(7, 512, seed=1))
    with pytest.raises(_lib.NrgbdError):
        ops.logsoftmax_rows_bwd(_rand(7, 192, seed=1), _rand(7, 192, seed=2))
    torch.cuda.synchronize()


# ---- 2. regression / export on channels-last rows -----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 24 * 40])
@pytest.mark.parametrize("Dv", [64, 128, 256])
def test_rows_regress_and_export_have_the_planar_bits(Dv, n):
    rows = torch.log_softmax(_rand(n, Dv, seed=Dv + n, scale=3.0), dim=1)          # [n][D]: the R-Net's memory
    view = rows.t()                                                               # [D, n] view of it
    planar = view.contiguous()
    assert ops.is_channels_last_view(view) or n == 1
    d = torch.linspace(0.1, 5.0, Dv, device=DEV)
    got = ops.depth_regress(view, d, channels_last=True)
    want = ops.depth_regress(planar, d)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    only_depth = ops.depth_regress(view, d, want_conf=False, channels_last=True)
    assert only_depth[1] is None and torch.equal(only_depth[0], want[0])
    ge = ops.export_depth_u16(view, d, 1000.0, 60000.0, channels_last=True)
    we = ops.export_depth_u16(planar, d, 1000.0, 60000.0)
    for a, b in zip(ge, we):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int16) if a.dtype == torch.uint16 else a,
                                                  b.view(torch.int16) if b.dtype == torch.uint16 else b)
    assert int(we[2].view(torch.int16).to(torch.int32).abs().max()) > 0


def test_rows_entries_argument_checks():
    x = torch.zeros(64 * 8 + 4, device=DEV)
    d, o = torch.zeros(2048, device=DEV), torch.zeros(64, device=DEV)
    lib = _lib.load()
    p = lambda t: t.data_ptr()
    call = lambda D_, n, off=0: lib.nrgbd_depth_regress_rows(p(x) + off, p(d), p(o), None, D_, n, None)
    assert call(64, 8) == 0
    assert call(6, 8) == -2 and call(1028, 1) == -2 and call(0, 8) == -2 and call(64, 0) == -2
    assert call(64, 8, off=4) == -3
    assert lib.nrgbd_depth_regress_rows(None, p(d), p(o), None, 64, 8, None) == -1
    assert lib.nrgbd_export_depth_u16_rows(p(x), p(d), 1.0, 1.0, None, None, None, None, 64, 8, None) == -1
    with pytest.raises(ValueError):
        ops.depth_regress(torch.zeros(64, 8, device=DEV)[:, ::2], d[:64], channels_last=True)
    torch.cuda.synchronize()


# ---- 3. the wide layers by themselves -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,Hh,Ww,Cin,Cout,tail", [(1, 24, 40, 272, 256, False), (2, 12, 20, 160, 128, True)])
def test_wide_winograd_layers(N, Hh, Ww, Cin, Cout, tail):
    """nrgbd_conv_wino_rnet_ex_f32 at the widths of the up-sampling net: 17 stages into four 64-column groups (conv2 / conv2_1 from
    64 candidates), 10 stages into two groups plus the 32-column tail of conv1 (160 -> 160 = 128 + 32) at ycoff 128 of a 192-wide buffer."""
    co_all = Cout + (32 if tail else 0)
    x = _rand(N, Cin, Hh, Ww, seed=41)
    w = _rand(co_all, Cin, 3, 3, seed=42, scale=0.05)
    b = _rand(co_all, seed=43, scale=0.2)
    want = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), 1, 1), 0.01)
    ldy = 192 if tail else Cout
    out = torch.full((N, Hh, Ww, ldy), 7.0, device=DEV)
    xc = x.permute(0, 2, 3, 1).contiguous()
    ops.conv_wino_rnet(xc, ops.conv_wino_pack(w[:Cout].contiguous()), Cout, bias=b[:Cout].contiguous(), lrelu=True, out=out, ycoff=0,
                       cout_valid=Cout)
    if tail:
        ops.conv_wino_rnet(xc, ops.conv_wino_pack32(w[Cout:].contiguous()), 32, bias=b[Cout:].contiguous(), lrelu=True, out=out,
                           ycoff=Cout, cout_valid=32)
    err = (out[..., :co_all].permute(0, 3, 1, 2).double() - want).abs().max().item()
    print("[parity] wide Winograd layer N%d %dx%d %d->%d: max|d vs fp64|=%.2e (|y|max %.1f)" % (N, Hh, Ww, Cin, co_all, err, want.abs().max().item()))
    assert err < 2e-5 * max(1.0, want.abs().max().item())
    assert bool((out[..., co_all:] == 7.0).all())


def test_few_columns_behind_256():
    """conv_few.hip with 17 input blocks: the 3 columns of conv2 (259 -> 259) beyond its four groups, at ycoff 256 of a 272-wide buffer."""
    N, Hh, Ww, Cin, ldx, Cout = 1, 21, 35, 259, 272, 3
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, Hh, Ww, ldx, generator=g)
    x[..., Cin:] = 0.0
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1
    b = torch.randn(Cout, generator=g)
    wp = torch.zeros(Cout, ldx, 3, 3)
    wp[:, :Cin] = w
    few = wp.reshape(Cout, ldx // 16, 16, 9).permute(1, 3, 0, 2).contiguous().to(DEV)
    assert few.shape[0] == 17
    out = torch.full((N, Hh, Ww, 272), 5.0, device=DEV)
    ops.conv2d_few(x.to(DEV), few, bias=b.to(DEV), lrelu=True, out=out, ycoff=256)
    want = F.leaky_relu(F.conv2d(x[..., :Cin].permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1), 0.01).permute(0, 2, 3, 1)
    err = (out[..., 256:259].double().cpu() - want).abs().max().item()
    print("[parity] conv_few 17 blocks -> 3 columns at 256: max|d|=%.2e (|y|max %.1f)" % (err, want.abs().max().item()))
    assert err < 2e-5 * max(1.0, want.abs().max().item())
    assert bool((out[..., :256] == 5.0).all()) and bool((out[..., 259:] == 5.0).all())


def test_transposed_conv_160_to_256_in_four_slices():
    """trans_conv1 of the up-sampling net from 64 candidates: mode 3 (all four sub-pixel phases per launch), one launch per 64-column
    slice, into a 272-wide buffer whose 16 remaining channels keep their sentinel."""
    Hh, Ww, Cin, Cout = 12, 20, 160, 256
    x = _rand(1, Cin, Hh, Ww, seed=51)
    w = _rand(Cin, Cout, 4, 4, seed=52, scale=0.05)
    b = _rand(Cout, seed=53, scale=0.1)
    want = F.leaky_relu(F.conv_transpose2d(x.double(), w.double(), b.double(), 2, 1), 0.01)
    xc = x.permute(0, 2, 3, 1).contiguous()
    out = torch.zeros(1, 2 * Hh, 2 * Ww, 272, device=DEV)
    out[..., Cout:] = 9.0
    for c0 in range(0, Cout, 64):
        packed = []
        for pa in (0, 1):
            for pb in (0, 1):
                ky = [3, 1] if pa == 0 else [2, 0]
                kx = [3, 1] if pb == 0 else [2, 0]
                packed.append(ops.conv_pack_weights(w[:, c0:c0 + 64][:, :, ky][:, :, :, kx].permute(1, 0, 2, 3).contiguous()))
        ops.conv2d_rnet(xc, torch.cat(packed), 64, bias=b[c0:c0 + 64].contiguous(), out=out, ldy=272, ycoff=c0, cout_valid=64, mode=3)
    err = (out[..., :Cout].permute(0, 3, 1, 2).double() - want).abs().max().item()
    print("[parity] transposed conv 160->256 (4 slices): max|d vs fp64|=%.2e (|y|max %.1f)" % (err, want.abs().max().item()))
    assert err < 2e-5 * max(1.0, want.abs().max().item())
    assert bool((out[..., Cout:] == 9.0).all())


# ---- 4. the whole up-sampler against the float64 module graph -----------------------------------------------------------------

def _rnet(Dq, seed=11):
    torch.manual_seed(seed)
    net = nets.DPVUpsampleNet(64, 32, 3, D=Dq, upsample_D=True)
    for m in net.modules():
        if getattr(m, "bias", None) is not None:
            torch.nn.init.normal_(m.bias, 0, 0.1)
    return net


def _graphs(net, dpv, feats):
    """(float64 module graph, error of the plain fp32 torch module graph on the host against it): the yardstick the code under
    test does not enter."""
    cpu = copy.deepcopy(net).cpu()
    with torch.no_grad():
        want = cpu.double()(dpv.cpu().double(), [f.cpu().double() for f in feats])
        plain = copy.deepcopy(net).cpu().float()(dpv.cpu(), [f.cpu() for f in feats])
    return want, (plain.double() - want).abs().max().item()


@pytest.mark.parametrize("h,w", [(6, 10), (16, 24)])
@pytest.mark.parametrize("Dq", [32, 64])
def test_forward_log_and_module_call_vs_float64_modules(Dq, h, w):
    """forward_log (batch of 1 and the frame's two volumes as a list) and the module call (with and without a graph being recorded)
    against Refine.py:79-107 in float64 on the host.  Allowed: the larger of the project's rule 1e-4 + 3e-6 max|log p|
    (test_gpu_cnn.py::test_rnet_module_call_vs_float64_modules) and 4 x what the plain fp32 torch graph on the host shows against
    the same float64 graph (Winograd sums in another order than a direct convolution)."""
    net = _rnet(Dq).to(DEV)
    lg = [torch.log_softmax(_rand(1, Dq, h, w, seed=60 + i, scale=2.0), dim=1) for i in range(2)]
    feats = [_rand(1, 64, h, w, seed=63), _rand(1, 32, 2 * h, 2 * w, seed=64), torch.rand(1, 3, 4 * h, 4 * w, generator=torch.Generator().manual_seed(65)).to(DEV)]
    wants, plain = zip(*[_graphs(net, torch.exp(v), feats) for v in lg])
    scale = max(w_.abs().max().item() for w_ in wants)
    bound = max(1e-4 + 3e-6 * scale, 4.0 * max(plain))
    print("[parity] up-sampling R-Net D=%d %dx%d: bound %.3e = max(1e-4 + 3e-6 x %.1f, 4 x %.3e)" % (Dq, h, w, bound, scale, max(plain)))
    with torch.no_grad():
        one = net.forward_log(lg[0], feats).clone()
        both = net.forward_log((lg[0], lg[1]), feats).clone()
    assert tuple(one.shape) == (1, 4 * Dq, 4 * h, 4 * w) and tuple(both.shape) == (2, 4 * Dq, 4 * h, 4 * w)
    assert one.permute(0, 2, 3, 1).is_contiguous()
    errs = {"forward_log": (one.cpu().double() - wants[0]).abs().max().item(),
            "forward_log[2] a": (both[0:1].cpu().double() - wants[0]).abs().max().item(),
            "forward_log[2] b": (both[1:2].cpu().double() - wants[1]).abs().max().item()}
    with torch.enable_grad():
        errs["module call, graph recorded"] = (net(torch.exp(lg[0]), feats).detach().cpu().double() - wants[0]).abs().max().item()
    with torch.no_grad():
        errs["module call"] = (net(torch.exp(lg[0]), feats).cpu().double() - wants[0]).abs().max().item()
    for k, e in errs.items():
        print("[parity]   %-28s max|d log p| %.3e" % (k, e))
    for k, e in errs.items():
        assert e < bound, (k, e, bound)
    # the regression reads the view where it lies: the bits of the transposing copy
    d_up = misc.d_candi_up4(np.linspace(0.1, 5.0, Dq))
    assert torch.equal(misc.depth_val_regression(one, d_up), misc.depth_val_regression(one.contiguous(), d_up))
    assert torch.equal(misc.dpv_confidence(one), misc.dpv_confidence(one.contiguous()))


def test_backward_from_64_candidates_vs_float64_autograd():
    """The module call under autograd at the widths only a 64-candidate up-sampling net has — LogSoftmaxCL at 256 channels, the 272 / 272
    data gradient with its 3 columns on conv_few.hip, the weight gradients at 272 and 160, the 160 -> 1024 transposed convolution with the
    32-column data-gradient tail — on a 6 x 10 grid: every parameter's gradient and the input's against torch autograd of the same
    graph in float64 on the host.  Allowed, relative to the largest element of each gradient: the larger of 3.6e-4 (nine layers
    forward and nine backward, each held to 2e-5 of its largest output by tests/test_gpu_rnet.py's rule, adding at worst linearly) and
    4 x what plain fp32 torch autograd on the host shows against the same float64 gradients."""
    Dq, h, w = 64, 6, 10
    net = nets.DPVUpsampleNet(64, 32, 3, D=Dq, upsample_D=True)
    net.load_state_dict(synth.seeded_state_dict(net, 3))
    dpv = torch.softmax(_rand(1, Dq, h, w, seed=70, scale=2.0), dim=1).cpu()
    feats = [_rand(1, 64, h, w, seed=71).cpu(), _rand(1, 32, 2 * h, 2 * w, seed=72).cpu(),
             torch.rand(1, 3, 4 * h, 4 * w, generator=torch.Generator().manual_seed(73))]
    gout = _rand(1, 4 * Dq, 4 * h, 4 * w, seed=74).cpu()

    def grads(module, cast):
        x = cast(dpv).requires_grad_(True)
        out = module(x, [cast(f) for f in feats])
        (out * cast(gout)).sum().backward()
        return dict([("input", x.grad.detach().double().cpu())] + [(k, p.grad.detach().double().cpu()) for k, p in module.named_parameters()])
    want = grads(copy.deepcopy(net).double(), lambda t: t.double())
    plain = grads(copy.deepcopy(net), lambda t: t.clone())
    got = grads(copy.deepcopy(net).to(DEV), lambda t: t.to(DEV))
    assert set(got) == set(want) and len(want) == 19
    for k in want:
        scale = want[k].abs().max().item()
        assert scale > 0, k
        e_plain, e_got = (plain[k] - want[k]).abs().max().item() / scale, (got[k] - want[k]).abs().max().item() / scale
        bound = max(3.6e-4, 4.0 * e_plain)
        print("[parity] D=64 backward %-24s rel err %.2e (plain fp32 on the host %.2e, bound %.2e)" % (k, e_got, e_plain, bound))
    for k in want:
        scale = want[k].abs().max().item()
        e_plain, e_got = (plain[k] - want[k]).abs().max().item() / scale, (got[k] - want[k]).abs().max().item() / scale
        assert e_got < max(3.6e-4, 4.0 * e_plain), (k, e_got, e_plain)


# ---- 5. whole frames against the unmodified reference -------------------------------------------------------------------------

def _model(upsample=True, Dq=None):
    cam, d_candi = gd.setup()
    if Dq is not None:
        d_candi = np.linspace(gd.DUP["d_min"], gd.DUP["d_max"], Dq)
    m = neuralrgbd_amd.KVNET(64, cam, d_candi, gd.DUP["sigma"], 64, None, if_refined=True, refineNet_name="DPV", t_win_r=R,
                             if_upsample_d=upsample)
    sd = synth.seeded_state_dict(m, gd.DUP["weight_seed"])
    m.load_state_dict(sd)
    return m.to(DEV), sd, cam, d_candi


@pytest.fixture(scope="module")
def golden():
    from oracle import gen_golden
    g = dict(np.load(gd.PATH))
    _, sd, _, _ = _model()
    assert abs(gen_golden.checksum(sd.values()) - float(g["weights_checksum"])) < 1e-6 * float(g["weights_checksum"])
    return g


def _two_frames(model, cam, d_candi, wins, r):
    """KVNET.forward + PREDICT into source view r per frame (test_utils/test_KVNet.py::test), every output kept."""
    import math
    from neuralrgbd_amd import homography as Hm
    outs, pred = [], None
    pad = math.log(1. / float(len(d_candi)))
    for (rf, s, p) in wins:
        with torch.no_grad():
            r_cur, r_kv, bv_cur, dpv = model(rf.cuda(), s.cuda(), p.cuda(), torch.zeros(1), cam_intrinsics=[cam], BV_predict=pred)
            nxt = Hm.resample_vol_cuda(dpv, ops.pose_inverse(p[0, r].cuda().contiguous()), cam_intrinsic=cam, d_candi=d_candi,
                                       padding_value=pad, clamp=(-1000., 0.)).unsqueeze(0)
        outs.append(dict(bv_cur=bv_cur.clone(), dpv=dpv.clone(), pred=nxt.clone(), refined_cur=r_cur.clone(), refined=r_kv.clone()))
        pred = nxt
    return outs


def test_two_frames_vs_the_reference(golden):
    """First frame, PREDICT, update frame of KVNET(if_upsample_d=True): BV_cur, DPV, BV_predict and the refined [1, 128, 256, 256]
    volumes under the gates of tests/test_gpu_parity_configs.py::_check on the pixels the fixture stores."""
    from test_gpu_parity_configs import _check
    model, _, cam, d_candi = _model()
    outs = _two_frames(model, cam, d_candi, gd.windows(), R)
    for o in outs:
        assert tuple(o["refined_cur"].shape) == tuple(o["refined"].shape) == (1, 4 * D, H, W)
    worst = {}
    for key, sub in gd.VOLUMES:
        name, f = key.rsplit("_f", 1)
        got = outs[int(f) - 1][name][:, :, ::sub, ::sub]
        assert torch.isfinite(got).all(), key
        kw = {}
        if name == "pred":
            kw = dict(argmax=False, max_abs=worst["bv_cur_f1"] + 2e-4)
        worst[key] = _check("up-sampling %s vs REFERENCE" % key, got, torch.from_numpy(golden[key])[None], **kw)
    # the export epilogue on the view, with the loaders' up-sampled candidates
    from neuralrgbd_amd import export_res
    r = outs[1]["refined"]
    a = export_res.depth_conf_u16(r, misc.d_candi_up4(d_candi))
    b = export_res.depth_conf_u16(r.contiguous(), misc.d_candi_up4(d_candi))
    assert all(torch.equal(x.view(torch.int16) if x.dtype == torch.uint16 else x, y.view(torch.int16) if y.dtype == torch.uint16 else y)
               for x, y in zip(a, b))


# ---- 6. the stream ------------------------------------------------------------------------------------------------------------

def _stream_outputs(wins, **kw):
    from neuralrgbd_amd.streaming import DepthStream
    model, _, cam, d_candi = _model()
    stream = DepthStream(model, cam, d_candi, t_win_r=R, copy_outputs=True, **kw)
    outs = []
    for rf, s, p in wins:
        o = stream.step(rf.to(DEV), s.to(DEV), p.to(DEV))
        if o is not None:
            outs.append((o[0].clone(), o[1].clone()))
    if kw.get("pipeline"):
        outs.append(stream.flush())
    torch.cuda.synchronize()
    stream.check()
    return stream, outs


def test_depth_stream_graph_and_pipeline_equal_eager():
    """DepthStream over six frames with an up-sampling model: the hipGraph replay and the pipelined form equal the eager stream bit
    for bit (tests/test_gpu_twin.py::test_depth_stream_graph_and_pipeline_equal_eager)."""
    wins = [synth.noise_window(280 + i, H, W, V=2 * R) for i in range(6)]
    _, eager = _stream_outputs(wins, use_graph=False)
    st_g, graph = _stream_outputs(wins, use_graph=True)
    st_p, piped = _stream_outputs(wins, use_graph=True, pipeline=True)
    assert st_g._graph is not None, st_g.graph_error
    assert st_p._graph is not None, st_p.graph_error
    assert len(eager) == len(graph) == len(piped) == 6
    shapes = {tuple(t.shape) for o in eager for t in o}
    assert (1, 4 * D, H, W) in shapes, shapes
    for f, (a, b, c) in enumerate(zip(eager, graph, piped)):
        assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "graph replay differs from eager at frame %d" % f
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]), "pipelined differs from sequential at frame %d" % f
    assert not torch.equal(eager[1][1], eager[2][1])


# ---- 7. training --------------------------------------------------------------------------------------------------------------

def _train_call(model, opt, cam, d_candi, win, dm, dmf, pred, **kw):
    from neuralrgbd_amd.train_step import train
    rf, s, p = win
    return train(1, model, opt, R, d_candi, [{"img": rf, "dmap": dm, "dmap_up4_imgsize_digit": dmf}],
                 [[{"img": s[0, v:v + 1]} for v in range(2 * R)]], p, pred, [cam], refine_dup=True, **kw)


def test_update_iteration_vs_the_reference(golden):
    """One UPDATE-branch iteration of train(refine_dup=True) from the fixture's weights, seeded volume and labels, plain SGD: loss,
    BV_predict and the weight change of the probe tensors (the fixture's sampled elements, relative to the largest change of the whole
    tensor) at the tolerances of tests/test_gpu_twin.py::test_update_iteration_vs_the_reference."""
    g = golden
    model, _, cam, d_candi = _model()
    opt = torch.optim.SGD(model.parameters(), lr=gd.DUP["lr"])
    before = {k: model.state_dict()[k].detach().clone() for k in gd.probes()}
    dm, dmf = gd.labels()
    r_dpv, pred, loss, lo, hi = _train_call(model, opt, cam, d_candi, gd.windows()[1], dm, dmf, gd.train_bv_predict().to(DEV))
    assert tuple(r_dpv.shape) == (1, 4 * D, H, W) and tuple(hi.shape) == (1, H, W) and tuple(lo.shape) == (1, H // 4, W // 4)
    assert float(hi.max()) <= float(d_candi.max()) * (1 + 1e-5) and float(hi.min()) >= 0.0      # regressed with linspace(0, d_max, 4 D)
    want = float(g["train_loss"])
    e_pred = np.abs(pred[0].cpu().numpy()[:, ::gd.SUB_T, ::gd.SUB_T] - g["train_pred"])
    print("[parity] up-sampling train update iteration: loss %.6f vs reference %.6f; BV_predict mean|d| %.2e max %.2e" %
          (float(loss), want, e_pred.mean(), e_pred.max()))
    assert abs(float(loss) - want) < 2e-5 * want
    assert e_pred.mean() < 2e-3
    for k in gd.probes():
        delta = gd.sample((model.state_dict()[k].detach() - before[k]).cpu().numpy())
        ref_d, ref_max = g["train_delta_" + k], float(g["train_delta_max_" + k])
        assert delta.shape == ref_d.shape and ref_max > 0
        rel = np.abs(delta - ref_d).max() / ref_max
        print("[parity]   d %-62s rel err %.2e (|lr grad| max %.2e)" % (k, rel, ref_max))
        assert rel < 5e-2, (k, rel)
        # every element of the change, through its sums over all but the first axis (same tolerance, relative to the largest sum)
        full = (model.state_dict()[k].detach() - before[k]).cpu().numpy()
        rows, ref_rows = gd.row_sums(full), g["train_delta_rows_" + k]
        rel_rows = np.abs(rows - ref_rows).max() / np.abs(ref_rows).max()
        print("[parity]     sums over the first axis: rel err %.2e" % rel_rows)
        assert rel_rows < 5e-2, (k, rel_rows)


def test_deterministic_training_is_bit_reproducible():
    rng = np.random.RandomState(31)
    wins = [synth.noise_window(4400 + i, H, W, V=2 * R) for i in range(3)]
    labels = [(torch.from_numpy(rng.randint(0, D, (1, H // 4, W // 4))), torch.from_numpy(rng.randint(0, 4 * D, (1, H, W)))) for _ in wins]

    def run():
        from neuralrgbd_amd.optim import FusedAdam
        model, _, cam, d_candi = _model()
        opt = FusedAdam(model.parameters(), lr=1e-4)
        pred = None
        for win, (dm, dmf) in zip(wins, labels):      # first frame, then two update iterations
            _, pred, loss, _, _ = _train_call(model, opt, cam, d_candi, win, dm, dmf, pred, deterministic=True)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        return {k: v.detach().clone() for k, v in model.state_dict().items()}
    s1, s2 = run(), run()
    bad = [k for k in s1 if not torch.equal(s1[k], s2[k])]
    assert not bad, "%d tensors differ between two deterministic runs, first %s" % (len(bad), bad[0])
    fresh = _model()[0].state_dict()
    assert not torch.equal(fresh["r_net.conv2_2.weight"], s1["r_net.conv2_2.weight"])


def test_train_graph_equals_eager_train():
    """TrainGraph(refine_dup=True).step against train(refine_dup=True) on an identical twin, at the bounds of
    tests/test_gpu_twin.py::test_train_graph_equals_eager_train."""
    from neuralrgbd_amd.train_step import TrainGraph
    model, _, cam, d_candi = _model()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, betas=(.9, .999), capturable=True)
    rng = np.random.RandomState(R)

    def window(i):
        rf, s, p = synth.noise_window(4500 + i, H, W, V=2 * R)
        return (rf, s, p, torch.from_numpy(rng.randint(0, D, (1, H // 4, W // 4))), torch.from_numpy(rng.randint(0, 4 * D, (1, H, W))))
    pred = None
    for i in range(2):
        w_ = window(i)
        _, pred, _, _, _ = _train_call(model, opt, cam, d_candi, w_[:3], w_[3], w_[4], pred)
    twin_m = copy.deepcopy(model)
    opt2 = torch.optim.Adam(twin_m.parameters(), lr=1e-4, betas=(.9, .999), capturable=True)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    w2 = window(2)
    _, pred_e, loss_e, _, _ = _train_call(model, opt, cam, d_candi, w2[:3], w2[3], w2[4], pred)
    tg = TrainGraph(twin_m, opt2, R, d_candi, cam, warmup=0, refine_dup=True)
    loss_g, pred_g = tg.step(*[t.to(DEV) for t in w2], pred)
    torch.cuda.synchronize()
    assert tg._graph is not None
    print("[parity] up-sampling train graph vs eager: loss %.6f vs %.6f, max|d BV_predict|=%.2e" %
          (float(loss_g), float(loss_e), (pred_g - pred_e).abs().max().item()))
    assert abs(float(loss_g) - float(loss_e)) < 1e-3 * abs(float(loss_e))
    assert (pred_g - pred_e).abs().mean().item() < 1e-3
    for a, b in ((model.kv_net.dres1[0][0].weight, twin_m.kv_net.dres1[0][0].weight),
                 (model.kv_net.dres0[0][0].weight, twin_m.kv_net.dres0[0][0].weight),
                 (model.r_net.conv2_2.weight, twin_m.r_net.conv2_2.weight)):
        assert (a - b).abs().max().item() < 5e-4


# ---- 8. what keeps raising ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Dq", [16, 128])
def test_uncovered_candidate_counts_raise(Dq):
    net = nets.DPVUpsampleNet(64, 32, 3, D=Dq, upsample_D=True).to(DEV)
    h, w = 8, 16
    feats = [_rand(1, 64, h, w, seed=1), _rand(1, 32, 2 * h, 2 * w, seed=2), _rand(1, 3, 4 * h, 4 * w, seed=3)]
    with torch.no_grad(), pytest.raises(_lib.NrgbdError):
        net.forward_log(torch.log_softmax(_rand(1, Dq, h, w, seed=4), dim=1), feats)


def test_lba_stream_raises_at_construction():
    from neuralrgbd_amd import camera, lba_step
    model, _, _, d_candi = _model()
    cams = [camera.scannet_intrinsics(W // k, H // k) for k in (4, 2, 1)]
    with pytest.raises(_lib.NrgbdError, match="if_upsample_d"):
        lba_step.LBADepthStream(model, cams, d_candi, R, 1, [np.eye(4)] * 8)
