"""Feature-CNN kernels (conv2d.hip): fp32-MFMA 3x3 convolution with fused BatchNorm / ReLU / residual, the
channels-last statistics / activation helpers, and the whole matrix-core trunk — against torch's F.conv2d /
F.batch_norm on the same GPU (a plain fp32 torch reference is the oracle for a floating-point kernel) and against
the module's own vendor-library forward()."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cl(x):   # [N,C,H,W] -> channels-last [N,H,W,C]
    return x.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("N,H,W,Cin,Cout,dil", [
    (2, 32, 48, 32, 32, 1), (1, 16, 16, 64, 64, 1), (3, 21, 37, 64, 64, 1), (2, 24, 40, 64, 128, 1),
    (2, 30, 34, 128, 128, 1), (2, 30, 34, 128, 128, 2), (1, 5, 7, 128, 128, 2), (1, 16, 32, 320, 128, 1),
    (5, 48, 64, 16, 32, 1), (1, 40, 56, 96, 96, 1), (1, 33, 47, 80, 64, 1)])
def test_conv2d_plain_vs_torch(N, H, W, Cin, Cout, dil):
    from neuralrgbd_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + H + Cin)
    x = torch.randn(N, Cin, H, W, generator=g).to(DEV)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05).to(DEV)
    want = F.conv2d(x, w, padding=dil, dilation=dil)
    y, stats, _ = ops.conv2d(_cl(x), ops.conv_pack_weights(w), Cout, dil)
    got = y.permute(0, 3, 1, 2)
    err = (got - want).abs().max().item()
    scale = want.abs().max().item()
    print("[parity] conv2d N%d %dx%d %d->%d dil%d max|d|=%.3e (|y|max %.2f)" % (N, H, W, Cin, Cout, dil, err, scale))
    assert err < 2e-5 * max(1.0, scale)
    s = stats.double().sum(0)
    assert torch.allclose(s[:Cout], want.double().sum((0, 2, 3)), rtol=1e-5, atol=1e-3)
    assert torch.allclose(s[Cout:], (want.double() ** 2).sum((0, 2, 3)), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("Cin,Cout,dil", [(32, 32, 1), (64, 64, 1), (128, 128, 2)])
def test_conv2d_fused_prologue_materialize_epilogue(Cin, Cout, dil):
    """in = relu(x*s+t) + (res*s'+t'); zero padding applies to the ACTIVATED tensor; bias + LeakyReLU epilogue."""
    from neuralrgbd_amd import ops
    N, H, W = 2, 19, 35
    g = torch.Generator().manual_seed(Cin + dil)
    x = torch.randn(N, Cin, H, W, generator=g).to(DEV)
    r = torch.randn(N, Cin, H, W, generator=g).to(DEV)
    ss = torch.randn(Cin, 2, generator=g).to(DEV)
    rs = torch.randn(Cin, 2, generator=g).to(DEV)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05).to(DEV)
    b = torch.randn(Cout, generator=g).to(DEV)
    inp = torch.relu(x * ss[:, 0].view(1, -1, 1, 1) + ss[:, 1].view(1, -1, 1, 1)) + (r * rs[:, 0].view(1, -1, 1, 1) + rs[:, 1].view(1, -1, 1, 1))
    want = F.leaky_relu(F.conv2d(inp, w, b, padding=dil, dilation=dil), 0.01)
    y, stats, mat = ops.conv2d(_cl(x), ops.conv_pack_weights(w), Cout, dil, x_ss=ss, x_relu=True, res=_cl(r), res_ss=rs,
                               materialize=True, bias=b, out_lrelu=True)
    assert (mat.permute(0, 3, 1, 2) - inp).abs().max().item() < 1e-5
    err = (y.permute(0, 3, 1, 2) - want).abs().max().item()
    print("[parity] conv2d fused %d->%d dil%d max|d|=%.3e" % (Cin, Cout, dil, err))
    assert err < 3e-5 * max(1.0, want.abs().max().item())
    s = stats.double().sum(0)
    assert torch.allclose(s[:Cout], want.double().sum((0, 2, 3)), rtol=1e-5, atol=1e-3)
    # identity residual (no scale/shift), no ReLU anywhere
    y2, _, _ = ops.conv2d(_cl(x), ops.conv_pack_weights(w), Cout, dil, res=_cl(r), want_stats=False)
    want2 = F.conv2d(x + r, w, padding=dil, dilation=dil)
    assert (y2.permute(0, 3, 1, 2) - want2).abs().max().item() < 3e-5 * max(1.0, want2.abs().max().item())


@pytest.mark.parametrize("C", [32, 64, 128])
def test_nhwc_stats_act_finalize_vs_batchnorm(C):
    """nhwc_stats -> bn_finalize -> nhwc_act == F.batch_norm(training=True) (+ReLU, + residual), running stats updated."""
    from neuralrgbd_amd import ops
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(3, 37, 53, C, generator=g) * 2 + 0.5).to(DEV)
    r = torch.randn(3, 37, 53, C, generator=g).to(DEV)
    gamma, beta = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    rm2, rv2 = rm.clone(), rv.clone()
    want = torch.relu(F.batch_norm(x.view(-1, C), rm2, rv2, gamma, beta, True, 0.1, 1e-5)).view_as(x) + r
    ss = ops.bn_finalize(ops.nhwc_stats(x), x.numel() // C, gamma, beta, 1e-5, 0.1, rm, rv)
    got = ops.nhwc_act(x, ss, True, r)
    assert (got - want).abs().max().item() < 2e-5
    assert torch.allclose(rm, rm2, atol=1e-6) and torch.allclose(rv, rv2, rtol=1e-5, atol=1e-6)
    wide = torch.full((3, 37, 53, C + 8), 7.0, device=DEV)
    ops.nhwc_act(x, ss, True, r, out=wide, ldy=C + 8)
    assert torch.equal(wide[..., :C], got) and bool((wide[..., C:] == 7.0).all())


@pytest.mark.parametrize("H,W", [(256, 384), (480, 640), (264, 328)])
def test_trunk_matrix_core_vs_vendor_forward(H, W):
    """PSMFeatures.forward_channels_last (inference kernels) and PSMFeatures.forward (the module composition of the autograd-capable
    kernels, here without a graph) against the CHECKER: oracle/kvnet_oracle.feature_cnn — the reference graph on ATen's own
    convolutions / batch norms — executed on the same GPU with the same weights and batch statistics.  (Since round 5 nothing
    in the package reaches the vendor library on a GPU tensor: the vendor result exists only here, as test infrastructure.)"""
    from neuralrgbd_amd import nets
    from oracle import kvnet_oracle as ko
    torch.manual_seed(3)
    fe = nets.FeatureExtractor(feature_dim=64, multi_scale=True).to(DEV)
    x = torch.rand(5, 3, H, W, device=DEV)
    with torch.no_grad():
        half_ref, feat_ref = ko.feature_cnn({k: v.detach() for k, v in fe.state_dict().items()}, "feature_extraction", x)
        half_mod, feat_mod = fe(x)
        half, feat = fe.forward_channels_last(x)
    for tag, hh, ff in (("inference kernels", half.permute(0, 3, 1, 2), feat.permute(0, 3, 1, 2)), ("module composition", half_mod, feat_mod)):
        e1 = (hh - half_ref).abs().max().item()
        e2 = (ff - feat_ref).abs().max().item()
        print("[parity] CNN trunk %dx%d, %s: layer1 max|d|=%.3e (|.|max %.2f)  feat max|d|=%.3e (|.|max %.2f)"
              % (H, W, tag, e1, half_ref.abs().max().item(), e2, feat_ref.abs().max().item()))
        assert e1 < 1e-4 * max(1.0, half_ref.abs().max().item())
        assert e2 < 2e-4 * max(1.0, feat_ref.abs().max().item())


def test_shapes_without_a_kernel_raise_instead_of_reaching_the_vendor_library():
    """DESIGN.md section 2 "no fallback": a layer shape the hand-written kernels do not cover is an NrgbdError on the GPU."""
    from neuralrgbd_amd import nets
    from neuralrgbd_amd._lib import NrgbdError
    fe = nets.FeatureExtractor(feature_dim=48, multi_scale=True).to(DEV)          # 1x1 head 128 -> 48: no instantiation
    with torch.no_grad(), pytest.raises(NrgbdError):
        fe.forward_channels_last(torch.rand(2, 3, 256, 256, device=DEV))
    fe = nets.FeatureExtractor(feature_dim=64, multi_scale=True).to(DEV)
    with torch.no_grad(), pytest.raises(NrgbdError):
        fe.forward_channels_last(torch.rand(2, 3, 258, 256, device=DEV))          # image side not a multiple of 4
    rn = nets.DPVUpsampleNet(64, 32, 3, D=16, upsample_D=True).to(DEV)            # candidate up-sampling: never selected by the reference's scripts
    with torch.no_grad(), pytest.raises(NrgbdError):
        rn.forward_log(torch.log_softmax(torch.randn(1, 16, 8, 8, device=DEV), 1),
                       [torch.randn(1, 64, 8, 8, device=DEV), torch.randn(1, 32, 16, 16, device=DEV), torch.rand(1, 3, 32, 32, device=DEV)])
    conv = torch.nn.Conv2d(16, 16, 5, padding=2).to(DEV)
    from neuralrgbd_amd.autograd import conv2d_module
    with pytest.raises(NrgbdError):
        conv2d_module(conv, torch.randn(1, 16, 8, 8, device=DEV))


def test_pack_nhwc_channels_last_input():
    from neuralrgbd_amd import ops
    g = torch.Generator().manual_seed(0)
    feat = torch.randn(3, 64, 24, 40, generator=g).to(DEV)
    rgb = torch.rand(3, 3, 96, 160, generator=g).to(DEV)
    a = ops.pack_nhwc(feat, rgb)
    b = ops.pack_nhwc(feat.permute(0, 2, 3, 1).contiguous(), rgb, channels_last=True)
    assert torch.equal(a, b)


@pytest.mark.parametrize("h,w,D", [(16, 24, 64), (30, 40, 64), (16, 24, 16)])
def test_rnet_module_call_vs_float64_modules(h, w, D):
    """DPVUpsampleNet.forward (the module call: probabilities in; the composition of the autograd-capable kernels, with and
    without a graph being recorded) == the plain nn.Module graph (Refine.py:79-107) in float64 on the host."""
    import copy
    from neuralrgbd_amd import nets, ops
    torch.manual_seed(11)
    net = nets.DPVUpsampleNet(64, 32, 3, D=D).to(DEV)
    for m in net.modules():
        if getattr(m, "bias", None) is not None:
            torch.nn.init.normal_(m.bias, 0, 0.1)
    dpv = torch.softmax(torch.randn(1, D, h, w, device=DEV), dim=1)
    feats = [torch.randn(1, 64, h, w, device=DEV), torch.randn(1, 32, 2 * h, 2 * w, device=DEV),
             torch.rand(1, 3, 4 * h, 4 * w, device=DEV)]
    with torch.no_grad():
        want = copy.deepcopy(net).cpu().double()(dpv.cpu().double(), [f.cpu().double() for f in feats]).float().to(DEV)
    with torch.enable_grad():
        got_g = net(dpv, feats).detach()
    with torch.no_grad():
        got = net(dpv, feats)
        feats_cl = [f.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for f in feats[:2]] + [feats[2]]
        got2 = net(dpv, feats_cl)       # channels-last feature views, as the matrix-core D-Net hands them over
    err = (got - want).abs().max().item()
    scale = want.abs().max().item()     # He-initialised convs + bilinear transposed convs: the logits of this random net reach ~1e4
    print("[parity] R-Net module call %dx%d D=%d max|d log p|=%.3e (|log p| max %.1f)" % (h, w, D, err, scale))
    # relative to the size of the logits (3e-6 = a few dozen ulps)
    assert got.shape == want.shape and err < 1e-4 + 3e-6 * scale
    assert (got_g - got).abs().max().item() < 1e-4 + 3e-6 * scale      # with a graph being recorded the padded widths (and so the kernel forms) may differ
    assert (got2 - got).abs().max().item() < 1e-4 + 3e-6 * scale
    x = torch.randn(2, 5, 6, 10, device=DEV)
    b = torch.randn(5, device=DEV)
    ref = F.leaky_relu(x + b.view(1, -1, 1, 1), 0.01)
    assert torch.allclose(ops.bias_act_(x.clone(), b, 0.01), ref, atol=1e-7)


# ----------------------------------------------------------------------------- Winograd-domain 2-D layers (wino_pc.hip, kd = 1)
@pytest.mark.parametrize("N,H,W,Cin,Cout,dil", [
    (1, 16, 16, 64, 64, 1), (3, 21, 37, 64, 64, 1), (2, 24, 40, 64, 128, 1), (2, 30, 34, 128, 128, 1),
    (2, 30, 34, 128, 128, 2), (1, 5, 7, 128, 128, 2), (1, 16, 32, 320, 128, 1), (5, 48, 64, 32, 64, 1),
    (5, 96, 128, 64, 64, 1), (2, 33, 47, 128, 128, 2)])
def test_conv_wino_pc_2d_plain_vs_torch(N, H, W, Cin, Cout, dil):
    """Producer/consumer Winograd kernel, kd = 1: the feature CNN's 3x3 stride-1 layers (dilation 1 and 2, 64-column output
    groups, any Cin % 16) vs F.conv2d in float64, statistics rows included."""
    from neuralrgbd_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + H + Cin)
    x = torch.randn(N, Cin, H, W, generator=g).to(DEV)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05).to(DEV)
    want = F.conv2d(x.double(), w.double(), padding=dil, dilation=dil)
    y, stats, _ = ops.conv_wino(_cl(x), ops.conv_wino_pack(w), Cout, 1, dil)
    err = (y.permute(0, 3, 1, 2).double() - want).abs().max().item()
    scale = want.abs().max().item()
    print("[parity] conv_wino_pc 2d N%d %dx%d %d->%d dil%d max|d vs fp64|=%.3e (|y|max %.2f)" % (N, H, W, Cin, Cout, dil, err, scale))
    assert err < 2e-5 * max(1.0, scale)
    assert stats.shape == (2 * Cout, ops.conv_wino_tiles(N, H, W, dil))
    s = stats.double().sum(1)
    assert torch.allclose(s[:Cout], want.sum((0, 2, 3)), rtol=1e-5, atol=1e-3)
    assert torch.allclose(s[Cout:], (want ** 2).sum((0, 2, 3)), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("Cin,Cout,dil", [(64, 64, 1), (128, 128, 2)])
def test_conv_wino_pc_2d_fused_prologue_materialize(Cin, Cout, dil):
    # at most 48 tiles: one tile per workgroup.  The fused forms where every workgroup hands a tile over to a next one (next-tile
    # book, owner bits, weight ring into the next tile), against float64, are in tests/test_gpu_wino_pc_walk.py
    from neuralrgbd_amd import ops
    N, H, W = 2, 19, 35
    g = torch.Generator().manual_seed(Cin + dil)
    x = torch.randn(N, Cin, H, W, generator=g).to(DEV)
    r = torch.randn(N, Cin, H, W, generator=g).to(DEV)
    ss = torch.randn(Cin, 2, generator=g).to(DEV)
    rs = torch.randn(Cin, 2, generator=g).to(DEV)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05).to(DEV)
    inp = torch.relu(x * ss[:, 0].view(1, -1, 1, 1) + ss[:, 1].view(1, -1, 1, 1)) + (r * rs[:, 0].view(1, -1, 1, 1) + rs[:, 1].view(1, -1, 1, 1))
    want = F.conv2d(inp, w, padding=dil, dilation=dil)
    y, stats, mat = ops.conv_wino(_cl(x), ops.conv_wino_pack(w), Cout, 1, dil, x_ss=ss, x_relu=True, res=_cl(r), res_ss=rs,
                                  materialize=True)
    assert (mat.permute(0, 3, 1, 2) - inp).abs().max().item() < 1e-5
    err = (y.permute(0, 3, 1, 2) - want).abs().max().item()
    print("[parity] conv_wino_pc 2d fused %d->%d dil%d max|d|=%.3e" % (Cin, Cout, dil, err))
    assert err < 1e-4 * max(1.0, want.abs().max().item())
    s = stats.double().sum(1)
    assert torch.allclose(s[:Cout], want.double().sum((0, 2, 3)), rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("N,H,W,fused", [(1, 16, 16, False), (3, 21, 37, False), (5, 48, 64, True), (2, 19, 35, True), (5, 96, 128, False)])
def test_conv_wino_pc_half_form_32_channels(N, H, W, fused):
    """The HALF form of wino_pc.hip (Cout = 32: firstconv.1/.2 and layer1 of the trunk, psm_submodule.py:90-103) vs F.conv2d in
    float64 — plain, and with the fused prologue (BatchNorm apply + ReLU, residual, materialise); statistics = two rows per tile.
    The fused cases have at most 120 tiles (one per workgroup); the walking regime of the fused HALF forms: tests/test_gpu_wino_pc_walk.py."""
    from neuralrgbd_amd import ops
    C = 32
    g = torch.Generator().manual_seed(N * 100 + H)
    x = torch.randn(N, C, H, W, generator=g).to(DEV)
    w = (torch.randn(C, C, 3, 3, generator=g) * 0.08).to(DEV)
    wp = ops.conv_wino_pack32(w)
    assert ops.conv_wino_supported(N, H, W, C, C, 1)
    if fused:
        r = torch.randn(N, C, H, W, generator=g).to(DEV)
        ss, rs = torch.randn(C, 2, generator=g).to(DEV), torch.randn(C, 2, generator=g).to(DEV)
        inp = torch.relu(x * ss[:, 0].view(1, -1, 1, 1) + ss[:, 1].view(1, -1, 1, 1)) + (r * rs[:, 0].view(1, -1, 1, 1) + rs[:, 1].view(1, -1, 1, 1))
        y, stats, mat = ops.conv_wino(_cl(x), wp, C, 1, 1, x_ss=ss, x_relu=True, res=_cl(r), res_ss=rs, materialize=True)
        assert (mat.permute(0, 3, 1, 2) - inp).abs().max().item() < 1e-5
        y2, _, _ = ops.conv_wino(_cl(x), wp, C, 1, 1, x_ss=ss, x_relu=True, res=_cl(r), res_ss=rs, want_stats=False)   # RES without MAT
        assert torch.equal(y, y2)
    else:
        inp = x
        y, stats, mat = ops.conv_wino(_cl(x), wp, C, 1, 1)
        ym, _, mat2 = ops.conv_wino(_cl(x), wp, C, 1, 1, materialize=True)                                              # MAT without RES
        assert torch.equal(y, ym) and torch.equal(mat2.permute(0, 3, 1, 2), x)
    want = F.conv2d(inp.double(), w.double(), padding=1)
    err = (y.permute(0, 3, 1, 2).double() - want).abs().max().item()
    print("[parity] conv_wino_pc HALF N%d %dx%d fused=%s max|d vs fp64|=%.3e (|y|max %.2f)" % (N, H, W, fused, err, want.abs().max().item()))
    assert y.shape == (N, H, W, C) and err < 2e-5 * max(1.0, want.abs().max().item())
    assert stats.shape == (2 * C, 2 * ops.conv_wino_tiles(N, H, W, 1))
    s = stats.double().sum(1)
    assert torch.allclose(s[:C], want.sum((0, 2, 3)), rtol=1e-5, atol=2e-3)
    assert torch.allclose(s[C:], (want ** 2).sum((0, 2, 3)), rtol=1e-5, atol=2e-3)
    # and against the direct kernel it replaces in the trunk
    yd, _, _ = ops.conv2d(_cl(inp), ops.conv_pack_weights(w), C, 1, want_stats=False)
    assert (yd - y).abs().max().item() < 2e-5 * max(1.0, want.abs().max().item())


def test_bn_finalize_cm_matches_row_major_finaliser():
    """Column-major partials (the Winograd kernel's) through nrgbd_bn_finalize_cm == the same partials through nrgbd_bn_finalize."""
    from neuralrgbd_amd import ops
    g = torch.Generator().manual_seed(3)
    rows, C = 777, 128
    st = torch.randn(rows, 2 * C, generator=g).to(DEV)
    st[:, C:] = st[:, C:].abs() * 50 + 5.0
    gamma, beta = torch.rand(C, generator=g).to(DEV) + 0.5, torch.randn(C, generator=g).to(DEV)
    rm1, rv1 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    rm2, rv2 = rm1.clone(), rv1.clone()
    a = ops.bn_finalize(st, 12345, gamma, beta, 1e-5, 0.1, rm1, rv1)
    b = ops.bn_finalize_cm(st.t().contiguous(), 12345, gamma, beta, 1e-5, 0.1, rm2, rv2)
    # both reduce in float64 (different fixed orders): equal to the last float32 bit or two
    assert torch.allclose(a, b, rtol=1e-6, atol=1e-7) and torch.allclose(rm1, rm2, rtol=1e-6, atol=1e-7) and torch.allclose(rv1, rv2, rtol=1e-6)


# ----------------------------------------------------------------------------- the trunk's stride-2 and 1x1 convolutions (conv2d.hip)
@pytest.mark.parametrize("N,H,W,C,Cout,nchw", [(2, 32, 48, 3, 32, True), (1, 64, 96, 32, 64, False), (3, 18, 34, 3, 32, True)])
def test_conv_stride2_via_space_to_depth_vs_torch(N, H, W, C, Cout, nchw):
    """Stride-2 pad-1 3x3 convolution (psm_submodule.py:90,120) = 2x2-window convolution on the space-to-depth input."""
    from neuralrgbd_amd import ops
    g = torch.Generator().manual_seed(H + C)
    x = torch.randn(N, C, H, W, generator=g).to(DEV)
    w = (torch.randn(Cout, C, 3, 3, generator=g) * 0.1).to(DEV)
    want = F.conv2d(x.double(), w.double(), stride=2, padding=1)
    s2d = ops.space_to_depth2(x if nchw else _cl(x), nchw=nchw)
    assert s2d.shape == (N, H // 2, W // 2, -(-4 * C // 16) * 16)
    y, stats = ops.conv2d_taps(s2d, ops.conv_s2_pack(w), Cout, 4)
    err = (y.permute(0, 3, 1, 2).double() - want).abs().max().item()
    print("[parity] conv stride 2 (s2d) N%d %dx%d %d->%d max|d vs fp64|=%.3e (|y|max %.2f)" % (N, H, W, C, Cout, err, want.abs().max().item()))
    assert err < 2e-5 * max(1.0, want.abs().max().item())
    s = stats.double().sum(0)
    assert torch.allclose(s[:Cout], want.sum((0, 2, 3)), rtol=1e-5, atol=1e-3)
    assert torch.allclose(s[Cout:], (want ** 2).sum((0, 2, 3)), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("N,C,H,W,nchw,cp", [(2, 3, 32, 48, True, None), (5, 3, 18, 34, True, None), (2, 32, 20, 28, False, None),
                                             (1, 8, 6, 10, False, 48), (2, 6, 8, 12, False, None), (2, 5, 8, 12, True, None), (1, 3, 8, 12, True, 32)])
def test_space_to_depth2_every_form(N, C, H, W, nchw, cp):
    """nrgbd_space_to_depth2: the 16-byte forms (planar RGB -> 16 channels, channels-last with C % 4 == 0) and the element-wise kernel
    every other shape takes all give y[n,yo,xo,(py*2+px)*C + c] = x[n,c,2yo+py,2xo+px], zero in the padding channels (pure data movement:
    compared with torch.equal)."""
    from neuralrgbd_amd import ops
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(C * H)).to(DEV)
    got = ops.space_to_depth2(x if nchw else _cl(x), nchw=nchw, cp=cp)
    Cp = got.shape[-1]
    want = torch.zeros(N, H // 2, W // 2, Cp, device=DEV)
    for py in range(2):
        for px in range(2):
            want[..., (py * 2 + px) * C:(py * 2 + px + 1) * C] = x[:, :, py::2, px::2].permute(0, 2, 3, 1)
    assert torch.equal(got, want)


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(5, 24, 32, 128, 32), (2, 3, 4, 128, 32), (2, 33, 47, 64, 128), (1, 40, 56, 32, 64), (1, 20, 20, 128, 64)])
def test_conv_1x1_vs_torch(N, H, W, Cin, Cout):
    """1x1 convolutions of the trunk (shortcuts, SPP branches, head) on the matrix-core kernel, with the loader prologue."""
    from neuralrgbd_amd import ops
    g = torch.Generator().manual_seed(H * 7 + Cin)
    x = torch.randn(N, Cin, H, W, generator=g).to(DEV)
    ss = torch.randn(Cin, 2, generator=g).to(DEV)
    w = (torch.randn(Cout, Cin, 1, 1, generator=g) * 0.1).to(DEV)
    inp = torch.relu(x * ss[:, 0].view(1, -1, 1, 1) + ss[:, 1].view(1, -1, 1, 1))
    want = F.conv2d(inp.double(), w.double())
    y, stats = ops.conv2d_taps(_cl(x), ops.conv_pack_weights(w), Cout, 1, x_ss=ss, x_relu=True)
    err = (y.permute(0, 3, 1, 2).double() - want).abs().max().item()
    print("[parity] conv 1x1 N%d %dx%d %d->%d max|d vs fp64|=%.3e (|y|max %.2f)" % (N, H, W, Cin, Cout, err, want.abs().max().item()))
    assert err < 2e-5 * max(1.0, want.abs().max().item())
    s = stats.double().sum(0)
    assert torch.allclose(s[:Cout], want.sum((0, 2, 3)), rtol=1e-5, atol=1e-3)


def test_spp_concat_vs_torch():
    """nrgbd_spp_concat (BatchNorm + ReLU of the four tiny SPP maps at the taps, bilinear up-sampling with align_corners=True, the
    320-channel concat) vs the torch ops it replaces (psm_submodule.py:149-161), incl. maps of a single row / column."""
    from neuralrgbd_amd import ops
    g = torch.Generator().manual_seed(3)
    for (N, h, w, sizes) in ((2, 24, 40, ((3, 5), (2, 3), (1, 2), (1, 1))), (5, 64, 96, ((8, 12), (4, 6), (2, 3), (1, 1)))):
        quarter = torch.randn(N, h, w, 64, generator=g).to(DEV)
        deep = torch.randn(N, h, w, 128, generator=g).to(DEV)
        br, want = [], [quarter, deep]
        for (bh, bw) in sizes:
            z = torch.randn(N, bh, bw, 32, generator=g).to(DEV)
            ss = torch.randn(32, 2, generator=g).to(DEV)
            br.append((z, ss))
            y = torch.relu(z * ss[:, 0] + ss[:, 1]).permute(0, 3, 1, 2)
            want.append(F.interpolate(y, size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1))
        want = torch.cat(want, dim=3)
        got = ops.spp_concat(quarter, deep, br)
        assert got.shape == want.shape
        assert torch.equal(got[..., :192], want[..., :192])
        err = (got - want).abs().max().item()
        print("[parity] spp_concat %dx%dx%d: max|d| vs torch %.2e" % (N, h, w, err))
        assert err < 2e-6


@pytest.mark.parametrize("N,bh,bw,H,W,C", [(5, 1, 1, 64, 96, 32), (5, 2, 3, 64, 96, 32), (2, 4, 6, 64, 96, 32), (1, 8, 12, 64, 96, 32),
                                           (2, 3, 4, 17, 23, 8), (1, 5, 5, 5, 5, 4), (1, 7, 2, 1, 9, 4), (1, 2, 2, 40, 56, 128), (1, 3, 3, 12, 12, 256)])
def test_upsample_bilinear_align_corners_forward_and_adjoint(N, bh, bw, H, W, C):
    """nrgbd_upsample_bilinear_ac (training path of the SPP branches, psm_submodule.py:153-158) against F.interpolate(bilinear,
    align_corners=True) and ITS autograd backward in float64: forward and the exact adjoint, through autograd.UpsampleBilinearCL."""
    from neuralrgbd_amd.autograd import UpsampleBilinearCL
    g = torch.Generator().manual_seed(N * 100 + bh * 10 + bw)
    x = torch.randn(N, C, bh, bw, generator=g).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gy = torch.randn(N, C, H, W, generator=g).to(DEV)
    y = UpsampleBilinearCL.apply(x, H, W)
    gx, = torch.autograd.grad(y, x, gy)
    x64 = x.detach().double().requires_grad_(True)
    want = F.interpolate(x64, size=(H, W), mode="bilinear", align_corners=True)
    gx64, = torch.autograd.grad(want, x64, gy.double())
    e_f, e_b = (y.double() - want).abs().max().item(), (gx.double() - gx64).abs().max().item()
    print("[parity] upsample (align_corners) %dx%d -> %dx%d C%d: forward max|d| %.2e, adjoint max|d| %.2e (|g|max %.1f)" %
          (bh, bw, H, W, C, e_f, e_b, gx64.abs().max().item()))
    assert e_f < 5e-6 and e_b < 2e-5 * max(1.0, gx64.abs().max().item())
    # <adjoint(gy), x> == <gy, forward(x)> (the kernel pair is an exact adjoint pair up to fp32 summation)
    lhs, rhs = (gx.double() * x.detach().double()).sum().item(), (gy.double() * y.detach().double()).sum().item()
    assert abs(lhs - rhs) < 1e-4 * max(1.0, abs(rhs))


def test_glue_kernels_pool_scatter_strided_pointwise_and_rgb_plane():
    """Round 6: the ATen launches that were left in the inference frame (avg_pool2d, strided copies, a cat) on csrc/glue.hip and as
    options of existing kernels, each against the torch op it replaces (psm_submodule.py:100-117,127-131; Refine.py:88-98;
    KVNET.py:147-158)."""
    from neuralrgbd_amd import ops
    g = torch.Generator().manual_seed(9)
    # channels-last average pooling, incl. a ragged border (floor like avg_pool2d)
    for (N, H, W, C, k) in ((5, 48, 64, 128, 8), (5, 192, 256, 128, 8), (2, 6, 8, 128, 2), (1, 70, 52, 32, 8), (2, 120, 160, 64, 8), (3, 64, 64, 64, 64)):
        x = torch.randn(N, H, W, C, generator=g).to(DEV)
        got = ops.avgpool_cl(x, k)
        want = F.avg_pool2d(x.permute(0, 3, 1, 2).double(), k).permute(0, 2, 3, 1)
        assert tuple(got.shape) == tuple(want.shape) and (got.double() - want).abs().max().item() < 1e-6
    # a strided [C,H,W] view into the channel window of every image of a wider channels-last buffer
    for src in (torch.randn(1, 3, 40, 56, generator=g).to(DEV)[0],                              # NCHW planes (the image)
                torch.randn(1, 20, 28, 32, generator=g).to(DEV).permute(0, 3, 1, 2)[0]):        # NCHW view of channels-last memory
        C, H, W = src.shape
        dst = torch.full((2, H, W, 64 + 48), 7.0, device=DEV)
        ops.scatter_channels(src, dst, 64)
        for r in range(2):
            assert torch.equal(dst[r, :, :, 64:64 + C], src.permute(1, 2, 0))
        assert bool((dst[..., :64] == 7.0).all()) and bool((dst[..., 64 + C:] == 7.0).all())    # the rest of the pixel untouched
    # 1x1 convolution with its own stride: no gather pass (layer2's shortcut)
    x = torch.randn(5, 32, 48, 32, generator=g).to(DEV)
    w = (torch.randn(64, 32, 1, 1, generator=g) * 0.2).to(DEV)
    y, st = ops.conv2d_taps(x, ops.conv_pack_weights(w), 64, 1, stride=2)
    want = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), stride=2).permute(0, 2, 3, 1)
    assert tuple(y.shape) == (5, 16, 24, 64) and (y.double() - want).abs().max().item() < 1e-5
    y1, st1 = ops.conv2d_taps(x[:, ::2, ::2].contiguous(), ops.conv_pack_weights(w), 64, 1)
    assert torch.equal(y, y1) and torch.equal(st, st1)                                           # the bits of the gathered form
    # the pooled-RGB word of the texels as a compact plane, from the same launch
    feat = torch.randn(5, 12, 16, 64, generator=g).to(DEV)
    rgb = torch.randn(5, 3, 48, 64, generator=g).to(DEV)
    tex, rgb4 = ops.pack_nhwc(feat, rgb, channels_last=True, want_rgb4=True)
    assert torch.equal(tex, ops.pack_nhwc(feat, rgb, channels_last=True)) and torch.equal(rgb4, tex[..., 64:].contiguous())
