"""The R-Net's transposed convolutions (m_submodule.py:36-45 ConvTranspose2d(k4, s2, p1) + bias + LeakyReLU) on the Winograd kernel's
deconv form (csrc/wino_pc.hip, EPI = 2: four sub-pixel phases per launch, the 7 dead transform points of a phase skipped): bit equality
with the unmasked Winograd evaluation, the masks on the packed stream, float64, the refusals, the whole net with the switch on / off."""
import functools

import pytest
import torch
import torch.nn.functional as F

from neuralrgbd_amd import _lib, ops, synth

gpu = pytest.mark.gpu
DEV = "cuda:0"

# input grids: one 8 x 16 tile; 2 x 2 tiles; 2 x 2 tiles of which three cross the lower / right edge; two samples of 3 x 1 tiles
SHAPES = [(1, 8, 16), (1, 16, 32), (1, 10, 18), (2, 24, 16)]
CHANNELS = [(96, 80), (128, 96)]      # (Cin, width of the output buffer): trans_conv1 into the 80-wide, trans_conv0 into the 96-wide concat


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@functools.lru_cache(maxsize=None)
def _case(N, H, W, Cin, ldy):
    """One layer on the three kernels + float64, computed once: NaN-filled [N,2H,2W,ldy] buffers written at ycoff 0, 64 valid columns."""
    x = _rand(N, Cin, H, W, seed=61)
    w = _rand(Cin, 64, 4, 4, seed=62, scale=0.05)
    b = _rand(64, seed=63, scale=0.1)
    want = F.leaky_relu(F.conv_transpose2d(x.double(), w.double(), b.double(), 2, 1), 0.01).permute(0, 2, 3, 1)   # [N,2H,2W,64]
    xc, wd, bd = x.permute(0, 2, 3, 1).contiguous().to(DEV), w.to(DEV), b.to(DEV)
    nan = lambda: torch.full((N, 2 * H, 2 * W, ldy), float("nan"), device=DEV)
    # the unmasked evaluation: the phase-stacked 3x3 weights on the R-Net form, then the pixel shuffle
    stream = ops.conv_wino_pack(ops.deconv_phase_weights(wd))
    y4 = ops.conv_wino_rnet(xc, stream, 256, bias=bd.repeat(4), lrelu=True)
    unmasked = nan()
    unmasked[..., :64] = y4.reshape(N, H, W, 2, 2, 64).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, 64)
    masked = ops.conv_wino_rnet_deconv(xc, ops.conv_wino_rnet_deconv_pack(stream, Cin), nan(), bias=bd, ycoff=0, cout_valid=64)
    packed = []
    for pa in (0, 1):
        for pb in (0, 1):
            ky, kx = ([3, 1] if pa == 0 else [2, 0]), ([3, 1] if pb == 0 else [2, 0])
            packed.append(ops.conv_pack_weights(wd[:, :, ky][:, :, :, kx].permute(1, 0, 2, 3).contiguous()))
    direct = ops.conv2d_rnet(xc, torch.cat(packed), 64, bias=bd, out=nan(), ldy=ldy, ycoff=0, cout_valid=64, mode=3)
    torch.cuda.synchronize()
    return {"want": want, "unmasked": unmasked.cpu(), "masked": masked.cpu(), "direct": direct.cpu()}


@gpu
@pytest.mark.parametrize("Cin,ldy", CHANNELS)
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_bit_equal_to_the_unmasked_winograd_evaluation(N, H, W, Cin, ldy):
    """A product with an exactly zero weight adds exactly nothing: the same bits as ops.conv_wino_rnet on the phase-stacked weights +
    pixel shuffle; the buffer's columns beyond the 64 valid ones keep their NaN."""
    c = _case(N, H, W, Cin, ldy)
    got, ref = c["masked"], c["unmasked"]
    assert bool(torch.isfinite(got[..., :64]).all())
    assert torch.equal(got[..., :64].contiguous().view(torch.int32), ref[..., :64].contiguous().view(torch.int32))
    assert bool(torch.isnan(got[..., 64:]).all())


@gpu
@pytest.mark.parametrize("Cin,ldy", CHANNELS)
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_against_float64(N, H, W, Cin, ldy):
    """vs F.conv_transpose2d + bias + LeakyReLU in float64 on the host.  Bounds: (1) the tolerance every R-Net kernel test uses against
    its reference, 2e-5 max(1, |y|max); (2) max and mean error at most TWICE those of the direct mode-3 kernel on the same inputs.  The
    factor: tests/test_gpu_rnet.py accepts the same 2e-5 max(1, |y|max) from the Winograd forms against float64 and from the direct forms
    against torch's fp32 operator, a reference that carries an error of the direct kernels' own class (the same fp32 products in another
    order); of that tolerance the direct kernel's own error may use half, the Winograd kernel's all of it."""
    c = _case(N, H, W, Cin, ldy)
    want = c["want"]
    e_new = (c["masked"][..., :64].double() - want).abs()
    e_dir = (c["direct"][..., :64].double() - want).abs()
    print("[parity] deconv N%d %dx%d %d->64: vs fp64 max / mean |d|: masked Winograd %.3e / %.3e, direct %.3e / %.3e (|y|max %.2f)"
          % (N, H, W, Cin, e_new.max().item(), e_new.mean().item(), e_dir.max().item(), e_dir.mean().item(), want.abs().max().item()))
    assert e_new.max().item() < 2e-5 * max(1.0, want.abs().max().item())
    assert e_new.max().item() <= 2.0 * e_dir.max().item()
    assert e_new.mean().item() <= 2.0 * e_dir.mean().item()


@pytest.mark.parametrize("Cin", [96, 128])
def test_dropped_lines_of_the_unmasked_stream_are_zero(Cin):
    """Host: of the 256-column stream of the phase-stacked weights every line the masked stream leaves out is exactly zero (random
    weights), and no kept line is: the masks are the zero pattern of U = G g G^T."""
    w = _rand(Cin, 64, 4, 4, seed=71)
    U = ops.conv_wino_pack_reference(ops.deconv_phase_weights(w)).reshape(4, Cin // 16, 16, 1024)   # [phase][stage][point][line]
    for ph in range(4):
        live = ops.deconv_live_points(ph)
        assert len(live) == 9
        dead = [xi for xi in range(16) if xi not in live]
        assert bool((U[ph][:, dead] == 0).all())
        assert bool((U[ph][:, live] != 0).any(dim=-1).all())


@gpu
def test_device_packer_copies_the_live_lines():
    Cin = 96
    stream = ops.conv_wino_pack(ops.deconv_phase_weights(_rand(Cin, 64, 4, 4, seed=72).to(DEV)))
    got = ops.conv_wino_rnet_deconv_pack(stream, Cin).reshape(4, Cin // 16, 9, 1024)
    U = stream.reshape(4, Cin // 16, 16, 1024)
    for ph in range(4):
        assert torch.equal(got[ph], U[ph][:, ops.deconv_live_points(ph)])


@gpu
def test_refusals():
    """Every refusal returns its code before anything is launched (the buffers are far too small for the shapes named)."""
    x, wm, y, b = (torch.zeros(4096, device=DEV) for _ in range(4))
    lib = _lib.load()
    p = lambda t: t.data_ptr()

    def call(Cin=96, Cout=64, ldy=80, ycoff=0, valid=64, xoff=0, woff=0, yoff=0):
        return lib.nrgbd_conv_wino_rnet_deconv_f32(p(x) + xoff, p(wm) + woff, p(b), 1, p(y) + yoff, 1, 8, 16, Cin, Cout, ldy, ycoff, valid, None)
    assert call(Cin=40) == -2 and call(Cin=16) == -2 and call(Cin=80) == -2      # not whole 16-channel stages / one stage / an odd count
    assert call(Cout=128) == -2 and call(Cout=32) == -2
    assert call(ldy=60) == -4 and call(ldy=80, ycoff=32) == -4 and call(valid=65) == -4
    assert call(xoff=4) == -3 and call(woff=8) == -3 and call(yoff=2) == -3
    assert lib.nrgbd_conv_wino_rnet_deconv_f32(None, p(wm), p(b), 1, p(y), 1, 8, 16, 96, 64, 80, 0, 64, None) == -1
    torch.cuda.synchronize()
    assert bool((y == 0).all())


@gpu
def test_whole_net_switch_on_against_off():
    """forward_log at D = 64 on a 16 x 32 quarter grid with the transposed convolutions on the deconv form and on the direct kernel:
    both within the whole-net parity tolerance (tests/test_gpu_rnet.py) of the float64 module graph, and of each other."""
    import copy
    from neuralrgbd_amd import nets
    h, w, D = 16, 32, 64
    net = nets.DPVUpsampleNet(64, 32, 3, D=D)
    net.load_state_dict(synth.seeded_state_dict(net, 3))
    net = net.to(DEV)
    dpv_log = torch.log_softmax(_rand(1, D, h, w, seed=10, scale=3.0), dim=1).to(DEV)
    feats = [_rand(1, 64, h, w, seed=11).to(DEV), _rand(1, 32, 2 * h, 2 * w, seed=12).to(DEV), _rand(1, 3, 4 * h, 4 * w, seed=13).to(DEV)]
    with torch.no_grad():
        ref = copy.deepcopy(net).cpu().double()
        mod = ref(torch.exp(dpv_log).cpu().double(), [f.cpu().double() for f in feats]).float().to(DEV)
        out = {}
        for first in ("wino", "direct"):
            net.deconv_kernels = (first, "direct")
            out[first] = net.forward_log(dpv_log, feats).clone()
    assert not torch.equal(out["wino"], out["direct"])          # the switch switches
    for k, v in out.items():
        e = (v - mod).abs()
        print("[parity] whole R-Net, deconv on %s vs the module graph in float64: max %.2e mean %.2e" % (k, e.max().item(), e.mean().item()))
        assert e.mean().item() < 1e-5 and e.max().item() < 2e-4
        assert int((v.argmax(1) != mod.argmax(1)).sum()) <= 2
    d = (out["wino"] - out["direct"]).abs()
    assert d.mean().item() < 1e-5 and d.max().item() < 2e-4
