"""csrc/wino_dw4.hip's producers form the depth combinations of t = 2 and t = 4 in the stages of t = 1 and t = 3 (same four input
slices, other coefficients) and keep them in registers for the partner stage.  Every FMA chain keeps its order, so the output is
the one the kernel gave when each phase loaded and activated its units afresh:
  * same bits: sha256 of y and of the statistics partials against tests/golden/dw4_pair_reuse.json, written by the library of the
    commit before the change (tools/dw4_pair_reuse_golden.py, which runs this module's cases);
  * accuracy against float64 F.conv3d, tolerance of test_gpu_knet.py::test_conv_wino_dw4_plain_vs_torch;
  * no dependence on what the output and workspace buffers held before the launch.
Shapes [D, H, W, Cin] and what each can break:
  [4, 8, 16, 16]    one tile, both outside slices, one channel block: the kept set is read in the very next stage
  [8, 16, 32, 32]   two channel blocks
  [12, 24, 16, 64]  an interior depth tile, four blocks (serpentine order), plane-edge masks
  [8, 96, 192, 64]  288 tiles: some workgroups walk two, the kept sets and the prefetch cross a tile boundary"""
import ctypes
import hashlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dw4_pair_reuse.json")
SHAPES = [(4, 8, 16, 16), (8, 16, 32, 32), (12, 24, 16, 64), (8, 96, 192, 64)]
FORMS = ["ident", "clamp", "relu_ss"]
UNIT = 2.0 ** -3
_cache = {}


def key(shape):
    return "%dx%dx%dx%d" % shape


def operands(shape):
    """Seeded x [D,H,W,Cin], w [64,Cin,3,3,3], (scale, shift) [Cin,2]: built once per shape and left unchanged.  relu(x * s + t)
    stays below 1 / UNIT = 8, where the clamped form is the plain ReLU."""
    if shape not in _cache:
        D, H, W, Cin = shape
        g = torch.Generator().manual_seed(D * 1000 + H + Cin)
        x = torch.randn(D, H, W, Cin, generator=g).clamp_(-4.0, 4.0)
        w = torch.randn(64, Cin, 3, 3, 3, generator=g) * 0.05
        ss = torch.stack((0.5 + torch.rand(Cin, generator=g), 0.2 * torch.randn(Cin, generator=g).clamp_(-4.0, 4.0)), 1).contiguous()
        _cache[shape] = (x.to(DEV), w.to(DEV), ss.to(DEV))
    return _cache[shape]


def run(shape, form):
    """-> (y [D,H,W,64], stats [128, tiles]) of one input form through ops.conv_wino_dw4"""
    from neuralrgbd_amd import ops
    x, w, ss = operands(shape)
    if form == "ident":
        return ops.conv_wino_dw4(x, ops.conv_wino_dw4_pack(w), 64)
    if form == "clamp":
        return ops.conv_wino_dw4(x, ops.conv_wino_dw4_pack(w / UNIT), 64, x_ss=ss, x_relu=True, x_unit=UNIT)
    return ops.conv_wino_dw4(x, ops.conv_wino_dw4_pack(w), 64, x_ss=ss, x_relu=True)


def digests(shape, form):
    y, stats = run(shape, form)
    sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    return {"y": sha(y), "stats": sha(stats)}


def reference(shape, form):
    """float64 F.conv3d of the form's input, channels first [64, D, H, W]; once per (shape, form)"""
    k = (shape, form)
    if k not in _cache:
        x, w, ss = operands(shape)
        xin = x.double()
        if form != "ident":
            xin = torch.relu(xin * ss[:, 0].double() + ss[:, 1].double())
        _cache[k] = F.conv3d(xin.permute(3, 0, 1, 2)[None], w.double(), padding=1)[0]
    return _cache[k]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=key)
def test_same_bits_as_before_the_pairing(shape, form):
    with open(GOLDEN) as f:
        want = json.load(f)[key(shape)][form]
    assert digests(shape, form) == want


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=key)
def test_against_float64(shape, form):
    from neuralrgbd_amd import ops
    x, w, ss = operands(shape)
    want = reference(shape, form)
    y, stats = run(shape, form)
    kw = {} if form == "ident" else dict(x_ss=ss, x_relu=True)
    y2, _, _ = ops.conv_wino_dw(x, ops.conv_wino_dw_pack(w), 64, **kw)                  # F(2, 3) along depth: the A/B of the bound
    err = (y.permute(3, 0, 1, 2).double() - want).abs()
    err2 = (y2.permute(3, 0, 1, 2).double() - want).abs()
    scale = want.abs().max().item()
    print("[parity] dw4 pair reuse %s %s: max|d vs fp64| %.3e mean %.3e  (wino_dw: %.3e / %.3e; |y|max %.2f)" %
          (key(shape), form, err.max().item(), err.mean().item(), err2.max().item(), err2.mean().item(), scale))
    assert err.max().item() < 4e-5 * max(1.0, scale) and err.mean().item() < 3.0 * err2.mean().item() + 1e-9
    s = stats.double().sum(1)
    assert torch.allclose(s[:64], want.sum((1, 2, 3)), rtol=1e-5, atol=2e-3)
    assert torch.allclose(s[64:], (want ** 2).sum((1, 2, 3)), rtol=1e-5, atol=2e-3)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=key)
def test_no_stale_data_dependence(shape, form):
    """The C entry on buffers the test owns: y, the statistics and the workspace start as NaN; twice, same result, all finite."""
    from neuralrgbd_amd import _lib, ops
    x, w, ss = operands(shape)
    D, H, W, Cin = shape
    clamp = form == "clamp"
    wp = ops.conv_wino_dw4_pack(w / UNIT if clamp else w)
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    _lib.check(lib.nrgbd_conv_wino_dw4_workspace(D, H, W, 64, ctypes.byref(nbytes)), "nrgbd_conv_wino_dw4_workspace")
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    out = []
    for _ in range(2):
        y = torch.full((D, H, W, 64), float("nan"), device=DEV)
        stats = torch.full((128, ops.conv_wino_tiles(D, H, W, 1)), float("nan"), device=DEV)
        ws = torch.full((nbytes.value // 4,), float("nan"), device=DEV)
        with torch.cuda.device(x.device):
            rc = lib.nrgbd_conv_wino_dw4_f32(p(x), p(None if form == "ident" else ss), int(form != "ident"), float(UNIT if clamp else 0.0),
                                             p(wp), p(y), p(stats), p(ws), ctypes.c_size_t(nbytes.value), D, H, W, Cin, 64,
                                             ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
        _lib.check(rc, "nrgbd_conv_wino_dw4_f32")
        out.append((y, stats))
    assert torch.isfinite(out[0][0]).all() and torch.isfinite(out[0][1]).all()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    y0, st0 = run(shape, form)
    assert torch.equal(out[0][0], y0) and torch.equal(out[0][1], st0)
