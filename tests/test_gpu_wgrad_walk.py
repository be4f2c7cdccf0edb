"""The four persistent gradient kernels where a workgroup walks SEVERAL tiles of its list — the regime of every real training window (the
K-Net grid 64x64x96 gives conv3d_wgrad 24 tiles per range), which no other test reaches: csrc/conv3d_wgrad.hip (128 tile ranges),
csrc/conv2d_wgrad.hip (clamp(1820 / blocks, 64, 1024) workgroups per weight block) and both kernels of csrc/conv3d_c1_bwd.hip (512 / 2,048
workgroups), called directly through ops at the grids of tests/wgrad_ref.py — the smallest that walk, ragged on every axis that can be.

Per grid:  guard    the launcher's own host query says workgroups < tiles (tests/test_host.py asserts the same without a GPU);
           exact    operands from {-1, 0, 1}: every partial sum is exactly representable in fp32 in any order, so the kernel must equal
                    the float64 reference BIT FOR BIT — a dropped, doubled or wrongly masked tile, a stale LDS halo, an accumulator not
                    carried across the loop or a partial left out of the reduction cannot hide behind a tolerance;
           parity   seeded normal operands against the float64 reference, e = max|kernel - ref64| / max|ref64|;
           twice    a second call returns identical bits (each kernel's file header: no atomics, bitwise reproducible).
The references run in float64 on the host; tests/test_wgrad_ref_host.py holds them against float64 autograd."""
import numpy as np
import pytest
import torch

import wgrad_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _diff_report(got, want, weights=True):
    """On {-1, 0, 1} operands a difference per (co, ci, tap) is an integer = voxels counted wrongly: say how many entries differ, the
    largest and where, and the summed |difference| per tap (a lost tile shows in every tap, a halo fault only in the shifted ones)."""
    d = got.detach().double().cpu() - want.double().cpu()
    nz = int((d != 0).sum())
    if nz == 0:
        return "identical"
    flat = int(d.abs().argmax())
    idx = tuple(int(i) for i in np.unravel_index(flat, tuple(d.shape)))
    msg = "%d of %d entries differ; largest %+g at %s (want %g)" % (nz, d.numel(), float(d.reshape(-1)[flat]), idx, float(want.reshape(-1)[flat]))
    if weights:                                          # [Co][Ci][taps...]
        taps = d.reshape(d.shape[0], d.shape[1], -1).abs().sum((0, 1))
        msg += "; sum|d| per tap " + " ".join("%g" % float(t) for t in taps)
    return msg


def _rel(got, want64):
    return float((got.detach().double().cpu() - want64).abs().max() / want64.abs().max())


def _guard(nwg, tiles, want_tiles):
    assert tiles == want_tiles and 0 < nwg < tiles, "nothing walks any more: %d workgroups, %d tiles" % (nwg, tiles)


# ---- conv3d_wgrad.hip ---------------------------------------------------------------------------------------------------------------

def _guard_3d(D, H, W, tiles):
    from neuralrgbd_amd import _lib
    _guard(_lib.load().nrgbd_conv3d_wgrad_ranges(), ref.tiles_3d(D, H, W), tiles)


@pytest.mark.parametrize("D,H,W,Cin,tiles", ref.WALK_3D)
def test_conv3d_wgrad_walk_exact(D, H, W, Cin, tiles):
    """Integer operands, bit for bit.  325 tiles: ranges of 3 and of 2 tiles in one launch (the priority schedule q = 4 it / my_tiles
    differs between workgroups); 512: four tiles each, every priority quarter; Cin 16 and 32: the other two instantiations, whose idle
    waves `continue` inside the loop (Cin 16) and whose quadrant list is halved (Cin 32)."""
    from neuralrgbd_amd import ops
    _guard_3d(D, H, W, tiles)
    assert ref.exact_3d(D, H, W)
    x, gy = ref.integer_operands(1000 + W + Cin, (D, H, W, Cin), (D, H, W, 64))
    want = ref.wgrad3d(x, gy)
    assert torch.equal(want, want.round()) and float(want.abs().max()) > 0
    xd, gd = x.to(DEV), gy.to(DEV)
    got, again = ops.conv3d_wgrad(xd, gd), ops.conv3d_wgrad(xd, gd)
    assert got.shape == (64, Cin, 3, 3, 3) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want.float()), _diff_report(got, want)
    assert torch.equal(got, again)


@pytest.mark.parametrize("D,H,W,Cin,tiles", ref.WALK_3D)
def test_conv3d_wgrad_walk_parity(D, H, W, Cin, tiles):
    """Normal operands against float64.  The project had no float64 bound for this kernel, so the yardstick is measured beside it:
    e_plain, the error of the plain 27-matmul reference evaluated in fp32 on the device, and the kernel may be R_WINO times worse.
    R_WINO = twice the largest e / e_plain measured on the MI355X over the four grids, rounded up to a power of two (the rule that
    introduced it allowed up to 16: the transforms of gy and x and the final G^T . G each cost about a factor two in rounding).
    Measured (e, e_plain, ratio; identical in two runs):
        9x18x200 Cin 64   3.362e-07  3.476e-06  0.0967
        8x16x512 Cin 64   4.603e-07  4.595e-06  0.1002
        9x18x200 Cin 16   3.453e-07  1.381e-06  0.2500
        5x10x264 Cin 32   2.990e-07  3.817e-06  0.0783        -> R_WINO = 0.5
    The ratios are below one because the yardstick is ten times worse on the device than on the host (3.6e-7 .. 4.0e-7 there): the vendor
    GEMM adds a tap's 32,400 .. 65,536 voxels in one chain per output, the kernel adds at most four tiles into an accumulator and reduces
    128 partials in eight interleaved slices.  The kernel's own e is what a plain fp32 evaluation reaches on the host."""
    from neuralrgbd_amd import ops
    _guard_3d(D, H, W, tiles)
    x, gy = ref.normal_operands(2000 + W + Cin, (D, H, W, Cin), (D, H, W, 64))
    want = ref.wgrad3d(x, gy)
    xd, gd = x.to(DEV), gy.to(DEV)
    got, again = ops.conv3d_wgrad(xd, gd), ops.conv3d_wgrad(xd, gd)
    e, e_plain = _rel(got, want), _rel(ref.wgrad3d(xd, gd, torch.float32), want)
    print("[parity] conv3d_wgrad walk %dx%dx%d Cin=%d (%d tiles): e %.3e  e_plain %.3e  ratio %.4f (R %g)" %
          (D, H, W, Cin, tiles, e, e_plain, e / e_plain, ref.R_WINO))
    assert e_plain > 0
    assert e <= ref.R_WINO * e_plain
    assert torch.equal(got, again)


# ---- conv2d_wgrad.hip ---------------------------------------------------------------------------------------------------------------

def _guard_2d(N, H, W, Cin, Cout, nwg, tiles):
    from neuralrgbd_amd import _lib
    got = _lib.load().nrgbd_conv2d_wgrad_workgroups(N, H, W, Cin, Cout)
    assert got == nwg, (got, nwg)
    _guard(got, ref.tiles_2d(N, H, W), tiles)


@pytest.mark.parametrize("N,H,W,Cin,Cout,dil,nwg,tiles", ref.WALK_2D)
def test_conv2d_wgrad_walk_exact(N, H, W, Cin, Cout, dil, nwg, tiles):
    """Integer operands, bit for bit: one block at the 1,024 cap, ten blocks at 182, dilation 2, and the 32- and 16-wide last blocks
    whose idle waves `continue` inside a multi-trip loop; the reduction runs over a full list of 1,024 / 182 / 455 / 303 partials."""
    from neuralrgbd_amd import ops
    _guard_2d(N, H, W, Cin, Cout, nwg, tiles)
    assert ref.exact_sum(N * H * W)
    x, gy = ref.integer_operands(3000 + W + Cin, (N, H, W, Cin), (N, H, W, Cout))
    want = ref.wgrad2d(x, gy, dil)
    assert float(want.abs().max()) > 0
    xd, gd = x.to(DEV), gy.to(DEV)
    got, again = ops.conv2d_wgrad(xd, gd, dil), ops.conv2d_wgrad(xd, gd, dil)
    assert got.shape == (Cout, Cin, 3, 3) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want.float()), _diff_report(got, want)
    assert torch.equal(got, again)


@pytest.mark.parametrize("N,H,W,Cin,Cout,dil,nwg,tiles", ref.WALK_2D)
def test_conv2d_wgrad_walk_parity(N, H, W, Cin, Cout, dil, nwg, tiles):
    """Normal operands against float64 at the bound of test_gpu_train.py::test_conv2d_autograd_function_vs_fp64 (5e-6 of max|ref|)."""
    from neuralrgbd_amd import ops
    _guard_2d(N, H, W, Cin, Cout, nwg, tiles)
    x, gy = ref.normal_operands(4000 + W + Cin, (N, H, W, Cin), (N, H, W, Cout))
    want = ref.wgrad2d(x, gy, dil)
    xd, gd = x.to(DEV), gy.to(DEV)
    got, again = ops.conv2d_wgrad(xd, gd, dil), ops.conv2d_wgrad(xd, gd, dil)
    e = _rel(got, want)
    print("[parity] conv2d_wgrad walk %dx%dx%d %d->%d dil %d (%d workgroups, %d tiles): e %.3e" % (N, H, W, Cin, Cout, dil, nwg, tiles, e))
    assert e < 5e-6
    assert torch.equal(got, again)


# ---- conv3d_c1_bwd.hip --------------------------------------------------------------------------------------------------------------

def _guard_c1(D, H, W, dgrad, nwg, tiles):
    from neuralrgbd_amd import _lib
    got = _lib.load().nrgbd_conv3d_cout1_bwd_workgroups(D, H, W, dgrad)
    assert got == nwg, (got, nwg)
    _guard(got, ref.tiles_2d(D, H, W), tiles)


def _tap_major(w):
    return w[0].reshape(64, 27).t().contiguous()


def test_conv3d_cout1_wgrad_walk_exact_and_parity():
    """600 tiles on 512 workgroups: 88 of them carry their 27 x 4 running sums across two tiles (ragged H: 36 = 4 tiles + 4 rows; ragged W:
    88 = 5 tiles + 8 columns), and the reduction reads a full list of 512 partials.  Integer operands bit for bit; normal operands at
    2e-5 of max|ref| (test_conv3d_cout1_three_directions_vs_torch_autograd's bound)."""
    from neuralrgbd_amd import ops
    D, H, W, nwg, tiles = ref.WALK_C1_WGRAD
    _guard_c1(D, H, W, 0, nwg, tiles)
    assert ref.exact_sum(D * H * W)
    x, gy = ref.integer_operands(5000, (D, H, W, 64), (D, H, W))
    want = ref.c1_wgrad(x, gy)
    assert float(want.abs().max()) > 0
    xd, gd = x.to(DEV), gy.to(DEV)
    got, again = ops.conv3d_cout1_wgrad(xd, gd), ops.conv3d_cout1_wgrad(xd, gd)
    assert got.shape == (1, 64, 3, 3, 3) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want.float()), _diff_report(got, want)
    assert torch.equal(got, again)
    x, gy = ref.normal_operands(5001, (D, H, W, 64), (D, H, W))
    want = ref.c1_wgrad(x, gy)
    xd, gd = x.to(DEV), gy.to(DEV)
    got, again = ops.conv3d_cout1_wgrad(xd, gd), ops.conv3d_cout1_wgrad(xd, gd)
    e = _rel(got, want)
    print("[parity] conv3d_cout1_wgrad walk %dx%dx%d (%d workgroups, %d tiles): e %.3e" % (D, H, W, nwg, tiles, e))
    assert e < 2e-5
    assert torch.equal(got, again)


def test_conv3d_cout1_dgrad_walk_exact_and_parity():
    """2,340 tiles on 2,048 workgroups: 292 of them stage a second halo of gy behind the loop-top barrier and store a second tile.
    Integer gy AND integer weights: the whole gx bit for bit (27 terms of magnitude <= 1); normal operands at 2e-6 of max|ref|."""
    from neuralrgbd_amd import ops
    D, H, W, nwg, tiles = ref.WALK_C1_DGRAD
    _guard_c1(D, H, W, 1, nwg, tiles)
    gy, w = ref.integer_operands(6000, (D, H, W), (1, 64, 3, 3, 3))
    want = ref.c1_dgrad(gy, w)
    assert float(want.abs().max()) > 0 and float(want.abs().max()) <= 27
    gd, wd = gy.to(DEV), _tap_major(w).to(DEV)
    got, again = ops.conv3d_cout1_dgrad(gd, wd), ops.conv3d_cout1_dgrad(gd, wd)
    assert got.shape == (D, H, W, 64) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want.float()), _diff_report(got, want, weights=False)
    assert torch.equal(got, again)
    gy, w = ref.normal_operands(6001, (D, H, W), (1, 64, 3, 3, 3))
    want = ref.c1_dgrad(gy, w)
    gd, wd = gy.to(DEV), _tap_major(w).to(DEV)
    got, again = ops.conv3d_cout1_dgrad(gd, wd), ops.conv3d_cout1_dgrad(gd, wd)
    e = _rel(got, want)
    print("[parity] conv3d_cout1_dgrad walk %dx%dx%d (%d workgroups, %d tiles): e %.3e" % (D, H, W, nwg, tiles, e))
    assert e < 2e-6
    assert torch.equal(got, again)
