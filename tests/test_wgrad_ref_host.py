"""tests/wgrad_ref.py (the float64 comparators of the gradient kernels) against float64 torch.autograd of F.conv3d / F.conv2d on tiny
ragged grids, and the property the exact GPU tests rest on: on {-1, 0, 1} operands the fp32 evaluation equals the float64 one.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

import wgrad_ref as ref

TOL = dict(rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("D,H,W,Ci,Co", [(1, 1, 1, 2, 3), (3, 5, 7, 4, 6), (2, 9, 4, 16, 5)])
def test_wgrad3d_vs_float64_autograd(D, H, W, Ci, Co):
    g = torch.Generator().manual_seed(D * 100 + W)
    x = torch.randn(D, H, W, Ci, generator=g, dtype=torch.float64)
    gy = torch.randn(D, H, W, Co, generator=g, dtype=torch.float64)
    w = torch.zeros(Co, Ci, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x.permute(3, 0, 1, 2)[None], w, padding=1)[0]
    (want,) = torch.autograd.grad(y, w, gy.permute(3, 0, 1, 2))
    got = ref.wgrad3d(x, gy)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert torch.allclose(got, want, **TOL)


@pytest.mark.parametrize("N,H,W,Ci,Co,dil", [(1, 1, 1, 2, 3, 1), (2, 5, 7, 4, 6, 1), (2, 5, 7, 4, 6, 2), (3, 2, 9, 16, 5, 2), (1, 9, 3, 3, 16, 1)])
def test_wgrad2d_vs_float64_autograd(N, H, W, Ci, Co, dil):
    g = torch.Generator().manual_seed(N * 100 + W + dil)
    x = torch.randn(N, H, W, Ci, generator=g, dtype=torch.float64)
    gy = torch.randn(N, H, W, Co, generator=g, dtype=torch.float64)
    w = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, None, 1, dil, dil)
    (want,) = torch.autograd.grad(y, w, gy.permute(0, 3, 1, 2))
    got = ref.wgrad2d(x, gy, dil)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert torch.allclose(got, want, **TOL)


@pytest.mark.parametrize("D,H,W", [(1, 1, 1), (3, 5, 7), (2, 9, 4)])
def test_c1_gradients_vs_float64_autograd(D, H, W):
    g = torch.Generator().manual_seed(D * 100 + W)
    x = torch.randn(D, H, W, 64, generator=g, dtype=torch.float64)
    gy = torch.randn(D, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(1, 64, 3, 3, 3, generator=g, dtype=torch.float64)
    x1, w1 = x.permute(3, 0, 1, 2)[None].clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv3d(x1, w1, padding=1)[0, 0]
    want_x, want_w = torch.autograd.grad(y, (x1, w1), gy)
    got_w, got_x = ref.c1_wgrad(x, gy), ref.c1_dgrad(gy, w)
    assert got_w.shape == (1, 64, 3, 3, 3) and got_x.shape == (D, H, W, 64)
    assert torch.allclose(got_w, want_w, **TOL)
    assert torch.allclose(got_x, want_x[0].permute(1, 2, 3, 0), **TOL)


def test_integer_operands_make_fp32_equal_float64():
    """{-1, 0, 1} operands: every partial sum is an integer below 2^24, so fp32 and float64 evaluate the references to the same numbers
    in any summation order — the premise of the bit-for-bit GPU tests (there the kernel stands in for the fp32 evaluation)."""
    D, H, W = 5, 10, 40
    x, gy, g1, w = ref.integer_operands(3, (D, H, W, 64), (D, H, W, 64), (D, H, W), (1, 64, 3, 3, 3))
    assert ref.exact_3d(D, H, W) and ref.exact_sum(D * H * W)
    assert set(x.unique().tolist()) == {-1.0, 0.0, 1.0} and x.dtype == torch.float32
    pairs = [(ref.wgrad3d(x, gy, torch.float32), ref.wgrad3d(x, gy)),
             (ref.wgrad2d(x, gy, 1, torch.float32), ref.wgrad2d(x, gy, 1)),
             (ref.wgrad2d(x, gy, 2, torch.float32), ref.wgrad2d(x, gy, 2)),
             (ref.c1_wgrad(x, g1, torch.float32), ref.c1_wgrad(x, g1)),
             (ref.c1_dgrad(g1, w, torch.float32), ref.c1_dgrad(g1, w))]
    for lo, hi in pairs:
        assert lo.dtype == torch.float32 and hi.dtype == torch.float64
        assert float(hi.abs().max()) > 0 and torch.equal(hi, hi.round())         # integers, and not all zero
        assert torch.equal(lo, hi.float()) and torch.equal(lo.double(), hi)
    a, b = ref.integer_operands(3, (4, 4)), ref.integer_operands(3, (4, 4))       # seeded: the same draw every time
    assert torch.equal(a[0], b[0])
    n1, n2 = ref.normal_operands(4, (4, 4)), ref.normal_operands(4, (4, 4))
    assert torch.equal(n1[0], n2[0]) and n1[0].dtype == torch.float32
