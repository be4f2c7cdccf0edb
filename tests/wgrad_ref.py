"""Plain float64 references of the four persistent gradient kernels (csrc/conv3d_wgrad.hip, csrc/conv2d_wgrad.hip and the two of
csrc/conv3d_c1_bwd.hip), written from the formulas in the kernels' headers as shifted views and matmuls in torch, on whatever device the
operands live; `dtype` evaluates the same expression in another precision (the fp32 yardstick of the parity tests).
tests/test_wgrad_ref_host.py holds them against float64 torch.autograd on the CPU; tests/test_gpu_wgrad_walk.py holds the kernels against
them at the grids below, the smallest at which a workgroup walks more than one tile of its list.

Operands drawn from {-1, 0, 1} make every product and every partial sum of all four kernels a small integer (quarter-integers after the
Winograd kernel's G^T . G), exactly representable in fp32 in any summation order while the bound of `exact_3d` / `exact_sum` holds: the
float64 result cast to fp32 then equals the kernel's output bit for bit."""
import torch
import torch.nn.functional as F

# conv3d_wgrad.hip: 2 x 4 x 16-voxel tiles, 128 tile ranges.  (D, H, W, Cin, tiles)
WALK_3D = [
    (9, 18, 200, 64, 325),    # ranges with 3 and with 2 tiles in one launch (my_tiles differs); ragged D, H, W
    (8, 16, 512, 64, 512),    # exactly 4 tiles each: every priority quarter; whole tiles
    (9, 18, 200, 16, 325),    # conv3d_wgrad_kernel<16>
    (5, 10, 264, 32, 153),    # conv3d_wgrad_kernel<32> with two quadrants: ranges with 2 and with 1 tile
]
# conv2d_wgrad.hip: 8 x 16-pixel tiles, workgroups per weight block = clamp(1820 / blocks, 64, 1024).
# (N, H, W, Cin, Cout, dilation, workgroups, tiles)
WALK_2D = [
    (5, 120, 224, 64, 64, 1, 1024, 1050),
    (1, 44, 520, 320, 128, 1, 182, 198),
    (2, 60, 472, 128, 128, 2, 455, 480),
    (2, 52, 360, 96, 160, 1, 303, 322),     # 32-wide last blocks: idle waves `continue` inside the loop
    (2, 60, 472, 80, 80, 1, 455, 480),      # 16-wide last blocks
]
# conv3d_c1_bwd.hip: 8 x 16-voxel tiles of one slice.  (D, H, W, workgroups, tiles)
WALK_C1_WGRAD = (20, 36, 88, 512, 600)
WALK_C1_DGRAD = (130, 20, 88, 2048, 2340)

# conv3d_wgrad.hip against float64 has no fixed bound: with e = max|kernel - ref64| / max|ref64| and e_plain the same statistic for
# wgrad3d evaluated in fp32 on the device, the tests hold e <= R_WINO * e_plain.  R_WINO = twice the largest e / e_plain measured on the
# MI355X over the four grids of WALK_3D, rounded up to a power of two, and by the rule that introduced it never above 16 (the transforms
# of gy and x and the final G^T . G each cost about a factor two in rounding).  Measured: 0.097, 0.100, 0.250, 0.078 — the figures and why
# they are below one are in the docstring of tests/test_gpu_wgrad_walk.py::test_conv3d_wgrad_walk_parity.
R_WINO = 0.5


def _cdiv(a, b):
    return -(-a // b)


def tiles_3d(D, H, W):
    return _cdiv(D, 2) * _cdiv(H, 4) * _cdiv(W, 16)


def tiles_2d(N, H, W):
    return N * _cdiv(H, 8) * _cdiv(W, 16)


def exact_3d(D, H, W):
    """conv3d_wgrad on {-1, 0, 1}: |Z| <= 4 and |V| <= 4, a point sums at most D H W / 4 products of magnitude <= 16, and G^T . G
    combines 16 points with two fraction bits: 64 D H W < 2^24 keeps every intermediate exact in fp32."""
    return 64 * D * H * W < 2 ** 24


def exact_sum(n):
    """a sum of n products of {-1, 0, 1} operands is exact in fp32 in any order while n < 2^24"""
    return n < 2 ** 24


def integer_operands(seed, *shapes):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-1, 2, s, generator=g).float() for s in shapes]


def normal_operands(seed, *shapes):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) for s in shapes]


def wgrad3d(x, gy, dtype=torch.float64):
    """x [D,H,W,Ci], gy [D,H,W,Co] -> dW [Co,Ci,3,3,3]:  dW[co][ci][kd][kh][kw] = sum_v gy[v][co] x[v + (kd,kh,kw) - 1][ci], x zero
    outside the volume — 27 matmuls on the zero-padded x."""
    D, H, W, Ci = x.shape
    Co = gy.shape[-1]
    xp = F.pad(x.to(dtype), (0, 0, 1, 1, 1, 1, 1, 1))
    g = gy.to(dtype).reshape(-1, Co).t()
    dw = torch.empty((Co, Ci, 3, 3, 3), dtype=dtype, device=x.device)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                dw[:, :, kd, kh, kw] = g @ xp[kd:kd + D, kh:kh + H, kw:kw + W].reshape(-1, Ci)
    return dw


def wgrad2d(x, gy, dilation=1, dtype=torch.float64):
    """x [N,H,W,Ci], gy [N,H,W,Co] -> dW [Co,Ci,3,3]:  dW[co][ci][kh][kw] = sum_(n,v) gy[n][v][co] x[n][v + ((kh,kw) - 1) dilation][ci]"""
    N, H, W, Ci = x.shape
    Co = gy.shape[-1]
    d = int(dilation)
    xp = F.pad(x.to(dtype), (0, 0, d, d, d, d))
    g = gy.to(dtype).reshape(-1, Co).t()
    dw = torch.empty((Co, Ci, 3, 3), dtype=dtype, device=x.device)
    for kh in range(3):
        for kw in range(3):
            dw[:, :, kh, kw] = g @ xp[:, kh * d:kh * d + H, kw * d:kw * d + W].reshape(-1, Ci)
    return dw


def c1_wgrad(x, gy, dtype=torch.float64):
    """Conv3d(64, 1): x [D,H,W,64], gy [D,H,W] -> dW [1,64,3,3,3]"""
    return wgrad3d(x, gy[..., None], dtype)


def c1_dgrad(gy, w, dtype=torch.float64):
    """Conv3d(64, 1): gy [D,H,W], w [1,64,3,3,3] -> gx [D,H,W,64]:  gx[v][ci] = sum_tap gy[v - (tap - 1)] w[0][ci][tap], gy zero outside
    the volume — the 27 shifted copies of gy as the columns of one matrix, times the tap-major weights."""
    D, H, W = gy.shape
    gp = F.pad(gy.to(dtype), (1, 1, 1, 1, 1, 1))
    cols = torch.stack([gp[2 - kd:2 - kd + D, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W].reshape(-1)
                        for kd in range(3) for kh in range(3) for kw in range(3)], 1)
    return (cols @ w.to(dtype)[0].reshape(w.shape[1], 27).t()).reshape(D, H, W, w.shape[1])
