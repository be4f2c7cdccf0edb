#!/usr/bin/env python
"""SHA-256 digests of the outputs of the producer/consumer Winograd kernel (csrc/wino_pc.hip), of its weight packer and of the
column-major BatchNorm finaliser, for a before/after comparison of two libraries on one device (one process per library): y,
stats and, where it exists, the materialised input, from seeded inputs.  The kernels are deterministic, so equal libraries print
equal lines.  The shapes are small and together reach all 21 instantiations of conv_wino_pc_kernel.
--lib PATH          another libnrgbd_hip.so (e.g. one built from the parent commit)"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from neuralrgbd_amd import _lib
if "--lib" in sys.argv:
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
import torch
from neuralrgbd_amd import ops
DEV = torch.device("cuda")
sha = lambda *ts: "  ".join("-" * 32 if t is None else hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:32] for t in ts)
FIVE = ("plain", "x_ss+relu", "res+res_ss+relu", "materialise", "res+materialise")
# (kd, dilation, Cin, Cout, (N, H, W), forms)
CASES = [
    (1, 1, 64, 64, (2, 19, 35), FIVE), (1, 1, 64, 128, (2, 24, 40), ("plain",)), (1, 1, 320, 128, (1, 16, 32), ("plain",)),   # 128: two column groups; 320: 20 stages
    (1, 2, 128, 128, (2, 19, 35), FIVE), (1, 2, 128, 128, (1, 5, 7), FIVE),                                                  # 5 x 7: smaller than a tile
    (1, 1, 32, 32, (2, 19, 35), FIVE), (1, 1, 32, 32, (5, 96, 128), ("plain",)),                                              # HALF; 480 tiles: a second tile per workgroup
    (3, 1, 64, 64, (5, 16, 32), FIVE), (3, 1, 64, 64, (6, 13, 21), ("plain",)), (3, 1, 64, 64, (64, 24, 32), ("plain",)),     # ragged edges; 384 tiles
    (3, 1, 16, 64, (5, 16, 32), ("plain",)), (3, 1, 16, 64, (64, 24, 32), ("plain",)),                                        # odd stage count, first and second tile
]
# EPI = 1: (Cin, cout, cout_valid, ycoff, ldy, (N, H, W))
RNET = [(128, 128, 128, 0, 128, (2, 24, 40)), (80, 64, 64, 0, 64, (1, 19, 35)), (80, 32, 3, 64, 96, (1, 19, 35)), (96, 32, 20, 8, 96, (1, 19, 35))]


def gen(seed):
    g = torch.Generator().manual_seed(seed)
    return g, (lambda *s: torch.randn(*s, generator=g))


print("library %s" % _lib.LIB_PATH)
for Cin in (64, 16, 128):                                               # weight streams of Cin -> 64 layers, 2-D and 3-D
    g, r = gen(Cin)
    for taps in ((3, 3), (3, 3, 3)):
        for tr in ((0, 1, 2) if Cin % 64 == 0 else (0, 1)):              # 2 (both streams in one launch) needs Cin % 64 == 0
            w = (r(*((Cin, 64) if tr == 1 else (64, Cin)), *taps) * 0.05).to(DEV)   # 1: the stored tensor is [Cin][Cout]
            print("pack kd=%d %3d->64 transposed=%d  %s" % (len(taps) == 3 and 3 or 1, Cin, tr, sha(ops.conv_wino_pack(w, tr))))
g, r = gen(7)
print("pack32 32->32  %s" % sha(ops.conv_wino_pack32((r(32, 32, 3, 3) * 0.05).to(DEV))))
stats_keep = None
for kd, dil, Cin, Cout, (N, H, W), forms in CASES:
    g, r = gen(1000 * N + H + Cin + 7 * kd + dil)
    ss = lambda: torch.stack((0.5 + torch.rand(Cin, generator=g), 0.2 * r(Cin)), 1).contiguous().to(DEV)
    x, res, xs, rs = r(N, H, W, Cin).to(DEV), r(N, H, W, Cin).to(DEV), ss(), ss()
    w = (r(Cout, Cin, *((3, 3, 3) if kd == 3 else (3, 3))) * 0.05).to(DEV)
    wp = ops.conv_wino_pack32(w) if Cout == 32 else ops.conv_wino_pack(w)
    kws = {"plain": {}, "x_ss+relu": dict(x_ss=xs, x_relu=True), "res+res_ss+relu": dict(x_ss=xs, x_relu=True, res=res, res_ss=rs, res_relu=True),
           "materialise": dict(x_ss=xs, x_relu=True, materialize=True), "res+materialise": dict(x_ss=xs, x_relu=True, res=res, materialize=True)}
    for name in forms:
        y, st, mat = ops.conv_wino(x, wp, Cout, kd, dil, **kws[name])
        print("pc kd=%d dil=%d %3d->%-3d %-10s %-16s y stats mat  %s" % (kd, dil, Cin, Cout, "%dx%dx%d" % (N, H, W), name, sha(y, st, mat)))
        if stats_keep is None:
            stats_keep = (st.clone(), Cout, N * H * W)
for Cin, cout, valid, ycoff, ldy, (N, H, W) in RNET:
    g, r = gen(Cin + cout + valid)
    x, b = r(N, H, W, Cin).to(DEV), (r(cout) * 0.2).to(DEV)
    w = (r(cout, Cin, 3, 3) * 0.05).to(DEV)
    wp = ops.conv_wino_pack32(w) if cout == 32 else ops.conv_wino_pack(w)
    for lrelu in (True, False):
        out = torch.full((N, H, W, ldy), 7.0, device=DEV)                # the whole buffer is digested: the sentinel columns count
        ops.conv_wino_rnet(x, wp, cout, bias=b, lrelu=lrelu, out=out, ycoff=ycoff, cout_valid=valid)
        print("rnet %3d->%-3d valid=%-3d ycoff=%-2d ldy=%-3d %-10s lrelu=%d  %s" % (Cin, cout, valid, ycoff, ldy, "%dx%dx%d" % (N, H, W), lrelu, sha(out)))
st, C, count = stats_keep
g, r = gen(3)
gamma, beta = (1.0 + 0.1 * r(C)).to(DEV), (0.1 * r(C)).to(DEV)
rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
ssout = ops.bn_finalize_cm(st, count, gamma, beta, 1e-5, 0.1, rm, rv)
print("bn_finalize_cm C=%d rows=%d  scale_shift running_mean running_var  %s" % (C, st.shape[1], sha(ssout, rm, rv)))
