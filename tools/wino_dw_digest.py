#!/usr/bin/env python
"""SHA-256 digests of the outputs of the two depth-Winograd kernels (csrc/wino_dw.hip, csrc/wino_dw4.hip) and of their weight
packers, for a before/after comparison of two libraries on one device (one process per library): y, stats and, where it exists,
the materialised input, from seeded inputs.  Both kernels are deterministic, so equal libraries print equal lines.
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
DW = [(2, 8, 16, 64), (6, 24, 48, 64), (8, 16, 32, 16), (8, 40, 224, 64)]                      # [D,H,W,Cin]; the last: 560 tiles
DW4 = [(4, 8, 16, 64), (8, 24, 48, 64), (8, 16, 32, 16), (4, 16, 32, 128), (16, 40, 224, 64)]  # the last: 280 tiles > CUs
sha = lambda *ts: "  ".join("-" * 32 if t is None else hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:32] for t in ts)


def inputs(D, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(D * 1000 + H + Cin)
    r = lambda *s: torch.randn(*s, generator=g)
    ss = lambda: torch.stack((0.5 + torch.rand(Cin, generator=g), 0.2 * r(Cin)), 1).contiguous().to(DEV)
    return r(D, H, W, Cin).to(DEV), r(D, H, W, Cin).to(DEV), (r(Cout, Cin, 3, 3, 3) * 0.05).to(DEV), ss(), ss()


print("library %s" % _lib.LIB_PATH)
for Cin in (64, 16, 128):                                              # weight streams of Cin -> 64 layers: both packers
    g = torch.Generator().manual_seed(Cin)
    for name, pack in (("dw", ops.conv_wino_dw_pack), ("dw4", ops.conv_wino_dw4_pack)):
        for tr in ((0, 1, 2) if Cin % 64 == 0 else (0, 1)):             # 2 (both streams in one launch) needs Cin % 64 == 0
            w = (torch.randn(*((Cin, 64) if tr == 1 else (64, Cin)), 3, 3, 3, generator=g) * 0.05).to(DEV)   # 1: the forward weight
            print("pack %-3s %3d->64 transposed=%d  %s" % (name, Cin, tr, sha(pack(w, tr))))
for D, H, W, Cin in DW:
    x, res, w, xs, rs = inputs(D, H, W, Cin, 64)
    wp, wpu, k = ops.conv_wino_dw_pack(w), ops.conv_wino_dw_pack(w * 64.0), 2.0 ** -6
    forms = [("plain", {}), ("x_ss+relu", dict(x_ss=xs, x_relu=True)), ("res", dict(x_ss=xs, x_relu=True, res=res)),
             ("res_ss+relu", dict(x_ss=xs, x_relu=True, res=res, res_ss=rs, res_relu=True)),
             ("materialise", dict(x_ss=xs, x_relu=True, materialize=True)),
             ("res+materialise", dict(x_ss=xs, x_relu=True, res=res, materialize=True)), ("x_unit", dict(x_ss=xs, x_relu=True, x_unit=k))]
    for name, kw in forms:                                              # "plain" without (scale, shift) is the IDENT instantiation
        y, st, mat = ops.conv_wino_dw(x, wpu if "x_unit" in kw else wp, 64, **kw)
        print("dw  %-16s %-16s y stats mat  %s" % ("%dx%dx%dx%d" % (D, H, W, Cin), name, sha(y, st, mat)))
for D, H, W, Cin in DW4:
    Cout = 128 if Cin == 128 else 64
    x, _, w, xs, _ = inputs(D, H, W, Cin, Cout)
    wp, wpu, k = ops.conv_wino_dw4_pack(w), ops.conv_wino_dw4_pack(w * 64.0), 2.0 ** -6
    for name, kw in [("ident", {}), ("x_ss+relu", dict(x_ss=xs, x_relu=True)), ("x_unit", dict(x_ss=xs, x_relu=True, x_unit=k))]:
        y, st = ops.conv_wino_dw4(x, wpu if "x_unit" in kw else wp, Cout, **kw)
        print("dw4 %-16s %-16s y stats      %s" % ("%dx%dx%dx%d" % (D, H, W, Cin), name, sha(y, st)))
