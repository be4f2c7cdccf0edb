#!/usr/bin/env python
"""Launch times of the Winograd kernels at the path's own shapes (HIP events, one process per library), for an alternated
parent / new comparison:  python tools/wino_time.py [--lib PATH] [--dw] [--only SUBSTRING] [--out FILE]
wino_pc.hip: the feature CNN's trunk, dilated, 320 -> 128 and HALF layers at config B, the R-Net's 80 -> 64 and 128 -> 128 blocks
at both of its resolutions, the K-Net's any-grid fallback (kd = 3) plain and with residual + materialise.
--dw: every launched form of wino_dw.hip (plain, IDENT, CLAMP, res, res + materialise, identity res + materialise, materialise) and of
wino_dw4.hip (IDENT, plain, CLAMP), 64 -> 64 at the K-Net's grid, instead.
Per shape: warm-up, then 5 windows of at least 0.25 s each; prints the median window's mean in us and the windows' range."""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from neuralrgbd_amd import _lib
if "--lib" in sys.argv:
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
import torch
from neuralrgbd_amd import ops
DEV = torch.device("cuda")
r = lambda *s: torch.randn(*s, device=DEV)


def timed(fn):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(n):
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n
    n = max(10, int(math.ceil(0.25e6 / window(10))))
    ws = sorted(window(n) for _ in range(5))
    return ws[2], ws[0], ws[4], n


def direct(fname, keep, *args):        # the C entry on buffers allocated once: a launch costs next to no host work
    f = getattr(_lib.load(), fname)
    args = [a.data_ptr() if torch.is_tensor(a) else a for a in args] + [torch.cuda.current_stream().cuda_stream]

    def go(keep=keep):
        _lib.check(f(*args), fname)
    return go


def pc(name, N, H, W, Cin, Cout, kd=1, dil=1, res=False, mat=False):
    x, w = r(N, H, W, Cin), r(Cout, Cin, *((3, 3, 3) if kd == 3 else (3, 3))) * 0.05
    wp = ops.conv_wino_pack32(w) if Cout == 32 else ops.conv_wino_pack(w)
    ss = torch.stack((0.5 + torch.rand(Cin, device=DEV), 0.2 * r(Cin)), 1).contiguous()
    rs = r(N, H, W, Cin) if res else None
    y, st, m = ops.conv_wino(x, wp, Cout, kd, dil, x_ss=ss, x_relu=True, res=rs, materialize=mat)
    return name, direct("nrgbd_conv_wino_f32", (x, wp, ss, rs, y, st, m), x, ss, 1, rs, None, 0, m, wp, y, st, N, H, W, Cin, Cout, kd, dil)


def rnet(name, N, H, W, Cin, Cout):
    x, wp, b = r(N, H, W, Cin), ops.conv_wino_pack(r(Cout, Cin, 3, 3) * 0.05), r(Cout)
    out = torch.empty(N, H, W, Cout, device=DEV)
    return name, direct("nrgbd_conv_wino_rnet_ex_f32", (x, wp, b, out), x, wp, b, 1, out, N, H, W, Cin, Cout, Cout, 0, Cout)


def dw(name, four, **kw):             # kw: the form, as keyword arguments of ops.conv_wino_dw / ops.conv_wino_dw4
    x, w = r(64, 192, 256, 64), r(64, 64, 3, 3, 3) * 0.05
    ss = torch.stack((0.5 + torch.rand(64, device=DEV), 0.2 * r(64)), 1).contiguous()
    if kw.pop("ss", False):
        kw.update(x_ss=ss, x_relu=True)
    if "x_unit" in kw:                  # the CLAMP forms: the weight stream carries 1 / x_unit
        w = w / kw["x_unit"]
    if kw.pop("res", False):
        kw["res"] = r(64, 192, 256, 64)
    if kw.pop("res_ss", False):         # else the residual operand comes as it is (the RSID instantiations)
        kw.update(res_ss=torch.stack((0.5 + torch.rand(64, device=DEV), 0.2 * r(64)), 1).contiguous(), res_relu=True)
    if four:
        wp = ops.conv_wino_dw4_pack(w)
        return name, lambda: ops.conv_wino_dw4(x, wp, 64, **kw)
    wp = ops.conv_wino_dw_pack(w)
    return name, lambda: ops.conv_wino_dw(x, wp, 64, **kw)


# every launched form of the two depth-Winograd kernels at 64 -> 64 @ 64x192x256
DW = [("dw  plain", False, dict(ss=True)), ("dw  IDENT", False, {}), ("dw  CLAMP", False, dict(ss=True, x_unit=2.0 ** -6)),
      ("dw  res", False, dict(ss=True, res=True, res_ss=True)), ("dw  res+mat", False, dict(ss=True, res=True, res_ss=True, materialize=True)),
      ("dw  RSID res+mat", False, dict(ss=True, res=True, materialize=True)), ("dw  mat", False, dict(ss=True, materialize=True)),
      ("dw4 IDENT", True, {}), ("dw4 plain", True, dict(ss=True)), ("dw4 CLAMP", True, dict(ss=True, x_unit=2.0 ** -6))]
CASES = [(n + " 64->64 @64x192x256", lambda n, four=four, kw=kw: dw(n, four, **kw)) for n, four, kw in DW] if "--dw" in sys.argv else [
    ("trunk 64->64 @5x192x256", lambda n: pc(n, 5, 192, 256, 64, 64)), ("128->128 dil 2 @5x64x96", lambda n: pc(n, 5, 64, 96, 128, 128, dil=2)),
    ("320->128 @5x64x96", lambda n: pc(n, 5, 64, 96, 320, 128)), ("HALF 32->32 @5x384x512", lambda n: pc(n, 5, 384, 512, 32, 32)),
    ("R-Net 80->64 @2x768x1024", lambda n: rnet(n, 2, 768, 1024, 80, 64)), ("R-Net 128->128 @2x768x1024", lambda n: rnet(n, 2, 768, 1024, 128, 128)),
    ("R-Net 80->64 @2x192x256", lambda n: rnet(n, 2, 192, 256, 80, 64)), ("R-Net 128->128 @2x192x256", lambda n: rnet(n, 2, 192, 256, 128, 128)),
    ("K-Net 64->64 kd=3 @64x192x256 plain", lambda n: pc(n, 64, 192, 256, 64, 64, kd=3)),
    ("K-Net 64->64 kd=3 @64x192x256 res+mat", lambda n: pc(n, 64, 192, 256, 64, 64, kd=3, res=True, mat=True))]
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None
for name, build in CASES:
    if only not in name:
        continue
    name, fn = build(name)
    med, lo, hi, n = timed(fn)
    line = "%-40s %10.2f us  (windows %.2f .. %.2f, %d launches each)" % (name, med, lo, hi, n)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()
    del fn
    torch.cuda.empty_cache()
