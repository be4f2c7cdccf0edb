#!/usr/bin/env python
"""Return codes of refused calls of the seven C entries of wino_dw.hip / wino_dw4.hip, for a before/after comparison of two libraries:
    python tools/wino_dw_refusals.py [--lib PATH]          one line per call; diff the output of the two libraries
Runs on a host WITHOUT a GPU only: the pointers are made up (tools/wino_pc_refusals.py is the same for wino_pc.hip).  Every call is
refused by the entry's own checks before any launch; those marked 'after the CU query' pass them and are stopped by the entry's
device query, which returns the runtime's no-device code here — among them the short workspace of nrgbd_conv_wino_dw4_f32."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
if os.path.exists("/dev/kfd"):
    sys.exit("wino_dw_refusals.py passes made-up pointers: run it on a host without a GPU")
from neuralrgbd_amd import _lib
if "--lib" in sys.argv:
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
L = _lib.load()
P = ctypes.c_void_p(0x10000)      # stands for any non-null, 16-byte aligned pointer: never dereferenced by a refused call
calls = []


def variants(fname, base, changes):
    """base: dict of named arguments in signature order; changes: (label, {name: value}) -> one refused call each."""
    for label, ch in changes:
        args = dict(base)
        args.update(ch)
        calls.append(("%s  %s" % (fname, label), fname, list(args.values())))


shapes = [("N=0", dict(N=0)), ("N=-2", dict(N=-2)), ("H=0", dict(H=0)), ("W=0", dict(W=0)), ("W=-16", dict(W=-16)), ("H=13", dict(H=13)), ("W=24", dict(W=24)),
          ("Cin=0", dict(Cin=0)), ("Cin=24", dict(Cin=24)), ("Cin=528", dict(Cin=528)), ("Cout=0", dict(Cout=0)), ("Cout=32", dict(Cout=32)), ("Cout=96", dict(Cout=96)),
          ("Cout=-64", dict(Cout=-64)), ("H*W*Cin = 2^30", dict(H=8192, W=8192, Cin=16)), ("tiles = 2^31", dict(N=1 << 19, H=8, W=16, Cin=16, Cout=1 << 19))]
pk = dict(w=P, wp=P, Cin=64, Cout=64, tr=0, stream=None)
for f in ("nrgbd_conv_wino_dw_pack", "nrgbd_conv_wino_dw4_pack"):
    variants(f, pk, [("w null", dict(w=None)), ("w_wino null", dict(wp=None)), ("Cin=0", dict(Cin=0)), ("Cin=24", dict(Cin=24)), ("Cin=-16", dict(Cin=-16)),
        ("Cout=0", dict(Cout=0)), ("Cout=32", dict(Cout=32)), ("Cout=96", dict(Cout=96)), ("transposed=-1", dict(tr=-1)), ("transposed=3", dict(tr=3)),
        ("transposed=2 Cin=16", dict(tr=2, Cin=16)), ("transposed=2 Cin=80", dict(tr=2, Cin=80))])
wg = dict(N=4, H=16, W=32, Cout=64)
variants("nrgbd_conv_wino_dw_workgroups", wg, [("N=0", dict(N=0)), ("N=3", dict(N=3)), ("N=-2", dict(N=-2)), ("H=0", dict(H=0)), ("W=0", dict(W=0)), ("Cout=0", dict(Cout=0)),
    ("Cout=32", dict(Cout=32)), ("Cout=96", dict(Cout=96)), ("4x16x32 (after the CU query)", {})])
nbytes = ctypes.c_size_t(0)
ws = dict(N=4, H=16, W=32, Cout=64, bytes=ctypes.byref(nbytes))
variants("nrgbd_conv_wino_dw4_workspace", ws, [("bytes null", dict(bytes=None)), ("N=0", dict(N=0)), ("N=2", dict(N=2)), ("N=6", dict(N=6)), ("H=0", dict(H=0)), ("W=-1", dict(W=-1)),
    ("Cout=0", dict(Cout=0)), ("Cout=96", dict(Cout=96)), ("4x16x32 (after the CU query)", {})])
dw = dict(x=P, x_ss=None, x_relu=0, res=None, res_ss=None, res_relu=0, mat=None, w=P, y=P, stats=None, N=4, H=16, W=32, Cin=64, Cout=64, stream=None)
variants("nrgbd_conv_wino_dw_f32", dw, [("x null", dict(x=None)), ("w_wino null", dict(w=None)), ("y null", dict(y=None)), ("all null", dict(x=None, w=None, y=None)),
    ("N=3", dict(N=3)), ("N=5 res", dict(N=5, res=P))] + shapes + [("4x16x32 plain (after the CU query)", {}), ("4x16x32 res + materialise (after the CU query)", dict(res=P, mat=P))])
un = dict(x=P, x_ss=P, unit=0.25, w=P, y=P, stats=None, N=4, H=16, W=32, Cin=64, Cout=64, stream=None)
variants("nrgbd_conv_wino_dw_unit_f32", un, [("x_ss null", dict(x_ss=None)), ("x null", dict(x=None)), ("w_wino null", dict(w=None)), ("y null", dict(y=None)),
    ("x_unit=0", dict(unit=0.0)), ("x_unit=-0.5", dict(unit=-0.5)), ("x_unit=2", dict(unit=2.0)), ("x_unit=0.3", dict(unit=0.3)), ("x_unit=0.75", dict(unit=0.75)),
    ("x_unit=nan", dict(unit=float("nan"))), ("x_unit=0.3 and x null", dict(unit=0.3, x=None)), ("N=3", dict(N=3))] + shapes + [("x_unit=1 (after the CU query)", dict(unit=1.0))])
d4 = dict(x=P, x_ss=None, x_relu=0, unit=0.0, w=P, y=P, stats=None, ws=P, ws_bytes=1 << 30, N=4, H=16, W=32, Cin=64, Cout=64, stream=None)
variants("nrgbd_conv_wino_dw4_f32", d4, [("x null", dict(x=None)), ("w_wino null", dict(w=None)), ("y null", dict(y=None)), ("workspace null", dict(ws=None)),
    ("N=2", dict(N=2)), ("N=6", dict(N=6))] + shapes + [("workspace misaligned by 4", dict(ws=ctypes.c_void_p(0x10004))), ("workspace misaligned by 8", dict(ws=ctypes.c_void_p(0x10008))),
    ("misaligned and N=6", dict(ws=ctypes.c_void_p(0x10004), N=6)), ("x_unit=0.25 without x_ss", dict(unit=0.25, x_relu=1)), ("x_unit=0.25 without x_relu", dict(unit=0.25, x_ss=P)),
    ("x_unit=0.3", dict(unit=0.3, x_ss=P, x_relu=1)), ("x_unit=2", dict(unit=2.0, x_ss=P, x_relu=1)), ("x_unit=0.3 and misaligned", dict(unit=0.3, x_ss=P, x_relu=1, ws=ctypes.c_void_p(0x10004))),
    ("workspace of 0 bytes (after the CU query)", dict(ws_bytes=0)), ("workspace of 16 bytes (after the CU query)", dict(ws_bytes=16))])

print("library %s" % _lib.LIB_PATH)
for label, fname, args in calls:
    print("%-84s -> %d" % (label, getattr(L, fname)(*args)))
print("%d calls" % len(calls))
