#!/usr/bin/env python
"""Return codes of refused calls of wino_pc.hip's six C entries, for a before/after comparison of two libraries:
    python tools/wino_pc_refusals.py [--lib PATH]          one line per call; diff the output of the two libraries
Runs on a host WITHOUT a GPU only: the pointers are made up.  Every call is refused by the entry's own checks before any launch; the
three marked 'after the CU query' are refused behind nrgbd_conv_wino_f32's device query and return the runtime's no-device code here."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
if os.path.exists("/dev/kfd"):
    sys.exit("wino_pc_refusals.py passes made-up pointers: run it on a host without a GPU")
from neuralrgbd_amd import _lib
if "--lib" in sys.argv:
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
L = _lib.load()
P = ctypes.c_void_p(0x10000)      # stands for any non-null pointer: never dereferenced by a refused call
calls = []


def variants(fname, base, changes):
    """base: dict of named arguments in signature order; changes: (label, {name: value}) -> one refused call each."""
    for label, ch in changes:
        args = dict(base)
        args.update(ch)
        calls.append(("%s  %s" % (fname, label), fname, list(args.values())))


BIG = 1 << 15
conv = dict(x=P, x_ss=None, x_relu=0, res=None, res_ss=None, res_relu=0, mat=None, w=P, y=P, stats=None, N=2, H=19, W=35, Cin=64, Cout=64, kd=1, dil=1, stream=None)
variants("nrgbd_conv_wino_f32", conv, [("x null", dict(x=None)), ("w_wino null", dict(w=None)), ("y null", dict(y=None)), ("all null", dict(x=None, w=None, y=None)),
    ("N=0", dict(N=0)), ("N=-1", dict(N=-1)), ("H=0", dict(H=0)), ("W=0", dict(W=0)), ("W=-3", dict(W=-3)), ("Cin=0", dict(Cin=0)), ("Cin=24", dict(Cin=24)),
    ("Cin=2064", dict(Cin=2064)), ("Cout=0", dict(Cout=0)), ("Cout=48", dict(Cout=48)), ("Cout=96", dict(Cout=96)), ("Cout=-64", dict(Cout=-64)),
    ("kd=0", dict(kd=0)), ("kd=2", dict(kd=2)), ("dil=0", dict(dil=0)), ("dil=3", dict(dil=3)), ("kd=3 dil=2", dict(kd=3, dil=2)),
    ("Cout=32 kd=3", dict(Cout=32, kd=3)), ("Cout=32 dil=2", dict(Cout=32, dil=2)), ("Cout=32 Cin=16", dict(Cout=32, Cin=16)),
    ("one stage", dict(Cin=16)), ("Cin=24 kd=2", dict(Cin=24, kd=2)), ("N*H*W*Cin >= 2^30", dict(N=1, H=BIG, W=BIG // 2, Cin=64)),
    ("kd=3 H*W*Cin >= 2^30", dict(kd=3, N=4, H=8192, W=8192, Cin=16)), ("tiles = 2^30", dict(kd=3, N=1 << 24, H=8, W=16, Cin=16, Cout=4096)),
    ("odd stages kd=1 (after the CU query)", dict(Cin=48)), ("odd stages kd=3 + res (after the CU query)", dict(kd=3, Cin=16, res=P)),
    ("odd stages kd=3 + materialise (after the CU query)", dict(kd=3, Cin=16, mat=P))])
rn = dict(x=P, w=P, bias=None, lrelu=1, y=P, N=1, H=19, W=35, Cin=80, Cout=64, ldy=0, ycoff=0, valid=0, stream=None)
variants("nrgbd_conv_wino_rnet_ex_f32", rn, [("x null", dict(x=None)), ("w_wino null", dict(w=None)), ("y null", dict(y=None)), ("N=0", dict(N=0)), ("H=0", dict(H=0)),
    ("W=0", dict(W=0)), ("H=-19", dict(H=-19)), ("Cin=16", dict(Cin=16)), ("Cin=0", dict(Cin=0)), ("Cin=40", dict(Cin=40)), ("Cout=0", dict(Cout=0)), ("Cout=96", dict(Cout=96)),
    ("Cout=16", dict(Cout=16)), ("N*H*W*Cin >= 2^30", dict(H=BIG, W=BIG // 2, Cin=64)), ("cout_valid=-1", dict(valid=-1)), ("cout_valid=65", dict(valid=65)),
    ("Cout=32 cout_valid=33", dict(Cout=32, valid=33)), ("ycoff=-1", dict(ycoff=-1)), ("ldy=63", dict(ldy=63)), ("ldy=66 ycoff=64 valid=3", dict(Cout=32, ldy=66, ycoff=64, valid=3)),
    ("ldy=70 ycoff=8", dict(ldy=70, ycoff=8)), ("N*H*W*ldy = 2^32", dict(H=4096, W=4096, Cin=32, ldy=256))])
variants("nrgbd_conv_wino_rnet_f32", {k: v for k, v in rn.items() if k not in ("ldy", "ycoff", "valid")}, [("x null", dict(x=None)), ("w_wino null", dict(w=None)),
    ("y null", dict(y=None)), ("N=0", dict(N=0)), ("H=0", dict(H=0)), ("W=0", dict(W=0)), ("Cin=16", dict(Cin=16)), ("Cin=40", dict(Cin=40)), ("Cout=96", dict(Cout=96)),
    ("N*H*W*Cin >= 2^30", dict(H=BIG, W=BIG // 2, Cin=64))])
pk = dict(w=P, wp=P, Cin=64, Cout=64, kd=1, tr=0, stream=None)
variants("nrgbd_conv_wino_pack", pk, [("w null", dict(w=None)), ("w_wino null", dict(wp=None)), ("Cin=0", dict(Cin=0)), ("Cin=24", dict(Cin=24)), ("Cout=0", dict(Cout=0)),
    ("Cout=32", dict(Cout=32)), ("Cout=96", dict(Cout=96)), ("kd=0", dict(kd=0)), ("kd=2", dict(kd=2)), ("transposed=-1", dict(tr=-1)), ("transposed=3", dict(tr=3)),
    ("transposed=2 Cin=16", dict(tr=2, Cin=16)), ("transposed=2 Cin=80 kd=3", dict(tr=2, Cin=80, kd=3))])
tl = dict(N=2, H=19, W=35, dil=1)
variants("nrgbd_conv_wino_tiles", tl, [("N=0", dict(N=0)), ("H=0", dict(H=0)), ("W=-1", dict(W=-1)), ("dil=0", dict(dil=0)), ("dil=3", dict(dil=3)),
    ("2x19x35 (a count, host only)", {}), ("1x5x7 dil=2 (a count, host only)", dict(N=1, H=5, W=7, dil=2)), ("64x24x32 (a count, host only)", dict(N=64, H=24, W=32))])
bn = dict(stats=P, rows=12, C=64, count=100, gamma=P, beta=P, eps=1e-5, mom=0.1, rm=P, rv=P, ss=P, cc=None, nbt=None, stream=None)
variants("nrgbd_bn_finalize_cm", bn, [("stats null", dict(stats=None)), ("gamma null", dict(gamma=None)), ("beta null", dict(beta=None)), ("scale_shift null", dict(ss=None)),
    ("rows=0", dict(rows=0)), ("rows=-2", dict(rows=-2)), ("C=0", dict(C=0)), ("count=0", dict(count=0)), ("count=-5", dict(count=-5)),
    ("running_mean alone", dict(rv=None)), ("running_var alone", dict(rm=None))])

print("library %s" % _lib.LIB_PATH)
for label, fname, args in calls:
    print("%-78s -> %d" % (label, getattr(L, fname)(*args)))
print("%d calls" % len(calls))
