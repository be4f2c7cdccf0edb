#!/usr/bin/env python
"""SHA-256 digests of the bit-deterministic outputs of the cost-volume backward, for a before/after comparison of two libraries on
one device (one process per library): g_ref and g_src of the deterministic path (L2 and L1, both align_corners values) and g_ref
of the LDS path (register sums in candidate order + the fixed-order reduce).  g_src of the atomic kernels and g_ref of the
global-atomic kernel depend on the order of the atomics: not digested, tests/test_gpu_costvol_bwd.py holds them to the comparator.
--lib PATH          another libnrgbd_hip.so (e.g. one built from the parent commit)"""
import ctypes, hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from neuralrgbd_amd import _lib
if "--lib" in sys.argv:
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
from neuralrgbd_amd import ops
import costvol_bwd_exact as cx
from costvol_bwd_gpu import _run
CASES = [(64, 96, 64, 4, 67, "driver"),                                  # the training shape
         (33, 47, 6, 2, 5, "large"), (9, 11, 6, 2, 3, "small"),          # LDS shapes, ragged last channel word
         (97, 131, 33, 2, 6, "driver"), (96, 128, 9, 4, 67, "driver")]   # beyond the LDS budget
sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()[:32]
print("library %s" % _lib.LIB_PATH)
for h, w, D, V, C, family in CASES:
    case = cx.make_case(h, w, D, V, C, family)
    name = "%dx%dx%d V%d C%d %s" % (h, w, D, V, C, family)
    n = ctypes.c_size_t(0)
    _lib.check(_lib.load().nrgbd_costvol_bwd_workspace(V, ops.padded_channels(C), D, h, w, ctypes.byref(n)), "workspace query")
    for dist in ("L2", "L1"):
        for align in (False, True):
            g_ref, g_src = _run(case, dist, align, deterministic=True)
            print("%-28s det %s align=%d  g_ref %s  g_src %s" % (name, dist, align, sha(g_ref), sha(g_src)))
            if n.value:                                                  # the LDS path
                print("%-28s lds %s align=%d  g_ref %s" % (name, dist, align, sha(_run(case, dist, align)[0])))
