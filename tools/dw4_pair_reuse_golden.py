#!/usr/bin/env python
"""sha256 digests of wino_dw4.hip's outputs (y and the statistics partials) on the cases of tests/test_gpu_dw4_pair_reuse.py, as JSON.
    python tools/dw4_pair_reuse_golden.py [--lib PATH] [--out FILE]
--lib PATH   another libnrgbd_hip.so: tests/golden/dw4_pair_reuse.json was written with the library of the commit before the
             producers began to keep the t = 2 / t = 4 combinations (built from that commit's wino_dw4.hip)
--out FILE   where to write (default: standard output).  The kernel is deterministic: equal libraries give equal files."""
import importlib.util, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from neuralrgbd_amd import _lib
if "--lib" in sys.argv:
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
spec = importlib.util.spec_from_file_location("dw4_cases", os.path.join(ROOT, "tests", "test_gpu_dw4_pair_reuse.py"))
cases = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cases)
out = {cases.key(s): {f: cases.digests(s, f) for f in cases.FORMS} for s in cases.SHAPES}
text = json.dumps(out, indent=1, sort_keys=True) + "\n"
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(text)
else:
    sys.stdout.write(text)
