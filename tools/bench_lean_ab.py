"""bench.py with the form of the K-Net residual passes in the pipelined back half taken from the environment: LEAN_PASSES = workgroups
per CU of the co-resident form (streaming.DepthStream.lean_passes; 0 = the plain pass, which is the frame as it was before the
co-resident form existed; unset = the shipped value).  Every other argument goes to bench.py.  For A/B series alternated run by run
in one session (profiles/pass_overlap.txt):  LEAN_PASSES=0 python tools/bench_lean_ab.py --gpus 1 --steps 20 --warmup 5"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuralrgbd_amd import streaming
if os.environ.get("LEAN_PASSES", "") != "":
    streaming.DepthStream.lean_passes = int(os.environ["LEAN_PASSES"])
sys.argv[0] = os.path.join(ROOT, "bench.py")
runpy.run_path(sys.argv[0], run_name="__main__")
