#!/bin/bash
# The measurements of DESIGN.md row f12: tools/bench_raycast.py per call, then one rocprofv3 kernel trace per form (a run of its own
# each), the per-call kernel time and launch count of every trace, then the streams at config B.  Every GPU step has its own time
# limit and the chain stops at the first step that fails.     tools/bench_raycast.sh <output directory>
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
O=${1:?usage: tools/bench_raycast.sh <output directory>}
mkdir -p "$O" || exit 1
trace() {   # grid, size, form, extra flag
    timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/tr_$3_$1_$2$4" -- \
        python tools/bench_raycast.py --trace-only --grid "$1" --size "$2" --form "$3" $4 > "$O/tr_$3_$1_$2$4.log" 2>&1
}
timeout -k 10 300 python tools/bench_raycast.py --json "$O/bench_raycast.json" 2>&1 | tee "$O/bench_raycast.log" &&
trace 256 768x1024 hip && trace 256 768x1024 hip --normals && trace 256 256x384 hip && trace 128 768x1024 hip && trace 128 256x384 hip &&
trace 256 768x1024 torch &&
for d in "$O"/tr_*/; do
    python tools/bench_raycast.py --stats "$(find "$d" -name '*kernel_stats.csv' | head -1)" || exit 1
done 2>&1 | tee "$O/kernel_stats.log" &&
timeout -k 10 300 python tools/bench_raycast.py --stream --json "$O/bench_raycast_stream.json" 2>&1 | tee "$O/bench_raycast_stream.log"
