#!/bin/bash
# The measurements of DESIGN.md row f9: tools/bench_eval.py per call, then one rocprofv3 kernel trace per form and size (a run of its own
# each), then the per-call kernel time and launch count of every trace.  Every GPU step has its own time limit and the chain stops at
# the first step that fails.     tools/bench_eval.sh <output directory>
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
O=${1:?usage: tools/bench_eval.sh <output directory>}
mkdir -p "$O" || exit 1
trace() {   # size, sets, form
    timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/tr_$3_$1_J$2" -- \
        python tools/bench_eval.py --trace-only --size "$1" --sets "$2" --form "$3" > "$O/tr_$3_$1_J$2.log" 2>&1
}
timeout -k 10 300 python tools/bench_eval.py --json "$O/bench_eval.json" 2>&1 | tee "$O/bench_eval.log" &&
trace 256x384 1 hip && trace 256x384 8 hip && trace 768x1024 1 hip && trace 768x1024 8 hip &&
trace 768x1024 1 torch && trace 768x1024 8 torch &&
for d in "$O"/tr_*/; do
    python tools/bench_eval.py --stats "$(find "$d" -name '*kernel_stats.csv' | head -1)" || exit 1
done 2>&1 | tee "$O/kernel_stats.log"
