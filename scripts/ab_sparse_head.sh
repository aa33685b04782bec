#!/bin/bash
# Same-box A/B of the shared head's sparse form (STM_SPARSE_HEAD=0 / 1): alternating plain runs of bench.py, then one rocprofv3 kernel
# trace of each side summarised as profiles/r06_bench_kernel_stats.md is.   usage: ab_sparse_head.sh [out dir] [pairs]
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$R/profiles}
PAIRS=${2:-3}
mkdir -p "$OUT"
cd "$R" || exit 1
: > "$OUT/sparse_head_ab.txt"
for i in $(seq 1 "$PAIRS"); do
    for side in 0 1; do
        STM_SPARSE_HEAD=$side timeout -k 10 300 python3 bench.py --gpus 1 2> "$OUT/ab_err.txt" | tail -1 > "$OUT/ab_line.json" || { echo "bench.py failed (STM_SPARSE_HEAD=$side)"; tail -5 "$OUT/ab_err.txt"; exit 1; }
        python3 -c "import json,sys; d=json.load(open(sys.argv[1])); print('pair', sys.argv[2], 'STM_SPARSE_HEAD=' + sys.argv[3], d['value'], d['unit'], round(1e3 * d['config']['clips_per_gpu'] / d['value'], 3), 'ms per step')" \
            "$OUT/ab_line.json" "$i" "$side" | tee -a "$OUT/sparse_head_ab.txt" || exit 1
    done
done
rm -f "$OUT/ab_err.txt" "$OUT/ab_line.json"
for side in 0 1; do
    name=$([ $side = 0 ] && echo dense_head || echo sparse_head)
    T=$(mktemp -d)
    STM_SPARSE_HEAD=$side timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o bench -- python3 bench.py --gpus 1 --steps 20 --warmup 6 > "$T/log.txt" 2>&1 || { echo "trace failed"; tail -5 "$T/log.txt"; exit 1; }
    t=$(ls "$T"/*/*kernel_trace.csv "$T"/*kernel_trace.csv 2>/dev/null | head -1)
    python3 scripts/summarize_trace.py "$t" > "$OUT/bench_kernel_stats_$name.md" || exit 1
    rm -rf "$T"
done
