#!/bin/bash
# Same-box A/B of the sparse head's output layers at the centre pixel (STM_HEAD_CENTER=0 / 1): the head's stages timed alone both ways, one
# plain run of bench.py that is not recorded (the first run on a box is slow), alternating plain runs at 32 / 8 / 4 clips, one run of a
# checkout of the parent commit where one is given (built; also compares the two runs' detections.npy), then one rocprofv3 kernel trace of
# each side summarised as profiles/bench_kernel_stats_sparse_head.md is.
# usage: ab_head_center.sh [out dir] [pairs at 32 clips] [pairs at 8 and 4 clips] [parent checkout]
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$R/profiles}
PAIRS=${2:-3}
PAIRS_SMALL=${3:-2}
PARENT=${4:-}
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
cd "$R" || exit 1
fail() { echo "$1 failed"; tail -5 "$OUT/ab_err.txt"; exit 1; }
bench() {   # directory, STM_HEAD_CENTER or "", label, bench.py flags ...
    local dir=$1 side=$2 label=$3; shift 3
    ( cd "$dir" && env ${side:+STM_HEAD_CENTER=$side} timeout -k 10 300 python3 bench.py --gpus 1 "$@" 2> "$OUT/ab_err.txt" | tail -1 > "$OUT/ab_line.json" ) || fail "bench.py ($label)"
    python3 -c "import json,sys; d=json.load(open(sys.argv[1])); print(sys.argv[2], d['value'], d['unit'], round(1e3 * d['config']['clips_per_gpu'] / d['value'], 3), 'ms per step')" \
        "$OUT/ab_line.json" "$label" | tee -a "$OUT/head_center_ab.txt" || exit 1
}
{
    for side in 0 1; do
        echo "== STM_HEAD_CENTER=$side"
        STM_HEAD_CENTER=$side timeout -k 10 300 python3 scripts/bench_sparse_head_stages.py 2> "$OUT/ab_err.txt" || fail "bench_sparse_head_stages.py"
    done
} > "$OUT/head_center_stages.txt"
grep -E "^==|small patches|trk patches|candidates|^assemble|^sum" "$OUT/head_center_stages.txt"
: > "$OUT/head_center_ab.txt"
STM_HEAD_CENTER=0 timeout -k 10 300 python3 bench.py --gpus 1 > /dev/null 2> "$OUT/ab_err.txt" || fail "bench.py (first run)"
for i in $(seq 1 "$PAIRS"); do
    for side in 0 1; do bench . $side "pair $i STM_HEAD_CENTER=$side"; done
done
if [ -n "$PARENT" ]; then
    D=$(mktemp -d)
    bench "$PARENT" "" "parent commit" --dump-outputs "$D/parent"
    bench . "" "this tree, switch unset" --dump-outputs "$D/new"
    python3 -c "import numpy as np, sys; a, b = (np.load(sys.argv[1] + '/' + s + '/detections.npy') for s in ('parent', 'new')); print('detections.npy of the two runs above', a.shape, 'array_equal', np.array_equal(a, b))" "$D" | tee -a "$OUT/head_center_ab.txt"
    rm -rf "$D"
fi
for c in 8 4; do
    for i in $(seq 1 "$PAIRS_SMALL"); do
        for side in 0 1; do bench . $side "clips $c pair $i STM_HEAD_CENTER=$side" --clips $c; done
    done
done
rm -f "$OUT/ab_err.txt" "$OUT/ab_line.json"
for side in 0 1; do
    T=$(mktemp -d)
    STM_HEAD_CENTER=$side timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o bench -- python3 bench.py --gpus 1 --steps 20 --warmup 6 > "$T/log.txt" 2>&1 || { echo "trace failed"; tail -5 "$T/log.txt"; exit 1; }
    t=$(ls "$T"/*/*kernel_trace.csv "$T"/*kernel_trace.csv 2>/dev/null | head -1)
    python3 scripts/summarize_trace.py "$t" > "$OUT/bench_kernel_stats_head_center_$side.md" || exit 1
    rm -rf "$T"
done
