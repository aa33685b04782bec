#!/bin/bash
# Same-box A/B of one switch of the sparse head, off / on: STM_HEAD_CENTER (output layers at the centre pixel), STM_HEAD_SPLIT (mask and track
# branches at the positions with a kept prior of their own only) or STM_HEAD_SHAPES (patch towers over each entry's own kernel footprint).
# Parts, in this order, each optional:
#   stages  the head's stages timed alone both ways (scripts/bench_sparse_head_stages.py)                      -> <tag>_stages.txt
#   bench   one plain run of bench.py that is not recorded (the first run on a box is slow), alternating plain runs at 32 clips, then -- where a
#           built checkout of the parent commit is given -- one run of it and one of this tree with their detections.npy compared, and one
#           switch-off run with the same comparison                                                             -> <tag>_ab.txt
#   small   alternating plain runs at 8 and 4 clips                                                             -> <tag>_ab.txt (appended)
#   trace   one rocprofv3 kernel trace of each side through scripts/summarize_trace.py                          -> bench_kernel_stats_<tag>_<0|1>.md
# <tag> is the switch's name in lower case without STM_.  Every GPU step runs under its own time limit, and the script stops at the first failure.
# usage: ab_head_switch.sh STM_HEAD_CENTER|STM_HEAD_SPLIT|STM_HEAD_SHAPES [out dir] [pairs at 32 clips] [pairs at 8 and 4 clips] [parent checkout] [parts]
set -o pipefail
SW=${1:?usage: ab_head_switch.sh STM_HEAD_CENTER|STM_HEAD_SPLIT|STM_HEAD_SHAPES [out dir] [pairs] [pairs at 8 and 4 clips] [parent checkout] [parts]}
case "$SW" in STM_HEAD_CENTER|STM_HEAD_SPLIT|STM_HEAD_SHAPES) ;; *) echo "unknown switch $SW"; exit 2 ;; esac
TAG=$(echo "${SW#STM_}" | tr 'A-Z' 'a-z')
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${2:-$R/profiles}
PAIRS=${3:-5}
PAIRS_SMALL=${4:-3}
PARENT=${5:-}
PARTS=${6:-stages bench small trace}
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
cd "$R" || exit 1
fail() { echo "$1 failed"; tail -5 "$OUT/ab_err.txt"; exit 1; }
has() { case " $PARTS " in *" $1 "*) return 0 ;; *) return 1 ;; esac; }
bench() {   # directory, switch value or "", label, bench.py flags ...
    local dir=$1 side=$2 label=$3; shift 3
    ( cd "$dir" && env ${side:+$SW=$side} timeout -k 10 300 python3 bench.py --gpus 1 "$@" 2> "$OUT/ab_err.txt" | tail -1 > "$OUT/ab_line.json" ) || fail "bench.py ($label)"
    python3 -c "import json,sys; d=json.load(open(sys.argv[1])); print(sys.argv[2], d['value'], d['unit'], round(1e3 * d['config']['clips_per_gpu'] / d['value'], 3), 'ms per step')" \
        "$OUT/ab_line.json" "$label" | tee -a "$OUT/${TAG}_ab.txt" || exit 1
}
same() {    # directory of dumps, two names
    python3 -c "import numpy as np, sys; a, b = (np.load(sys.argv[1] + '/' + s + '/detections.npy') for s in sys.argv[2:4]); print('detections.npy of', sys.argv[2], 'and', sys.argv[3], a.shape, 'array_equal', np.array_equal(a, b))" "$@" \
        | tee -a "$OUT/${TAG}_ab.txt" || exit 1
}
if has stages; then
    {
        for side in 0 1; do
            echo "== $SW=$side"
            env $SW=$side timeout -k 10 300 python3 scripts/bench_sparse_head_stages.py 2> "$OUT/ab_err.txt" || fail "bench_sparse_head_stages.py"
        done
    } > "$OUT/${TAG}_stages.txt"
    grep -E "^==|patches|candidates|^assemble|^sum|shape" "$OUT/${TAG}_stages.txt"
fi
if has bench; then
    : > "$OUT/${TAG}_ab.txt"
    env $SW=0 timeout -k 10 300 python3 bench.py --gpus 1 > /dev/null 2> "$OUT/ab_err.txt" || fail "bench.py (first run)"
    for i in $(seq 1 "$PAIRS"); do
        for side in 0 1; do bench . $side "pair $i $SW=$side"; done
    done
    D=$(mktemp -d)
    bench . "" "this tree, switch unset" --dump-outputs "$D/new"
    bench . 0 "this tree, $SW=0" --dump-outputs "$D/off"
    same "$D" new off
    if [ -n "$PARENT" ]; then
        bench "$PARENT" "" "parent commit" --dump-outputs "$D/parent"
        same "$D" parent new
    fi
    rm -rf "$D"
fi
if has small; then
    for c in 8 4; do
        for i in $(seq 1 "$PAIRS_SMALL"); do
            for side in 0 1; do bench . $side "clips $c pair $i $SW=$side" --clips $c; done
        done
    done
fi
rm -f "$OUT/ab_err.txt" "$OUT/ab_line.json"
if has trace; then
    for side in 0 1; do
        T=$(mktemp -d)
        env $SW=$side timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o bench -- python3 bench.py --gpus 1 --steps 20 --warmup 6 > "$T/log.txt" 2>&1 || { echo "trace failed"; tail -5 "$T/log.txt"; exit 1; }
        t=$(ls "$T"/*/*kernel_trace.csv "$T"/*kernel_trace.csv 2>/dev/null | head -1)
        python3 scripts/summarize_trace.py "$t" > "$OUT/bench_kernel_stats_${TAG}_$side.md" || exit 1
        rm -rf "$T"
    done
fi
