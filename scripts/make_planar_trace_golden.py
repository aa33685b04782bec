"""Writes tests/golden/planar_trace.json.gz (JSON, {case: lines}, one line per C call; gzip with no time stamp, so the same lines give the same
bytes): what the Python half of the planar launch path sent across the C boundary BEFORE PlanarConv.__call__
became a sequence of steps, for every case of tests/planar_trace.py.

The package it records is whichever `stmask_amd` Python finds first: put a checkout of the parent commit (with its library built) on PYTHONPATH
-- scripts/planar_trace_golden_parent.md has the commit and the commands.  The recorder and the case list are this checkout's
tests/planar_trace.py either way; they use names the parent has too.  No GPU is used.

    PYTHONPATH=/path/to/parent python scripts/make_planar_trace_golden.py            # write the golden
    python scripts/make_planar_trace_golden.py --time /path/to/parent [groups]       # host cost of the traced dense forward, parent against this tree

--time starts one process per group, parent and this tree alternating; each builds the first case's net once, makes 3 warm-up and 20 timed passes of
its forward_single with a recorder that only counts the calls (one thread), and prints its median.  The answer: both medians over all groups and the parent's spread between its groups."""
import gzip
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.append(ROOT)          # behind PYTHONPATH: a parent checkout given there is the package that is traced


def write_golden():
    import planar_trace as pt
    import stmask_amd
    golden = {name: pt.run_case(name) for name in pt.CASES}
    path = os.path.join(ROOT, "tests", "golden", "planar_trace.json.gz")
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=raw, mtime=0) as f:
        f.write((json.dumps(golden, indent=0, sort_keys=True) + "\n").encode())
    print(f"{len(golden)} cases, {sum(len(v) for v in golden.values())} lines, {os.path.getsize(path)} bytes; package {os.path.dirname(stmask_amd.__file__)}")


def time_child(reps=20, warm=3):
    import torch
    import planar_trace as pt
    torch.set_num_threads(1)
    run = pt.forward_case(pt.R50, "fp16x2", net=pt.build_net(pt.R50, "fp16x2"))       # the first case, its net built once
    times = []
    for i in range(warm + reps):
        rec = pt.Recorder(record=False)
        t0 = time.perf_counter()
        run(rec)
        times.append(time.perf_counter() - t0)
    print(json.dumps({"median_ms": 1e3 * statistics.median(times[warm:]), "calls": rec.n_calls}))


def time_both(parent, groups):
    res = {"parent": [], "branch": []}
    for g in range(groups):
        for who, path in (("parent", parent), ("branch", None)):
            env = dict(os.environ)
            env.pop("PYTHONPATH", None)
            if path:
                env["PYTHONPATH"] = path
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--time-child"], env=env, check=True, capture_output=True, text=True).stdout
            res[who].append(json.loads(out.strip().splitlines()[-1]))
    for who, rows in res.items():
        meds = [r["median_ms"] for r in rows]
        print(f"{who}: {rows[0]['calls']} calls per pass; group medians (ms) {' '.join('%.2f' % m for m in meds)}; median {statistics.median(meds):.2f}; "
              f"spread (max - min) {max(meds) - min(meds):.2f}")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--time-child"]:
        time_child()
    elif sys.argv[1:2] == ["--time"]:
        time_both(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    else:
        write_golden()
