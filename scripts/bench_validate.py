#!/usr/bin/env python3
"""What validation during training costs on one MI355X (stmask_amd.validate), R50 FCA and R50 ada.  A measuring tool, not a test.

1. Getting the live weights into the inference graph, three ways, each from the same live net on the device:
     baseline   what exists without the twin: copy.deepcopy + fuse.optimize_for_inference(planar=True)
     torch      InferenceTwin(fold="torch").refresh()
     device     InferenceTwin(fold="device").refresh()     (csrc/fold.hip)
   For each: the parameter write alone (baseline: the deepcopy and the folds, planar=False) and the whole (with the planar graph built), as the
   median and the spread of --reps device-synchronised wall-clock runs after one warm-up run; the aten operations dispatched (a count of what
   torch launches or copies; a TorchDispatchMode) and the launches of csrc/fold.hip; and the bytes the caching allocator handed out
   (torch.cuda.memory_stats "allocated_bytes.all.allocated", the delta over one run).
2. Serving the split: a seeded synthetic video queue (the one of scripts/serve_videos.py, smaller) through datasets.YTVISValSet / LazyVideo with an
   in-memory frame_reader, read_ahead 0 and 8, against VideoBatcher(batched_output=True).run on the same videos held on the device -- one warm
   batcher each on the same twin generation, alternating, --rounds rounds.  The in-memory runs are the yardstick and their spread the margin.
   Then validation() whole, once per read_ahead: refresh, a new batcher (its graphs are captured again) and the queue.

usage: python scripts/bench_validate.py [--configs ...] [--videos 16] [--slots 8] [--reps 5] [--rounds 3] [--out profiles/bench_validate.txt]"""
import argparse
import copy
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

from stmask_amd import datasets, fuse, synthetic, validate  # noqa: E402
from stmask_amd.config import get_cfg  # noqa: E402
from stmask_amd.model import STMask  # noqa: E402

SIZES = [(720, 1280), (480, 854)]
DEV = "cuda:0"


class OpCounter(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def timed(fn, reps):
    """-> (median, min, max) seconds of `reps` runs after one warm-up run, (aten ops, fold launches, allocated bytes) of one more."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    a0 = torch.cuda.memory_stats()["allocated_bytes.all.allocated"]
    with OpCounter() as oc:
        fn()
    torch.cuda.synchronize()
    alloc = torch.cuda.memory_stats()["allocated_bytes.all.allocated"] - a0
    return (statistics.median(ts), min(ts), max(ts)), (oc.n, validate.COUNTERS["fold_launches"], alloc)


def fmt(name, t, counts):
    (med, lo, hi), (ops, launches, alloc) = t, counts
    return f"  {name:34s} {med * 1e3:9.2f} ms  (min {lo * 1e3:8.2f}  max {hi * 1e3:8.2f})   aten ops {ops:6d}   fold launches {launches:2d}   allocated {alloc / 2**20:8.1f} MiB"


def live(config):
    net = STMask(get_cfg(config))
    synthetic.fill_state_dict(net, seed=0, bg_bias=4.7)
    return net.to(DEV).train()


def baseline(net, planar):
    c = copy.deepcopy(net)
    c.eval()
    fuse.optimize_for_inference(c, planar=planar)
    return c


def make_queue(n, lo, hi, seed):
    g = np.random.default_rng(seed)
    lengths = g.integers(lo, hi + 1, n).tolist()
    frames, videos = {}, []
    for i, T in enumerate(lengths):
        h, w = SIZES[i % 2]
        base = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        names = []
        for t in range(T):
            frames[f"v{i}/{t:05d}.jpg"] = np.ascontiguousarray(np.roll(base, (4 * t, 6 * t), axis=(0, 1)))
            names.append(f"v{i}/{t:05d}.jpg")
        videos.append(dict(id=i, height=h, width=w, length=T, file_names=names))
    return dict(videos=videos, categories=[dict(id=c, name=str(c)) for c in range(1, 41)]), frames


def bench_config(config, a, out):
    out(f"== {config}")
    net = live(config)
    out(" parameter write and refresh (median of %d)" % a.reps)
    validate.COUNTERS["fold_launches"] = 0
    out(fmt("baseline: deepcopy + fold", *timed(lambda: baseline(net, False), a.reps)))
    out(fmt("baseline: ... + planar graph", *timed(lambda: baseline(net, True), a.reps)))
    whole = {}
    for fold in ("torch", "device"):
        twin = validate.InferenceTwin(net, fold=fold)
        out(fmt(f"twin {fold}: write_parameters()", *timed(twin.write_parameters, a.reps)))
        t, counts = timed(twin.refresh, a.reps)
        whole[fold] = t[0]
        out(fmt(f"twin {fold}: refresh()", t, counts))
        del twin
    out(f"  refresh() device / torch: {whole['device'] / whole['torch']:.3f}")
    # serving
    ann, frames = make_queue(a.videos, a.min_frames, a.max_frames, 0)
    n_frames = sum(v["length"] for v in ann["videos"])
    held = [(v["id"], torch.stack([torch.from_numpy(frames[n]) for n in v["file_names"]]).to(DEV)) for v in ann["videos"]]
    twin = validate.InferenceTwin(net)
    twin.refresh()
    sets = {k: datasets.YTVISValSet(ann, frame_reader=frames.__getitem__, read_ahead=k) for k in (0, 8)}
    modes = {"in memory": lambda vb: twin.run(vb, held), "lazy read_ahead=0": lambda vb: twin.run(vb, sets[0].videos()),
             "lazy read_ahead=8": lambda vb: twin.run(vb, sets[8].videos())}
    batchers = {m: twin.batcher(a.slots) for m in modes}
    for m, run in modes.items():                      # warm-up: graph capture, workspaces
        run(batchers[m])
    torch.cuda.synchronize()
    fps = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m, run in modes.items():
            t0 = time.perf_counter()
            run(batchers[m])
            torch.cuda.synchronize()
            fps[m].append(n_frames / (time.perf_counter() - t0))
    out(f" serving {a.videos} videos, {n_frames} frames, {a.slots} slots, warm batchers, {a.rounds} alternating rounds (frames/s)")
    for m in modes:
        out(f"  {m:20s} median {statistics.median(fps[m]):8.1f}   min {min(fps[m]):8.1f}   max {max(fps[m]):8.1f}")
    floor = min(fps["in memory"])
    for m in list(modes)[1:]:
        out(f"  {m}: median {'below' if statistics.median(fps[m]) < floor else 'not below'} the lowest in-memory run ({floor:.1f})")
    with tempfile.TemporaryDirectory() as tmp:
        for k in (0, 8):
            t0 = time.perf_counter()
            validate.validation(twin, sets[k], os.path.join(tmp, f"r{k}.json"), n_slots=a.slots)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out(f"  validation() whole, read_ahead={k}: {dt:7.2f} s = {n_frames / dt:7.1f} frames/s (refresh, new batcher and its graph capture included)")
    for s in sets.values():
        s.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["STMask_plus_resnet50_config", "STMask_plus_resnet50_ada_config"])
    ap.add_argument("--videos", type=int, default=16)
    ap.add_argument("--min-frames", type=int, default=8)
    ap.add_argument("--max-frames", type=int, default=20)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_validate.txt"))
    a = ap.parse_args()
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)

    out(f"scripts/bench_validate.py on {torch.cuda.get_device_name(0)}: wall clock around device-synchronised runs; one warm-up run each")
    for config in a.configs:
        bench_config(config, a, out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
