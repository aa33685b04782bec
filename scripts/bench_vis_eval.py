"""Times stmask_amd.vis_eval (video mask AP) on a seeded synthetic set of validation-like size: by default 300 videos x
36 frames at 720 x 1280, 40 categories, about 2 ground-truth and 10 detection tracks per video.  Objects are ragged blobs (a span of rows per
column, jittered column by column: a few hundred runs per mask); detections are the ground truths shifted and shrunk, plus false positives.
Ground truth is uncompressed RLE, results are compressed strings packed by the library's host packer.

Reports: the host part (VisEval(): grouping, sorting, flattening the masks), evaluate() end to end (wall clock around a device synchronise, after a warm-up evaluate) with its
launches, bytes copied and host synchronisations (vis_eval.COUNTERS), the four kernels' own times (device events around each stm_vis_* call inside
that evaluate), accumulate() and summarize().  There is no baseline to divide by: the reference's evaluator (the youtubevos cocoapi fork) is not a
dependency and cannot be run.  --restate N: the numpy restatement of the tests (tests/vis_eval_restate.py, dense masks, Python loops) on the first
N videos, as context only -- it is the tests' yardstick, not an implementation anybody would run.

    python scripts/bench_vis_eval.py [--videos 300] [--frames 36] [--out profiles/bench_vis_eval.txt]
"""
import argparse
import io
import contextlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stmask_amd import output_utils, vis_eval  # noqa: E402


def blob_counts(h, w, x0, x1, top, bot):
    """Run lengths (column-major) of the mask that covers rows [top[i], bot[i]) of column x0 + i; 1 <= top < bot <= h - 1."""
    cols = np.arange(x0, x1, dtype=np.int64) * h
    bounds = np.stack([cols + top, cols + bot], axis=1).reshape(-1)
    return np.diff(np.concatenate([[0], bounds, [h * w]]))


def make_track(rng, h, w, frames, bh, bw, y0, x0, vy, vx, jitter):
    out = []
    for f in range(frames):
        cy = int(np.clip(y0 + vy * f, 2, h - bh - 2))
        cx = int(np.clip(x0 + vx * f, 0, w - bw))
        top = np.clip(cy + rng.randint(-jitter, jitter + 1, size=bw), 1, h - 3)
        bot = np.clip(cy + bh + rng.randint(-jitter, jitter + 1, size=bw), top + 1, h - 1)
        out.append(blob_counts(h, w, cx, cx + bw, top, bot))
    return out


def strings_of(track):
    """Compressed strings of a track's frames through the library's host packer (one call per track)."""
    width = max(len(c) for c in track)
    counts = np.zeros((len(track), width), dtype=np.int32)
    for i, c in enumerate(track):
        counts[i, :len(c)] = c
    n_runs = torch.tensor([len(c) for c in track], dtype=torch.int32)
    return [s.decode() for s in output_utils.rle_strings(torch.from_numpy(counts), n_runs)]


def synthetic_set(videos, frames, h, w, cats, seed):
    rng = np.random.RandomState(seed)
    ann = {"videos": [{"id": v + 1, "height": h, "width": w, "length": frames} for v in range(videos)],
           "categories": [{"id": c + 1, "name": f"c{c + 1}"} for c in range(cats)], "annotations": []}
    results = []
    for v in range(videos):
        vid_cats = rng.randint(1, cats + 1, size=2)
        gts = []
        for g in range(int(rng.randint(1, 4))):                    # 1-3 ground truths, 2 on average
            bh, bw = int(rng.randint(40, 500)), int(rng.randint(40, 600))
            geo = (bh, bw, int(rng.randint(2, h - bh - 2)), int(rng.randint(0, w - bw)), int(rng.randint(-4, 5)), int(rng.randint(-6, 7)))
            cat = int(vid_cats[g % 2])
            track = make_track(rng, h, w, frames, *geo, jitter=3)
            segs = [{"size": [h, w], "counts": c.tolist()} if rng.rand() > 0.05 else None for c in track]
            ann["annotations"].append({"id": len(ann["annotations"]) + 1, "video_id": v + 1, "category_id": cat, "iscrowd": 0, "segmentations": segs,
                                       "areas": [None if s is None else int(sum(s["counts"][1::2])) for s in segs]})
            gts.append((cat, geo))
        for d in range(10):
            if d < 2 * len(gts):                                   # two detections near every ground truth, the rest false positives
                cat, (bh, bw, y0, x0, vy, vx) = gts[d % len(gts)]
                shrink = int(rng.randint(0, 1 + bh // 4))
                geo = (max(bh - shrink, 8), bw, y0 + int(rng.randint(-10, 11)), max(0, min(w - bw, x0 + int(rng.randint(-15, 16)))), vy, vx)
            else:
                cat = int(rng.randint(1, cats + 1)) if rng.rand() < 0.5 else int(vid_cats[d % 2])
                bh, bw = int(rng.randint(30, 300)), int(rng.randint(30, 300))
                geo = (bh, bw, int(rng.randint(2, h - bh - 2)), int(rng.randint(0, w - bw)), 0, 0)
            strs = strings_of(make_track(rng, h, w, frames, *geo, jitter=3))
            segs = [{"size": [h, w], "counts": s} if rng.rand() > 0.05 else None for s in strs]
            results.append({"video_id": v + 1, "category_id": cat, "score": float(np.round(rng.rand(), 3)), "segmentations": segs})
    return ann, results


def timed_evaluate(ann, results):
    """One evaluate() with device events around every stm_vis_* call -> (VisEval, wall seconds, {entry point: ms}, counters)."""
    marks = []
    plain = vis_eval.call

    def call(name, *args):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        plain(name, *args)
        b.record()
        marks.append((name, a, b))

    e = vis_eval.VisEval(ann, results)
    vis_eval.reset_counters()
    vis_eval.call = call
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.evaluate()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        vis_eval.call = plain
    kernels = {}
    for name, a, b in marks:
        kernels[name] = kernels.get(name, 0.0) + a.elapsed_time(b)
    return e, wall, kernels, dict(vis_eval.COUNTERS)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--videos", type=int, default=300)
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--categories", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--restate", type=int, default=0, help="also time the tests' numpy restatement on the first N videos (context, not a baseline)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_vis_eval.txt"))
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_vis_eval.py needs the MI355X"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    ann, results = synthetic_set(args.videos, args.frames, args.height, args.width, args.categories, args.seed)
    say(f"# scripts/bench_vis_eval.py on {torch.cuda.get_device_name(0)}: {args.videos} videos x {args.frames} frames at {args.height} x {args.width}, "
        f"{args.categories} categories, {len(ann['annotations'])} ground-truth and {len(results)} detection tracks (seed {args.seed}; made in "
        f"{time.perf_counter() - t0:.1f} s)")
    t0 = time.perf_counter()
    vis_eval.VisEval(ann, results)
    say(f"host part (VisEval(): group, sort, flatten):  {1e3 * (time.perf_counter() - t0):9.1f} ms")
    timed_evaluate(ann, results)                                   # warm-up: library load, allocator, first launches
    walls, last = [], None
    for _ in range(3):
        last = timed_evaluate(ann, results)
        walls.append(last[1])
    e, _, kernels, counters = last
    c = e.counters
    say(f"evaluate() end to end, wall clock:            {1e3 * float(np.median(walls)):9.1f} ms   (median of 3 after a warm-up; "
        f"min {1e3 * min(walls):.1f}, max {1e3 * max(walls):.1f})")
    say(f"  {c['masks']} masks ({c['rle_bytes']} string bytes), {c['tracks']} tracks, {c['pairs']} (detection, ground truth) pairs, {c['groups']} groups")
    say(f"  stm_vis_* launches {counters['launches']}, host -> device {counters['h2d_bytes']} bytes, device -> host {counters['d2h_bytes']} bytes in "
        f"{counters['host_syncs']} copies (each one a host synchronisation; there is no other)")
    for name in ("stm_vis_rle_decode", "stm_vis_rle_check", "stm_vis_tube_iou", "stm_vis_match"):
        say(f"  {name:<22} device events:      {kernels.get(name, 0.0):9.3f} ms")
    say(f"  the rest of evaluate() (uploads, the final copies, torch glue):                "
        f"{1e3 * float(np.median(walls)) - sum(kernels.values()):.1f} ms")
    t0 = time.perf_counter()
    e.accumulate()
    say(f"accumulate() (numpy float64):                 {1e3 * (time.perf_counter() - t0):9.1f} ms")
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        t0 = time.perf_counter()
        stats = e.summarize()
        dt = time.perf_counter() - t0
    say(f"summarize():                                  {1e3 * dt:9.1f} ms")
    for line in buf.getvalue().splitlines():
        say("  " + line)
    again = vis_eval.VisEval(ann, results).evaluate().accumulate()
    same = all(e.ious[k].tobytes() == again.ious[k].tobytes() for k in e.ious) and e.eval["precision"].tobytes() == again.eval["precision"].tobytes()
    say(f"two evaluations give identical bytes: {same}; AP {stats[0]:.6f}")
    if args.restate > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import vis_eval_restate as R
        vids = {v["id"] for v in ann["videos"][:args.restate]}
        sub = dict(ann, videos=ann["videos"][:args.restate], annotations=[a for a in ann["annotations"] if a["video_id"] in vids])
        sub_res = [r for r in results if r["video_id"] in vids]
        t0 = time.perf_counter()
        R.evaluate(sub, sub_res)
        say(f"context only, not a baseline: the tests' dense numpy restatement, evaluate of the first {args.restate} videos ({len(sub_res)} detection "
            f"tracks): {time.perf_counter() - t0:.1f} s")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
