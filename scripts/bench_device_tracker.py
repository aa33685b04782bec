#!/usr/bin/env python3
"""Host tracker against device tracker (BatchedClipPipeline(device_tracker=True)), same box, one job.  A measuring tool, not a test.

Default: the benchmark's workload driven as benchlib.runner.Runner drives it (planar fp16x2 graph, trunks replayed from HIP graphs, default
look-ahead, seeded synthetic 16-frame clips at 384x640) at --sizes clips.  Host mode and device mode alternate, --runs runs each, every run a
process of its own under its own time limit.  Per mode and size: every run's frames/s, the median, min..max, and the host -> device and
device -> host bytes per step (counted in a second pass over the same steps with the copying calls wrapped).  Runner.step reads pipe.prev_n
after every step, which in device mode settles at once: these rows time the resolution followed by an immediate wait for the row counts, not
the "one step late" read -- only the --serve rows exercise that.

--serve: scripts/serve_videos.py --batched-output with and without --device-tracker, alternating in the same way, at --sizes slots; prints its
JSON lines and its columns per mode.

Device mode counts as "not slower" in a row where its median lies at or above the lowest host-mode run of that row.  Raw lines of every child
are printed as they come, so the output is its own record (profiles/device_tracker_ab.txt).

usage: python scripts/bench_device_tracker.py [--sizes 1 8 32] [--runs 3] [--steps 48] [--warmup 4] [--timeout 420] [--serve]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class TransferCounter:
    """Counts, while active, the bytes that cross between host and device through the calls the pipeline copies with."""

    def __init__(self):
        self.h2d, self.d2h = 0, 0

    def __enter__(self):
        import torch
        T = torch.Tensor
        self.saved = [(n, getattr(T, n)) for n in ("cpu", "tolist", "item", "to", "copy_")]
        nbytes = lambda t: t.numel() * t.element_size()   # noqa: E731

        def down(fn):
            def counted(t, *a, **k):
                if t.is_cuda:
                    self.d2h += nbytes(t)
                return fn(t, *a, **k)
            return counted

        def to(fn):
            def counted(t, *a, **k):
                out = fn(t, *a, **k)
                if out.is_cuda and not t.is_cuda:
                    self.h2d += nbytes(t)
                elif t.is_cuda and not out.is_cuda:
                    self.d2h += nbytes(t)
                return out
            return counted

        def copy(fn):
            def counted(dst, src, *a, **k):
                if torch.is_tensor(src) and dst.is_cuda != src.is_cuda:
                    if dst.is_cuda:
                        self.h2d += nbytes(dst)
                    else:
                        self.d2h += nbytes(dst)
                return fn(dst, src, *a, **k)
            return counted

        wrap = {"cpu": down, "tolist": down, "item": down, "to": to, "copy_": copy}
        for n, fn in self.saved:
            setattr(T, n, wrap[n](fn))
        return self

    def __exit__(self, *exc):
        import torch
        for n, fn in self.saved:
            setattr(torch.Tensor, n, fn)
        return False


def child(a):
    """One run: `steps` timed steps of one mode at one size -> one JSON line."""
    import torch
    from benchlib.runner import Runner
    from stmask_amd.pipeline import BatchedClipPipeline
    args = argparse.Namespace(config=a.config, planes="fp16x2", fuse=True, channels_last=True, planar=True, frames=16, height=384, width=640,
                              pipeline="batched", max_instances=0, overlap="early", graph="auto")
    dev = torch.device("cuda", 0)
    run = Runner(args, dev, 0, 1, a.clips)
    if a.mode == "device":
        pipe = BatchedClipPipeline(run.net, a.clips, device_tracker=True)
        pipe.max_instances, pipe.prefetch_early, pipe.use_graph = run.pipe.max_instances, run.pipe.prefetch_early, run.pipe.use_graph
        run.pipe = pipe
    seconds = run.timed(a.warmup, a.steps)[0]
    rows = run.tracked_sum / max(run.tracked_steps, 1)
    with TransferCounter() as tc:
        for t in range(a.steps):                    # whole clips again (steps is a multiple of the clip length by default)
            run.step(t)
        run.gatherer.wait()
        torch.cuda.synchronize()
    print(json.dumps({"tool": "bench_device_tracker", "mode": a.mode, "clips": a.clips, "steps": a.steps,
                      "frames_per_s": round(a.clips * a.steps / seconds, 1), "seconds": round(seconds, 4),
                      "tracked_rows_per_clip": round(rows, 1), "h2d_bytes_per_step": round(tc.h2d / a.steps),
                      "d2h_bytes_per_step": round(tc.d2h / a.steps), "graph": bool(run.pipe.graph_active), "device_tracker": run.pipe.device_tracker}))


def run_child(cmd, timeout):
    """-> the child's last JSON line (None when it failed or ran out of time); its output is echoed."""
    t0 = time.time()
    try:
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
        out, rc = p.stdout, p.returncode
    except subprocess.TimeoutExpired as e:
        out = e.stdout or ""
        out, rc = out.decode(errors="replace") if isinstance(out, bytes) else out, "timeout"
    res = None
    for line in out.splitlines():
        if line.startswith("{"):
            res = json.loads(line)
            print("raw:", line, flush=True)
    if rc != 0 or res is None:
        print(f"child failed (exit {rc}, {time.time() - t0:.0f} s): {' '.join(cmd)}\n{out[-2000:]}", flush=True)
        return None, rc
    return res, rc


def summary(tag, size, results, cols):
    for mode in ("host", "device"):
        rs = [r for r in results[mode] if r is not None]
        if not rs:
            print(f"{tag} {size:>3}  {mode:<6}  no run finished", flush=True)
            continue
        fps = [r["frames_per_s"] for r in rs]
        extra = "  ".join(f"{c}={rs[-1][c]}" for c in cols)
        print(f"{tag} {size:>3}  {mode:<6}  runs {' '.join(f'{v:.1f}' for v in fps)}  median {statistics.median(fps):.1f}  "
              f"min..max {min(fps):.1f}..{max(fps):.1f}  {extra}", flush=True)
    h = [r["frames_per_s"] for r in results["host"] if r is not None]
    d = [r["frames_per_s"] for r in results["device"] if r is not None]
    if h and d:
        verdict = "not slower" if statistics.median(d) >= min(h) else "SLOWER"
        print(f"{tag} {size:>3}  device median {statistics.median(d):.1f} against the lowest host run {min(h):.1f}: {verdict} "
              f"(median / median {statistics.median(d) / statistics.median(h):.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 32], help="clips per step (slots with --serve)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--timeout", type=int, default=420, help="time limit of one run, seconds")
    ap.add_argument("--config", default="STMask_plus_resnet50_config")
    ap.add_argument("--serve", action="store_true", help="A/B scripts/serve_videos.py --batched-output instead")
    ap.add_argument("--videos", type=int, default=64, help="--serve: videos in the queue")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--mode", choices=("host", "device"), default="host", help=argparse.SUPPRESS)
    ap.add_argument("--clips", type=int, default=1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    py = sys.executable
    for size in a.sizes:
        results = {"host": [], "device": []}
        for _ in range(a.runs):
            for mode in ("host", "device"):
                if a.serve:
                    cmd = [py, os.path.join(ROOT, "scripts", "serve_videos.py"), "--batched-output", "--slots", str(size), "--videos", str(a.videos),
                           "--config", a.config] + (["--device-tracker"] if mode == "device" else [])
                else:
                    cmd = [py, os.path.abspath(__file__), "--child", "--mode", mode, "--clips", str(size), "--steps", str(a.steps), "--warmup",
                           str(a.warmup), "--config", a.config]
                res, rc = run_child(cmd, a.timeout)
                if res is not None and a.serve:
                    res = res["runs"][0]
                results[mode].append(res)
                if rc != 0 or res is None:
                    # (a device fault usually ends a child as a Python exception, exit status 1: only a clean run is followed by another)
                    print("a child did not finish cleanly: nothing more is started", flush=True)
                    summary("serve" if a.serve else "bench", size, results, [])
                    return 1
        cols = (["host_waits_per_step", "d2h_bytes_per_step", "occupancy", "videos", "frames", "steps", "graph"] if a.serve else
                ["h2d_bytes_per_step", "d2h_bytes_per_step", "tracked_rows_per_clip", "graph"])
        summary("serve" if a.serve else "bench", size, results, cols)
    return 0


if __name__ == "__main__":
    sys.exit(main())
