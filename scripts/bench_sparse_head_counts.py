#!/usr/bin/env python3
"""Step time of the benchmark's pipeline (32 clips, graphs, the plain run's settings) against the number of priors that pass the class
threshold, dense head and sparse head side by side: where the patch launches stop paying and the dense launches of the three branches take
over (planar.PlanarGraph.sparse_capacity).  The count is pushed through eval_conf_thresh: the threshold is set between the n-th and the
(n+1)-th best foreground probability of the first step's frames, pooled over the batch.
usage: bench_sparse_head_counts.py [kept priors per frame, ...]   (default: the configured threshold, then 100 and 300 per frame)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                      # noqa: E402
from benchlib.runner import Runner, build_net   # noqa: E402
from stmask_amd import ops        # noqa: E402


def main():
    per_frame = [int(v) for v in sys.argv[1:]] or [0, 100, 300]
    args = bench.parse_args([])
    dev = torch.device("cuda:0")
    net = build_net(args, dev)
    thresh0 = net.cfg.eval_conf_thresh
    probe = Runner(args, dev, 0, 1, args.clips, net=net)
    with torch.no_grad():
        _, pred = net.forward_single(probe.frames_t[0])
    p = torch.softmax(pred["conf"], -1)[..., 1:].amax(-1)
    s = torch.sort(p.reshape(-1), descending=True).values
    del pred, probe
    rows = []
    for n in per_frame:
        k = n * args.clips
        net.cfg.eval_conf_thresh = thresh0 if n == 0 else 0.5 * (s[k - 1].item() + s[k].item())
        row = {"asked_per_frame": n, "eval_conf_thresh": net.cfg.eval_conf_thresh,
               "kept_priors_per_frame_frame0": float((p > net.cfg.eval_conf_thresh).sum().item()) / args.clips}
        for name, on in (("dense", False), ("sparse", True)):
            r = Runner(args, dev, 0, 1, args.clips, net=net)
            r.pipe.sparse_head, r.pipe.sparse_min_clips = on, 1
            sec, _, _, _ = r.timed(args.warmup, args.steps)
            row[name + "_ms_per_step"] = 1e3 * sec / args.steps
            if on:
                ctl = net._planar.sparse_ctl.tolist()        # (the slot captured last: one step's counts)
                row["positions_last_capture"] = ctl[ops.HEAD_CTL_RAW]
                row["capacity"] = net._planar.sparse_capacity(args.clips, [(48, 80), (24, 40), (12, 20), (6, 10), (3, 5)]) if (args.height, args.width) == (384, 640) else None
                row["overflow_last_capture"] = ctl[ops.HEAD_CTL_OVERFLOW]
                if net._planar.sparse_segments is not None:     # shapes form: "positions" are (pixel, shape) entries; per kernel shape, and the segments' size
                    full, _, seg_cap = net._planar.sparse_segments
                    full = full.tolist()
                    row["entries_per_shape"] = [full[ops.HEAD_CTL_SEG * (k + 1) + ops.HEAD_CTL_RAW] for k in range(len(full) // ops.HEAD_CTL_SEG - 1)]
                    row["segment_capacity"] = seg_cap
            del r
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
    net.cfg.eval_conf_thresh = thresh0


if __name__ == "__main__":
    main()
