#!/usr/bin/env python3
"""Continuous batching of a video queue (stmask_amd.serve.VideoBatcher) on the GPU: seeded synthetic uint8 videos of seeded lengths in two source
sizes, served at each --slots count with graph-replayed trunks.  A measuring tool, not a test.

Prints one JSON line: per slot count the frames/s (device-synchronised wall clock around the whole queue, after one warm-up queue), the slot
occupancy (active slot-steps / all slot-steps) and the number of videos and frames.  --render: every busy slot's frame is also drawn on the
device each step (VideoBatcher.run(on_frame=...), stmask_amd.display source mode); the annotated frames are dropped.  --batched-output: the
output stage of a step is one batched device stage read one step late (VideoBatcher(batched_output=True)) instead of postprocess_ytbvis per
slot.  After the timed queue the same queue runs once more with the synchronising calls wrapped (Tensor.cpu / tolist / item / nonzero,
event and device synchronize): host_waits_per_step and d2h_bytes_per_step of the chosen mode come from that run.  --device-tracker: the
pipeline keeps the tracker's state and decisions on the device (BatchedClipPipeline(device_tracker=True)).

usage: python scripts/serve_videos.py [--videos 64] [--min-frames 8] [--max-frames 36] [--slots 8 32] [--render] [--batched-output]
                                      [--device-tracker]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from stmask_amd import synthetic  # noqa: E402
from stmask_amd.config import get_cfg  # noqa: E402
from stmask_amd.fuse import optimize_for_inference  # noqa: E402
from stmask_amd.model import STMask  # noqa: E402
from stmask_amd.pipeline import BatchedClipPipeline  # noqa: E402
from stmask_amd.serve import VideoBatcher  # noqa: E402

SIZES = [(720, 1280), (480, 854)]


def make_queue(n, lo, hi, seed, dev):
    """n videos: lengths uniform in [lo, hi], sizes alternating; every video a seeded noise base image translated per frame (on the device)."""
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(lo, hi + 1, (n,), generator=g).tolist()
    vids = []
    for i, T in enumerate(lengths):
        h, w = SIZES[i % 2]
        base = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(dev)
        vids.append((i, torch.stack([torch.roll(base, shifts=(4 * t, 6 * t), dims=(0, 1)) for t in range(T)])))
    return vids


def build_net(config, dev):
    net = STMask(get_cfg(config))
    net.eval()
    synthetic.fill_state_dict(net, seed=0, bg_bias=4.7)
    net = net.to(dev)
    optimize_for_inference(net, planar=True)
    net = net.to(memory_format=torch.channels_last)
    net.TemporalNet = net.TemporalNet.to(memory_format=torch.contiguous_format)
    return net


class WaitCounter:
    """Counts, while active, the calls that make the host wait for the device and the bytes they bring back."""

    def __init__(self):
        self.waits, self.bytes = 0, 0

    def __enter__(self):
        T = torch.Tensor
        self.saved = [(T, "cpu", T.cpu), (T, "tolist", T.tolist), (T, "item", T.item), (torch, "nonzero", torch.nonzero),
                      (torch.cuda.Event, "synchronize", torch.cuda.Event.synchronize), (torch.cuda, "synchronize", torch.cuda.synchronize)]

        def wrap(fn, tensor_arg):
            def counted(*args, **kw):
                t = args[0] if tensor_arg and args and torch.is_tensor(args[0]) else None
                if t is None or t.is_cuda:
                    self.waits += 1
                    if t is not None and fn is not torch.nonzero:
                        self.bytes += t.numel() * t.element_size()
                return fn(*args, **kw)
            return counted

        for owner, name, fn in self.saved:
            setattr(owner, name, wrap(fn, owner is T or owner is torch))
        return self

    def __exit__(self, *exc):
        for owner, name, fn in self.saved:
            setattr(owner, name, fn)
        return False


def measure(net, slots, queue, warm, render=False, batched_output=False, device_tracker=False):
    pipe = BatchedClipPipeline(net, slots, device_tracker=True) if device_tracker else None
    vb = VideoBatcher(net, slots, use_graph=True, batched_output=batched_output, pipeline=pipe)
    on_frame = (lambda vid, fid, img: None) if render else None
    vb.run(warm, on_frame=on_frame)                   # warm-up queue: graph capture, workspaces, prior cache
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vb.run(queue, on_frame=on_frame)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    frames = sum(int(v.shape[0]) for _, v in queue)
    copied0 = vb.output_stage.bytes_copied if batched_output else 0
    with WaitCounter() as wc:
        vb.run(queue, on_frame=on_frame)
    torch.cuda.synchronize()
    d2h = wc.bytes + (vb.output_stage.bytes_copied - copied0 if batched_output else 0)
    return {"slots": slots, "batched_output": batched_output, "device_tracker": device_tracker, "host_waits_per_step": round(wc.waits / vb.steps, 1),
            "d2h_bytes_per_step": round(d2h / vb.steps), "frames_per_s": round(frames / dt, 1), "occupancy": round(vb.occupancy(), 4), "videos": len(queue),
            "frames": frames, "steps": vb.steps, "graph": vb.pipe.graph_active, "seconds": round(dt, 3), "render": render}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--min-frames", type=int, default=8)
    ap.add_argument("--max-frames", type=int, default=36)
    ap.add_argument("--slots", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--config", default="STMask_plus_resnet50_config")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--render", action="store_true", help="draw every served frame on the device (display source mode)")
    ap.add_argument("--batched-output", action="store_true", help="one batched output stage per step, read one step late")
    ap.add_argument("--device-tracker", action="store_true", help="tracker state and decisions on the device (BatchedClipPipeline(device_tracker=True))")
    a = ap.parse_args()
    dev = "cuda"
    net = build_net(a.config, dev)
    queue = make_queue(a.videos, a.min_frames, a.max_frames, a.seed, dev)
    rows = []
    for s in a.slots:
        warm = make_queue(max(s, 4), a.min_frames, a.min_frames + 4, a.seed + 1, dev)
        rows.append(measure(net, s, queue, warm, a.render, a.batched_output, a.device_tracker))
    print(json.dumps({"tool": "serve_videos", "config": a.config, "runs": rows}))
