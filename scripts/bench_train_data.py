"""Times stmask_amd.datasets.collate_device on batches of 2, 8 and 16 clips: 720 x 1280 uint8 frames, four instances per
frame whose run lists are the synthetic rectangles and ellipses (synthetic._shape_mask) at that size, resized to (640, 360) and padded to
384 x 640.  Per batch size, three rounds, alternating:
  device    collate_device(check="deferred") end to end (pinned staging, uploads, launches; wall clock around a device synchronise), and the launches
            alone (device events around stm_data_frames_u8_f32 and around the ground-truth launches over buffers already uploaded);
  host      the numpy / torch-CPU restatement of the reference's chain (tests/train_data_restate.py: every RLE decoded to a dense 720 x 1280 mask,
            nearest resize, flip, pad, stack; frames through the oracle's cv2-linear resize and normalisation) plus the upload of its outputs.
The reference's own cv2 / mmcv chain cannot run here -- neither is installed -- so the baseline is that restatement, single-threaded, not the
reference's DataLoader workers.  Also reported: the bytes copied to the device per batch on both sides.

    python scripts/bench_train_data.py [--batches 2 8 16] [--rounds 3] [--out profiles/bench_train_data.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_data_restate as R  # noqa: E402
from stmask_amd import datasets, synthetic  # noqa: E402
from stmask_amd.preprocess import MEANS, STD  # noqa: E402

H0, W0, SIZE, DIVISOR, PER_FRAME = 720, 1280, (640, 360), 32, 4


def counts_of_mask(mask):
    flat = np.asarray(mask, dtype=bool).reshape(-1, order="F")
    edges = np.flatnonzero(np.diff(flat.astype(np.int8))) + 1
    cnts = np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()
    return ([0] + cnts) if flat[0] else cnts


def make_records(bs, seed):
    """bs host records in YTVISTrainSet's layout (frames, run lists, boxes, labels, ids, flip), seeded."""
    rng = np.random.default_rng(seed)
    pool = [rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8) for _ in range(4)]
    h, w, Hp, Wp = datasets.padded_size(SIZE, DIVISOR)
    recs = []
    for c in range(bs):
        flip = bool(rng.random() < 0.5)
        segs, boxes = [], []
        for t in range(2):
            s, b = [], []
            for k in range(PER_FRAME):
                cy, cx = rng.uniform(0.3, 0.7) * H0, rng.uniform(0.3, 0.7) * W0
                ry, rx = rng.uniform(0.10, 0.22) * H0, rng.uniform(0.08, 0.18) * W0
                m = synthetic._shape_mask(k % 2, cy, cx, ry, rx, H0, W0).numpy()
                ys, xs = np.nonzero(m)
                s.append({"size": [H0, W0], "counts": counts_of_mask(m)})
                b.append([xs.min(), ys.min(), xs.max(), ys.max()])
            segs.append(s)
            boxes.append(np.array(b, dtype=np.float32))
        ids = [list(range(100 * c, 100 * c + PER_FRAME))] * 2
        meta = dict(ori_shape=(H0, W0, 3), img_shape=(h, w, 3), pad_shape=(Hp, Wp, 3), video_id=c, frame_id=1, is_first=False, flip=flip)
        recs.append(dict(frames=[pool[(2 * c + t) % 4] for t in range(2)], size=(H0, W0), flip=flip, video_id=c, frame_ids=[0, 1], bboxes=boxes,
                         labels=[np.arange(1, PER_FRAME + 1, dtype=np.int64)] * 2, obj_ids=ids, segms=segs, img_meta=meta,
                         img_scale=SIZE, size_divisor=DIVISOR, to_rgb=True, mean=MEANS, std=STD))
    return recs


def host_chain(recs, dev):
    """The restatement of the reference's per-sample chain and the upload of what it makes.  -> (images, masks, boxes, bytes uploaded)."""
    imgs, masks, boxes = [], [], []
    for r in recs:
        for t in range(2):
            imgs.append(R.frame_target(r["frames"][t], SIZE, DIVISOR, r["flip"], True, MEANS, STD))
            masks.append(np.stack([R.mask_target(R.dense(s["counts"], H0, W0), SIZE, DIVISOR, r["flip"]) for s in r["segms"][t]]))
            boxes.append(R.boxes_target(r["bboxes"][t], H0, W0, SIZE, DIVISOR, r["flip"]))
    host = [torch.from_numpy(np.stack(imgs)), torch.from_numpy(np.concatenate(masks)), torch.from_numpy(np.concatenate(boxes))]
    out = [x.pin_memory().to(dev, non_blocking=True) for x in host]
    torch.cuda.synchronize()
    return out + [sum(x.numel() * x.element_size() for x in host)]


def events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def med(xs):
    return f"{np.median(xs):8.2f} ms   (min {min(xs):.2f}, max {max(xs):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8, 16])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_data.py measures on the MI355X: no GPU, no numbers")
    dev = torch.device("cuda:0")
    lines = [f"# scripts/bench_train_data.py on {torch.cuda.get_device_name(0)}: {H0} x {W0} frames -> {SIZE} padded to 384 x 640, {PER_FRAME} instances per "
             f"frame, {args.rounds} rounds alternating device / host; baseline = the numpy / torch-CPU restatement of the reference's chain (cv2 and "
             "mmcv are not installed), single-threaded"]
    for bs in args.batches:
        recs = make_records(bs, seed=bs)
        n_runs = sum(len(s["counts"]) for r in recs for t in range(2) for s in r["segms"][t])
        datasets.collate_device(recs, dev)                                                   # warm-up: code objects, pinned pools
        host_chain(recs[:1], dev)
        t_dev, t_host, t_frames, t_gt = [], [], [], []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            datasets.reset_counters()
            t0 = time.perf_counter()
            *batch, status = datasets.collate_device(recs, dev, check="deferred")
            torch.cuda.synchronize()
            t_dev.append(1e3 * (time.perf_counter() - t0))
            counters = dict(datasets.COUNTERS)
            status.raise_if_bad()
            t0 = time.perf_counter()
            ref = host_chain(recs, dev)
            t_host.append(1e3 * (time.perf_counter() - t0))
            # the launches alone, over buffers already on the device
            frames = datasets.upload_frames([f for r in recs for f in r["frames"]], dev)
            flips = [r["flip"] for r in recs for _ in range(2)]
            gt = datasets.render_ground_truth([s for r in recs for t in range(2) for s in r["segms"][t]], [(H0, W0)] * (2 * bs * PER_FRAME),
                                              [r["flip"] for r in recs for _ in range(2 * PER_FRAME)],
                                              np.concatenate([b for r in recs for b in r["bboxes"]]), device=dev)
            torch.cuda.synchronize()
            t_frames.append(events_ms(lambda: datasets.train_frames(frames, flips)))
            t_gt.append(events_ms(lambda: datasets.launch_ground_truth(gt.uploaded)))
        same = (batch[0].view(-1, 3, 384, 640).cpu().numpy().tobytes() == ref[0].cpu().numpy().tobytes()
                and torch.equal(torch.cat([m for clip in batch[3] for m in clip]), ref[1])
                and torch.equal(torch.cat([b for clip in batch[1] for b in clip]).view(torch.int32), ref[2].view(torch.int32)))
        lines += [f"batch of {bs} clips ({2 * bs} frames, {2 * bs * PER_FRAME} masks, {n_runs} runs):",
                  f"  device: collate_device end to end, wall clock:           {med(t_dev)}",
                  f"    {counters['launches']} launches, {counters['uploads']} uploads, {counters['h2d_bytes']} bytes to the device "
                  f"(uint8 frames {2 * bs * H0 * W0 * 3}, run lists {4 * n_runs})",
                  f"    stm_data_frames_u8_f32, device events:                 {med(t_frames)}",
                  f"    starts + masks + boxes launches, device events:        {med(t_gt)}",
                  f"  host: restatement of the reference's chain + upload:     {med(t_host)}",
                  f"    {ref[3]} bytes to the device (float images {2 * bs * 3 * 384 * 640 * 4}, masks {2 * bs * PER_FRAME * 384 * 640})",
                  f"  images, masks and boxes of the two sides are the same bytes: {same}"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
