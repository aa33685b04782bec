"""Times stmask_amd.datasets.collate_device with ExtraAugmentation on batches of 2, 8 and 16 clips of 720 x 1280 frames
with four instances per frame (the records of scripts/bench_train_data.py), in one job, per batch size three rounds, alternating:
  augmented   collate_device(check="deferred") of records that carry aug -- all three transforms on, drawn by ExtraAugmentation.sample from a
              seeded RandomState -- end to end (wall clock around a device synchronise);
  plain       the same records without aug: the baseline on the same card;
  host        the single-threaded numpy restatement of the reference's chain (tests/extra_aug_restate.py: the photometric chain, Expand and
              RandomCrop on whole arrays at source resolution, the uint8 cast, then the plain transforms) plus the upload of its outputs.
The reference's own cv2 / mmcv chain cannot run here -- neither is installed.  Also reported: launches, uploads and bytes copied to the device.

    python scripts/bench_extra_aug.py [--batches 2 8 16] [--rounds 3] [--out profiles/bench_extra_aug.txt]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import extra_aug_restate as RA  # noqa: E402
import train_data_restate as R  # noqa: E402
from bench_train_data import DIVISOR, H0, PER_FRAME, SIZE, W0, events_ms, make_records, med  # noqa: E402
from stmask_amd import datasets  # noqa: E402
from stmask_amd.extra_aug import ExtraAugmentation  # noqa: E402
from stmask_amd.preprocess import MEANS, STD  # noqa: E402

ALL_ON = dict(photo_metric_distortion=dict(), expand=dict(mean=MEANS, to_rgb=True, ratio_range=(1, 3)), random_crop=dict())


def augment_records(recs, seed):
    """The records with aug = [AugParams, AugParams] and the annotations ExtraAugmentation.sample leaves."""
    aug, rng, out = ExtraAugmentation(**ALL_ON), np.random.RandomState(seed), []
    for r in recs:
        r = dict(r, bboxes=list(r["bboxes"]), labels=list(r["labels"]), obj_ids=list(r["obj_ids"]), segms=list(r["segms"]), aug=[])
        for t in range(2):
            p, r["bboxes"][t], r["labels"][t], r["obj_ids"][t], r["segms"][t] = aug.sample(H0, W0, r["bboxes"][t], r["labels"][t], r["obj_ids"][t],
                                                                                         r["segms"][t], rng=rng)
            r["aug"].append(p)
        out.append(r)
    return out


def host_chain(recs, dev):
    imgs, masks, boxes = [], [], []
    for r in recs:
        for t in range(2):
            p = r["aug"][t]
            imgs.append(RA.frame_target(r["frames"][t], p, SIZE, DIVISOR, r["flip"], True, MEANS, STD))
            masks.append(np.stack([RA.mask_target(R.dense(s["counts"], H0, W0), p, SIZE, DIVISOR, r["flip"]) for s in r["segms"][t]]))
            boxes.append(R.boxes_target(r["bboxes"][t], H0, W0, SIZE, DIVISOR, r["flip"]))
    host = [torch.from_numpy(np.stack(imgs)), torch.from_numpy(np.concatenate(masks)), torch.from_numpy(np.concatenate(boxes))]
    out = [x.pin_memory().to(dev, non_blocking=True) for x in host]
    torch.cuda.synchronize()
    return out + [sum(x.numel() * x.element_size() for x in host)]


def timed_collate(recs, dev):
    torch.cuda.synchronize()
    datasets.reset_counters()
    t0 = time.perf_counter()
    *batch, status = datasets.collate_device(recs, dev, check="deferred")
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    status.raise_if_bad()
    return batch, ms, dict(datasets.COUNTERS)


def launches_alone(recs, dev):
    """Device-event times of the frame launch and of the ground-truth launches over buffers already uploaded -> (frames ms, ground truth ms)."""
    frames = datasets.upload_frames([f for r in recs for f in r["frames"]], dev)
    flips = [r["flip"] for r in recs for _ in range(2)]
    block = None
    if "aug" in recs[0]:
        frame_of = [2 * c + t for c, r in enumerate(recs) for t in range(2) for _ in r["segms"][t]]
        block = datasets.upload_aug(frames, flips, [p for r in recs for p in r["aug"]], frame_of, dev)
    gt = datasets.render_ground_truth([s for r in recs for t in range(2) for s in r["segms"][t]],
                                      [(H0, W0)] * sum(len(r["segms"][t]) for r in recs for t in range(2)),
                                      [r["flip"] for r in recs for t in range(2) for _ in r["segms"][t]],
                                      np.concatenate([b for r in recs for b in r["bboxes"]]), device=dev, aug=block)
    torch.cuda.synchronize()
    return events_ms(lambda: datasets.train_frames(frames, flips, aug=block)), events_ms(lambda: datasets.launch_ground_truth(gt.uploaded))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8, 16])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_extra_aug.py measures on the MI355X: no GPU, no numbers")
    dev = torch.device("cuda:0")
    lines = [f"# scripts/bench_extra_aug.py on {torch.cuda.get_device_name(0)}: {H0} x {W0} frames -> {SIZE} padded to 384 x 640, {PER_FRAME} instances "
             f"per frame before RandomCrop, photometric + Expand (1, 3) + RandomCrop all on, {args.rounds} rounds alternating augmented / plain / host; "
             "host = the numpy restatement of the reference's chain (cv2 and mmcv are not installed), single-threaded"]
    for bs in args.batches:
        plain = make_records(bs, seed=bs)
        recs = augment_records(plain, seed=bs)
        n_masks = sum(len(r["segms"][t]) for r in recs for t in range(2))
        taken = [sum(bool(getattr(p, k)) for r in recs for p in r["aug"]) for k in ("expand", "crop")]
        datasets.collate_device(recs, dev)                                                   # warm-up: code objects, pinned pools
        datasets.collate_device(plain, dev)
        host_chain(recs[:1], dev)
        t_aug, t_plain, t_host, k_aug, k_plain = [], [], [], [], []
        for _ in range(args.rounds):
            batch, ms, c_aug = timed_collate(recs, dev)
            t_aug.append(ms)
            _, ms, c_plain = timed_collate(plain, dev)
            t_plain.append(ms)
            t0 = time.perf_counter()
            ref = host_chain(recs, dev)
            t_host.append(1e3 * (time.perf_counter() - t0))
            k_aug.append(launches_alone(recs, dev))
            k_plain.append(launches_alone(plain, dev))
        same = (batch[0].view(-1, 3, 384, 640).cpu().numpy().tobytes() == ref[0].cpu().numpy().tobytes()
                and torch.equal(torch.cat([m for clip in batch[3] for m in clip]), ref[1])
                and torch.equal(torch.cat([b for clip in batch[1] for b in clip]).view(torch.int32), ref[2].view(torch.int32)))
        lines += [f"batch of {bs} clips ({2 * bs} frames; Expand taken on {taken[0]}, a crop on {taken[1]}; {n_masks} of {2 * bs * PER_FRAME} masks kept):",
                  f"  augmented: collate_device end to end, wall clock:        {med(t_aug)}",
                  f"    {c_aug['launches']} launches, {c_aug['uploads']} uploads, {c_aug['h2d_bytes']} bytes to the device",
                  f"    frame launch, device events:                           {med([k[0] for k in k_aug])}",
                  f"    starts + masks + boxes launches, device events:        {med([k[1] for k in k_aug])}",
                  f"  plain:     collate_device end to end, wall clock:        {med(t_plain)}",
                  f"    {c_plain['launches']} launches, {c_plain['uploads']} uploads, {c_plain['h2d_bytes']} bytes to the device",
                  f"    frame launch, device events:                           {med([k[0] for k in k_plain])}",
                  f"    starts + masks + boxes launches, device events:        {med([k[1] for k in k_plain])}",
                  f"  host: restatement of the reference's chain + upload:     {med(t_host)}",
                  f"    {ref[3]} bytes to the device",
                  f"  images, masks and boxes of the augmented batch and the host chain are the same bytes: {same}"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
