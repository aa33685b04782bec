"""Training target assignment on one MI355X: layers.match_batch and the per-image layers.match (csrc/match.hip, three launches per call) next to
the torch-op restatement of the reference's match (tests/match_restate.py) run in fp32 on the same card.

Shape: B = 8 images, the P = 15 345 priors of a 384x640 frame (tests/golden/priors.npz), C = 41, G = 1 / 5 / 20 / 40 ground-truth boxes per image
(seeded boxes of 4-49 % of each frame side, conf = 2 * randn).  Three whole paths, each from the per-image inputs on the device to the five target
tensors of the batch:
  batch     one layers.match_batch call (concatenations, one offsets copy, three launches)
  per-image B layers.match calls filling rows of preallocated targets + the gather gt_boxes_t[b] = bbox[idx_t[b]], the loop of multibox_loss.py:134-142
  torch     B calls of the restatement: ~30 small launches, a Python loop of G picks with two max reductions over [G, P] each, and the host
            synchronisations the reference's own code has (the count of kept priors)
Each figure: host clock around `--reps` back-to-back calls ending in a device synchronise, after a warm-up, median of 5 groups (the torch path
synchronises inside, so device events around it would measure the same thing).  The integer targets of the kernels and of the restatement are
compared on the card's inputs and the number of differing priors is printed (the restatement's exp / log are the card's torch kernels, not the
reference's CPU ones, so a prior within rounding of a threshold may differ; the goldens of tests/test_gpu_match.py are the exact check).
Usage: python scripts/bench_match.py [--reps 20] [--torch-reps 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import match_restate as R  # noqa: E402
from stmask_amd import layers  # noqa: E402

B, C, POS, NEG = 8, 41, 0.5, 0.4
LEVELS = ("p_48x80", "p_24x40", "p_12x20", "p_6x10", "p_3x5")


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e6 / reps)
    return statistics.median(per), min(per), max(per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_match.py measures on the MI355X: no device found")
    dev = "cuda"
    z = np.load(os.path.join(ROOT, "tests", "golden", "priors.npz"))
    priors = torch.cat([torch.from_numpy(z[k]) for k in LEVELS]).to(dev)
    P = priors.shape[0]
    lines = [f"# {torch.cuda.get_device_name(0)}; B={B} P={P} C={C} pos={POS} neg={NEG}; us per batch of {B} images, median [min, max] of 5 groups",
             f"# {'G':>3s} {'batch':>24s} {'per-image':>24s} {'torch restatement':>30s} {'torch/batch':>11s} {'torch/per-image':>15s} {'differing priors':>16s}"]
    print("\n".join(lines), flush=True)
    for G in (1, 5, 20, 40):
        g = torch.Generator().manual_seed(100 + G)
        boxes, labels, ids = [], [], []
        for _ in range(B):
            c = torch.rand(G, 2, generator=g) * 0.8 + 0.1
            wh = torch.rand(G, 2, generator=g) * 0.45 + 0.04
            boxes.append(torch.cat((c - wh / 2, c + wh / 2), 1).to(dev))
            labels.append(torch.randint(1, C, (G,), generator=g).to(dev))
            ids.append((torch.randperm(500, generator=g)[:G] + 1).to(dev))
        conf = (2 * torch.randn(B, P, C, generator=g)).to(dev)
        loc_t, gt_t = torch.empty(B, P, 4, device=dev), torch.empty(B, P, 4, device=dev)
        conf_t, idx_t, ids_t = (torch.empty(B, P, dtype=torch.int64, device=dev) for _ in range(3))

        def batch():
            return layers.match_batch(POS, NEG, boxes, labels, ids, priors, conf)

        def per_image():
            for b in range(B):
                layers.match(POS, NEG, boxes[b], labels[b], ids[b], priors, None, conf[b], loc_t, conf_t, idx_t, ids_t, b)
                gt_t[b] = boxes[b][idx_t[b]]

        def restated():
            return [R.match(POS, NEG, boxes[b], labels[b], ids[b], priors, conf[b]) for b in range(B)]

        kb = batch()
        per_image()
        rs = restated()
        torch.cuda.synchronize()
        assert torch.equal(kb[1], conf_t) and torch.equal(kb[2], idx_t) and torch.equal(kb[3], ids_t) and torch.equal(kb[4], gt_t)
        diff = sum(int(((kb[1][b] != rs[b]["conf_t"]) | (kb[2][b] != rs[b]["idx_t"]) | (kb[3][b] != rs[b]["ids_t"])).sum()) for b in range(B))
        tb, tp, tt = timed(batch, args.reps), timed(per_image, args.reps), timed(restated, args.torch_reps)
        fmt = lambda t: f"{t[0]:9.1f} [{t[1]:.1f}, {t[2]:.1f}]"  # noqa: E731
        line = f"  {G:3d} {fmt(tb):>24s} {fmt(tp):>24s} {fmt(tt):>30s} {tt[0] / tb[0]:10.1f}x {tt[0] / tp[0]:14.1f}x {diff:11d} of {B * P}"
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
