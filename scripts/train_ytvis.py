#!/usr/bin/env python3
"""Train on a YouTube-VIS / OVIS annotation file and its folder of frames: stmask_amd.datasets (YTVISTrainSet, TrainLoader) -> NetLoss -> SGD with
the reference's defaults (lr 1e-3, momentum 0.9, weight decay 1e-4, gamma 0.1, lr_steps 150000 / 200000, warm-up from 1e-4 over 500 iterations,
250000 iterations: config.py:397-415, :625), train.lr_at each iteration, the loss terms printed every 10 iterations (the one host read of the loop:
the criterion runs with max_pos, the loader defers its status check).  No DataParallel, no logging beyond the print, no checkpoints.
    python scripts/train_ytvis.py ANN IMG_PREFIX [--config STMask_plus_resnet50_config] [--batch_size 4] [--iters 250000] [--backbone PATH]"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stmask_amd import datasets, layers  # noqa: E402
from stmask_amd.config import get_cfg  # noqa: E402
from stmask_amd.model import STMask  # noqa: E402
from stmask_amd.train import NetLoss, autoscale, lr_at, train_step  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ann")
    ap.add_argument("img_prefix")
    ap.add_argument("--config", default="STMask_plus_resnet50_config")
    ap.add_argument("--batch_size", type=int, default=4)
    ap.add_argument("--iters", type=int, default=250000)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--decay", type=float, default=1e-4)
    ap.add_argument("--gamma", type=float, default=0.1)
    ap.add_argument("--lr_steps", type=int, nargs="*", default=[150000, 200000])
    ap.add_argument("--lr_warmup_until", type=int, default=500)
    ap.add_argument("--lr_warmup_init", type=float, default=1e-4)
    ap.add_argument("--autoscale", action="store_true", help="scale lr, iterations and lr_steps for a batch size other than 4 (train.py:88-96)")
    ap.add_argument("--max_pos", type=int, default=4096, help="row capacity of the criterion's positive lists: no host read inside the step")
    ap.add_argument("--backbone", default=None, help="backbone weights for init_weights (a state dict file)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    dev = "cuda:0"
    lr, max_iter, lr_steps = (autoscale(args.lr, args.iters, args.lr_steps, args.batch_size) if args.autoscale
                              else (args.lr, args.iters, args.lr_steps))
    cfg = get_cfg(args.config)
    net = STMask(cfg)
    torch.manual_seed(args.seed)
    if args.backbone:
        net.init_weights(args.backbone)
    net = net.to(dev).train()
    crit = layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3, temporal_fusion=cfg.temporal_fusion_module, max_pos=args.max_pos)
    net_loss = NetLoss(net, crit)
    opt = torch.optim.SGD(net.parameters(), lr=lr, momentum=args.momentum, weight_decay=args.decay)
    loader = datasets.TrainLoader(datasets.YTVISTrainSet(args.ann, args.img_prefix), args.batch_size, seed=args.seed, device=dev)
    if len(loader) == 0:
        raise SystemExit(f"{len(loader.dataset)} frame pairs do not fill one batch of {args.batch_size}")
    print(f"{len(loader.dataset)} frame pairs, {len(loader)} iterations per epoch, {math.ceil(max_iter / len(loader))} epochs")
    iteration = 0
    while iteration < max_iter:
        for batch in loader:
            if iteration >= max_iter:
                break
            cur = lr_at(iteration, lr, args.gamma, lr_steps, args.lr_warmup_until, args.lr_warmup_init)
            for group in opt.param_groups:
                group["lr"] = cur
            losses = train_step(net_loss, opt, batch)
            if iteration % 10 == 0:
                vals = {k: v.item() for k, v in losses.items()}
                print(f"iter {iteration} lr {cur:.3e}: " + "  ".join(f"{k} {v:.4f}" for k, v in vals.items()) + f"  sum {sum(vals.values()):.4f}")
            iteration += 1


if __name__ == "__main__":
    main()
