#!/usr/bin/env python3
"""K steps of the reference's SGD (lr 1e-3, momentum 0.9, weight decay 1e-4: config.py:402-405) on synthetic frame pairs, the loss dict printed per
step.  The net starts as a training run does: init_weights from a backbone file (here the seeded synthetic backbone), Xavier for the rest, zero
biases -- the heads of synthetic.fill_state_dict are calibrated for inference and diverge under these settings.
    python scripts/train_synthetic.py --config STMask_plus_resnet50_config --steps 5 --bs 2 --hw 128 192"""
import argparse
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stmask_amd import layers, synthetic  # noqa: E402
from stmask_amd.config import get_cfg  # noqa: E402
from stmask_amd.model import STMask  # noqa: E402
from stmask_amd.train import NetLoss, train_step, use_deterministic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="STMask_plus_resnet50_config")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--bs", type=int, default=2)
    ap.add_argument("--hw", type=int, nargs=2, default=(128, 192))
    ap.add_argument("--composed", action="store_true", help="T2S_concat_feat from torch ops instead of csrc/t2s_feat.hip")
    ap.add_argument("--same-batch", action="store_true", help="every step on the batch of seed 0")
    ap.add_argument("--deterministic", action="store_true",
                    help="torch.use_deterministic_algorithms(True) and MIOpen's deterministic solvers: a bit-reproducible backward")
    args = ap.parse_args()
    if args.deterministic:
        use_deterministic()
    dev = "cuda:0"
    cfg = get_cfg(args.config)
    net = STMask(cfg)
    sd = synthetic.fill_state_dict(net, seed=0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "backbone.pth")
        torch.save({k: v for k, v in sd.items() if k.startswith("backbone.")}, path)
        torch.manual_seed(0)
        net.init_weights(path)
    net = net.to(dev).train()
    net.fused_t2s_feat = not args.composed
    crit = layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3, temporal_fusion=cfg.temporal_fusion_module)
    net_loss = NetLoss(net, crit)
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    for step in range(args.steps):
        batch = synthetic.synthetic_train_batch(args.bs, args.hw[0], args.hw[1], seed=0 if args.same_batch else step, device=dev)
        losses = train_step(net_loss, opt, batch)
        print(f"step {step}: " + "  ".join(f"{k} {float(v):.4f}" for k, v in losses.items()) + f"  sum {float(sum(losses.values())):.4f}")


if __name__ == "__main__":
    main()
