#!/usr/bin/env python3
"""What the deterministic backward (autograd.set_deterministic, csrc/det_backward.hip) costs on one MI355X:
    python scripts/bench_deterministic.py [--out profiles/bench_deterministic.txt]

(a) ops.deform_conv_backward (the DCN backward: both products, the recomputed columns, grad_x, grad_offset / grad_mask) at the 7 R50 layer shapes
    of scripts/bench_backward.py, batch 8, with the bytes of workspace the mode adds per layer;
(b) ops.roi_align_backward at the shift-loss shape of scripts/bench_t2s_loss.py (633 x 48 x 80 maps of 8 clips, 160 RoIs of 7 x 7 bins);
(c) the adjoint of bilinear upsampling at the FPN levels of a 384 x 640 batch of 4 (256 channels, 12x20 -> 24x40 -> 48x80): the gather kernel against
    torch's own backward;
(d) train.train_step as in scripts/bench_train_step.py part (b): R50 ada, 384 x 640, 2 clips, MIOpen's deterministic solvers on both sides.
    "on" also takes the gather adjoint in FPN and the proto net; "off" is the code as it runs without the mode.

HIP events; mode off and mode on alternate within each of `--groups` groups (at least 3) after a warm-up, so both see the same clocks; the median of
the groups is reported with the spread (fastest .. slowest group).  The mode-off runs of the same job are the baseline."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stmask_amd import autograd, layers, ops, synthetic  # noqa: E402
from stmask_amd.config import get_cfg  # noqa: E402
from stmask_amd.model import STMask  # noqa: E402
from stmask_amd.train import NetLoss, train_step  # noqa: E402

DEV = "cuda:0"
R50 = [("L1.0", 128, 96, 160, 2), ("L1.2", 128, 48, 80, 1), ("L2.0", 256, 48, 80, 2), ("L2.2", 256, 24, 40, 1), ("L2.4", 256, 24, 40, 1),
       ("L3.0", 512, 24, 40, 2), ("L3.2", 512, 12, 20, 1)]


def alternating(fns, reps, groups, warm=2):
    """{name: (median, fastest, slowest) microseconds of one call over the groups}; within a group every fn is timed once, in turn."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(groups):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            per[k].append(e0.elapsed_time(e1) * 1000.0 / reps)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in per.items()}


def with_mode(mode, fn):
    def run():
        autograd.set_deterministic(mode)
        try:
            fn()
        finally:
            autograd.set_deterministic(None)
    return run


def row(emit, label, t, unit=1.0, extra=""):
    (off, off_lo, off_hi), (on, on_lo, on_hi) = t["off"], t["on"]
    emit(f"  {label:<28} off {off / unit:9.1f} ({off_lo / unit:8.1f} .. {off_hi / unit:8.1f})   on {on / unit:9.1f} ({on_lo / unit:8.1f} .. "
         f"{on_hi / unit:8.1f})   on/off {on / off:5.2f}{extra}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_deterministic.txt"))
    args = ap.parse_args()
    if args.groups < 3:
        ap.error("--groups: at least 3")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(0)
    emit(f"bench_deterministic.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; microseconds unless said, median of {args.groups} "
         f"alternating groups x {args.reps} calls (fastest .. slowest group)")
    emit("(a) DCN backward (ops.deform_conv_backward, fused conv_offset_mask input), R50 layers at batch 8")
    tot = {"off": 0.0, "on": 0.0}
    for name, C, H, W, s in R50:
        g = ops._geom(torch.empty(8, C, H, W, device="meta"), (3, 3), s, 1, 1, 1)
        x = torch.randn(8, C, H, W, device=DEV)
        om = torch.randn(8, 27, g.Ho, g.Wo, device=DEV)
        w = torch.randn(C, C, 3, 3, device=DEV) * 0.02
        go = torch.randn(8, C, g.Ho, g.Wo, device=DEV)

        def whole():
            ops.deform_conv_backward(go, x, None, None, w, s, 1, 1, 1, fused_om=om)

        t = alternating({"off": with_mode(False, whole), "on": with_mode(True, whole)}, args.reps, args.groups)
        row(emit, f"{name} {C}x{H}x{W} s{s}", t, extra=f"   workspace {8 * (x.numel() + 1) / 1e6:7.1f} MB")
        for k in tot:
            tot[k] += t[k][0]
        del x, om, w, go
    emit(f"  all 7 layers: off {tot['off']:.0f} us, on {tot['on']:.0f} us, on/off {tot['on'] / tot['off']:.2f}")

    emit("(b) RoIAlign backward at the shift-loss shape: 160 RoIs x 7x7 into 8 x 633 x 48 x 80, sampling_ratio 0")
    gen = torch.Generator().manual_seed(1)
    n, C, H, W = 160, 633, 48, 80
    xy = torch.rand(n, 2, generator=gen) * torch.tensor([W * 0.7, H * 0.7])
    wh = torch.rand(n, 2, generator=gen) * torch.tensor([W * 0.3, H * 0.3]) + 1
    rois = torch.cat([torch.arange(n).remainder(8).float()[:, None], xy, xy + wh], 1).to(DEV)
    go = torch.randn(n, C, 7, 7, device=DEV)

    def roi():
        ops.roi_align_backward(go, rois, (8, C, H, W), 7)

    t = alternating({"off": with_mode(False, roi), "on": with_mode(True, roi)}, args.reps, args.groups)
    row(emit, "roi_align_backward", t, extra=f"   workspace {8 * (8 * C * H * W + 1) / 1e6:7.1f} MB")
    del go

    emit("(c) adjoint of bilinear upsampling, 4 x 256 channels: torch's backward (off) against the gather kernel (on)")
    for h, w_ in ((12, 20), (24, 40)):
        x = torch.randn(4, 256, h, w_, device=DEV, requires_grad=True)
        go = torch.randn(4, 256, 2 * h, 2 * w_, device=DEV)
        y = F.interpolate(x, size=(2 * h, 2 * w_), mode="bilinear", align_corners=False)

        def torchs():
            torch.autograd.grad(y, x, go, retain_graph=True)

        def gather():
            ops.upsample_bilinear_backward(go, x.shape)

        row(emit, f"{h}x{w_} -> {2 * h}x{2 * w_}", alternating({"off": torchs, "on": gather}, args.reps, args.groups))
        del x, go, y

    emit("(d) train.train_step, R50 ada, 384x640, 2 clips, SGD(lr 1e-3, momentum 0.9, weight decay 1e-4), MIOpen deterministic; milliseconds")
    cfg = get_cfg("STMask_plus_resnet50_ada_config")
    net = STMask(cfg)
    synthetic.fill_state_dict(net, seed=0)
    net = net.to(DEV).train()
    nl = NetLoss(net, layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3))
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    batch = synthetic.synthetic_train_batch(2, 384, 640, seed=0, device=DEV)

    def step():
        train_step(nl, opt, batch)

    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        t = alternating({"off": with_mode(False, step), "on": with_mode(True, step)}, max(2, args.reps // 2), args.groups)
    row(emit, "train_step r50_ada", t, unit=1e3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
