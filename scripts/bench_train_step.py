#!/usr/bin/env python3
"""T2S_concat_feat as one kernel pair (csrc/t2s_feat.hip) against its composed form (torch ops over the correlation drop-in), and one whole train step
with either:  python scripts/bench_train_step.py [--out profiles/bench_train_step.txt]

(a) layers.t2s_concat_feat forward + backward at bs = 2, 8, 16 clips, C = Cu = 256, 24x40 (the P4 maps of 384x640 frames), with the device launches
    of one forward + backward seen by torch.profiler ("not measured" if the profiler cannot trace the device).
(b) train.train_step for R50 FCA and R50 ada at 384x640, 2 clips, reference SGD settings, with the peak memory of a step.

HIP events; every shape warmed up; fused and composed alternate within each of 5 groups and the median of the groups is reported, so both forms see
the same clocks.  The composed runs of the same job are the baseline."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stmask_amd import layers, synthetic  # noqa: E402
from stmask_amd.config import get_cfg  # noqa: E402
from stmask_amd.model import STMask  # noqa: E402
from stmask_amd.train import NetLoss, train_step  # noqa: E402

DEV = "cuda:0"


def alternating(fns, reps, groups=5, warm=3):
    """{name: median over the groups of the microseconds of one call}; within a group every fn is timed once, in turn."""
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
    return {k: statistics.median(v) for k, v in per.items()}, {k: max(v) for k, v in per.items()}


def device_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return str(n) if n else "not measured"
    except Exception as exc:  # noqa: BLE001  (a measuring aid: the timings below do not depend on it)
        return f"not measured ({type(exc).__name__})"


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 1e6


def feature_rows(emit):
    emit("(a) layers.t2s_concat_feat forward + backward, C = Cu = 256, 24x40, P = 11; microseconds, median of 5 alternating groups (slowest group)")
    emit(f"{'clips':>5} {'fused':>18} {'composed':>18} {'composed/fused':>15} {'launches fused':>15} {'launches composed':>18}")
    slower = False
    for bs in (2, 8, 16):
        g = torch.Generator().manual_seed(bs)
        fpn = torch.randn(2 * bs, 256, 24, 40, generator=g).to(DEV).requires_grad_()
        t2s = torch.randn(2 * bs, 256, 24, 40, generator=g).to(DEV).requires_grad_()
        go = torch.randn(bs, 121 + 512, 24, 40, generator=g).to(DEV)

        def step(fused):
            fpn.grad = t2s.grad = None
            layers.t2s_concat_feat(fpn, t2s, 11, fused=fused).backward(go)

        med, worst = alternating({"fused": lambda: step(True), "composed": lambda: step(False)}, reps=20)
        n_f, n_c = device_launches(lambda: step(True)), device_launches(lambda: step(False))
        emit(f"{bs:>5} {med['fused']:>9.1f} ({worst['fused']:>6.1f}) {med['composed']:>9.1f} ({worst['composed']:>6.1f}) "
             f"{med['composed'] / med['fused']:>15.2f} {n_f:>15} {n_c:>18}")
        slower |= med["fused"] > worst["composed"]
    return slower


def step_rows(emit):
    emit("")
    emit("(b) train.train_step, 384x640, 2 clips, SGD(lr 1e-3, momentum 0.9, weight decay 1e-4); milliseconds, median of 5 alternating groups "
         "(slowest group); peak memory of one step in MB")
    emit(f"{'config':>10} {'fused':>18} {'composed':>18} {'composed/fused':>15} {'peak fused':>11} {'peak composed':>14}")
    slower = False
    for name, tag in (("STMask_plus_resnet50_config", "r50_fca"), ("STMask_plus_resnet50_ada_config", "r50_ada")):
        cfg = get_cfg(name)
        net = STMask(cfg)
        synthetic.fill_state_dict(net, seed=0)
        net = net.to(DEV).train()
        nl = NetLoss(net, layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3))
        opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
        batch = synthetic.synthetic_train_batch(2, 384, 640, seed=0, device=DEV)

        def step(fused):
            net.fused_t2s_feat = fused
            train_step(nl, opt, batch)

        med, worst = alternating({"fused": lambda: step(True), "composed": lambda: step(False)}, reps=3, warm=2)
        pf, pc = peak_mb(lambda: step(True)), peak_mb(lambda: step(False))
        emit(f"{tag:>10} {med['fused'] / 1e3:>9.2f} ({worst['fused'] / 1e3:>6.2f}) {med['composed'] / 1e3:>9.2f} ({worst['composed'] / 1e3:>6.2f}) "
             f"{med['composed'] / med['fused']:>15.3f} {pf:>11.1f} {pc:>14.1f}")
        slower |= med["fused"] > worst["composed"]
        del net, nl, opt
    return slower


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_train_step.txt"))
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"bench_train_step.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    slower = feature_rows(emit)
    slower |= step_rows(emit)
    emit("")
    emit("fused slower than the slowest composed group at some row: " + ("YES -- STMask.fused_t2s_feat should default to False" if slower else "no"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
