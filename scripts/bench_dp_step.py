#!/usr/bin/env python3
"""The finish of a data-parallel step (optim.DataParallelSGD.step, csrc/optim.hip: average, step and clear the gradient arena in one pass)
against what the single-process loop does for the same work -- optim.GuardedSGD.step plus a memset of the gradients -- and, where the machine
has two GPUs or more, the scaling of a synthetic-batch training loop:   python scripts/bench_dp_step.py [--out profiles/bench_dp_step.txt]

(a) one card, the parameter shapes of R50 FCA and R50 ada, seeded gradients: device time (HIP events around 20 steps queued while a spin kernel
    holds the device), wall-clock per step, device launches and host synchronisations of one step, and the bytes the step has to move (finish:
    12 read + 12 written per element; GuardedSGD + memset: 12 + 8, then 4 written) over the measured device time.  The memset comes in the two
    forms a loop could use: one zero_() over a flat arena the gradients are views of, and torch's foreach zero over separate gradient tensors.
    All sides run in one process and alternate within each of 3 groups; the median of the groups is reported with the slowest group beside it.
(b) with 2 or more GPUs: train.train_step_dp on synthetic batches at 384x640, 2 clips per rank, max_pos=4096, over RCCL at 1 / 2 / 4 / 8 ranks
    (as many as the machine has): frames/s over 20 iterations after warm-up, and the exchange's share of a step (HIP events around the
    all-reduce of a filled arena, 10 times, against the step's wall-clock).  With one GPU this part is reported as not measured."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_sgd_step import CONFIGS, SGD, alternating, device_launches, host_syncs, param_shapes  # noqa: E402
from stmask_amd import layers, parallel, synthetic  # noqa: E402
from stmask_amd.config import get_cfg  # noqa: E402
from stmask_amd.model import STMask  # noqa: E402
from stmask_amd.optim import DataParallelSGD, GuardedSGD  # noqa: E402
from stmask_amd.train import NetLoss, train_step_dp  # noqa: E402

DEV = "cuda:0"
ITERS, WARM = 20, 3


def step_alone(emit):
    emit("(a) the step alone, seeded gradients; microseconds, median of 3 alternating groups (slowest group); GB/s = counted bytes / device time")
    emit(f"{'config':>8} {'side':>34} {'tensors':>8} {'Melem':>7} {'device us':>19} {'wall us':>19} {'launches':>9} {'host syncs':>11} {'MB moved':>9} {'GB/s':>7}")
    verdict = []
    for name, tag in CONFIGS:
        shapes = param_shapes(name)
        n_elem = sum(int(torch.Size(s).numel()) for s in shapes)
        gen = torch.Generator().manual_seed(0)
        loss = torch.tensor(1.0, device=DEV)

        def make():
            return [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.05).to(DEV)) for s in shapes]

        finish = DataParallelSGD(make(), guard="loss", world=2, rank=0, **SGD)
        for v in finish.grads.views:
            v.copy_(torch.randn(v.shape, generator=gen) * 1e-3)
        finish.grads.write_tail([loss])
        # the single-process step over gradients that are views of one flat buffer: its memset is one launch
        flat_params = make()
        arena = parallel.GradArena(flat_params, n_tail=0)
        arena.bind_grads()
        flat_opt = GuardedSGD(flat_params, guard="loss", **SGD)
        # ... and over separate gradient tensors, cleared the way zero_grad(set_to_none=False) clears them
        sep_params = make()
        for p in sep_params:
            p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).to(DEV)
        sep_opt = GuardedSGD(sep_params, guard="loss", **SGD)
        sep_grads = [p.grad for p in sep_params]

        def flat_side():
            flat_opt.step(loss)
            arena.flat.zero_()

        def sep_side():
            sep_opt.step(loss)
            torch._foreach_zero_(sep_grads)

        sides = {"DataParallelSGD finish": finish.step, "GuardedSGD + flat memset": flat_side, "GuardedSGD + foreach zero": sep_side}
        dev, wall = alternating(sides, reps=20, groups=3, device_fns=sides)
        for label, fn in sides.items():
            emit(f"{tag:>8} {label:>34} {len(shapes):>8} {n_elem / 1e6:>7.1f} {dev[label][0]:>9.1f} ({dev[label][1]:>7.1f}) "
                 f"{wall[label][0]:>9.1f} ({wall[label][1]:>7.1f}) {device_launches(fn):>9} {host_syncs(fn):>11} {24 * n_elem / 1e6:>9.1f} "
                 f"{24 * n_elem / dev[label][0] / 1e3:>7.0f}")
        verdict.append((tag, dev["DataParallelSGD finish"], dev["GuardedSGD + flat memset"], dev["GuardedSGD + foreach zero"]))
        del sides, finish, flat_opt, sep_opt, arena, sep_grads
        torch.cuda.empty_cache()
    return verdict


# ---- (b): one rank of the scaling run (started by scaling() through benchlib.launch.start_ranks) ------------------------------------------------
def rank_main(config):
    import datetime
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = f"cuda:{int(os.environ['LOCAL_RANK'])}"
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", timeout=datetime.timedelta(minutes=10))
    cfg = get_cfg(config)
    net = STMask(cfg)
    synthetic.fill_state_dict(net, seed=0)
    net = net.to(dev).train()
    nl = NetLoss(net, layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3, max_pos=4096))
    batch = synthetic.synthetic_train_batch(2, 384, 640, seed=rank, device=dev)
    opt = DataParallelSGD(net.parameters(), world=world, rank=rank, **dict(SGD, lr=0.0))     # lr 0: the timing must not depend on where the weights wander
    trainer = parallel.DataParallelTrainer(nl, opt)
    for _ in range(WARM):
        trainer.step(batch)
    torch.cuda.synchronize()
    dist.barrier(device_ids=[torch.cuda.current_device()])
    t0 = time.perf_counter()
    for _ in range(ITERS):
        trainer.step(batch)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / ITERS
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dist.barrier(device_ids=[torch.cuda.current_device()])
    e0.record()
    for _ in range(10):
        parallel.exchange(opt.grads)
    e1.record()
    e1.synchronize()
    worst = torch.tensor([step_ms, e0.elapsed_time(e1) / 10], device=dev)
    dist.all_reduce(worst, op=dist.ReduceOp.MAX)
    if rank == 0:
        step_ms, exchange_ms = worst.tolist()
        print(json.dumps({"dp_scaling": True, "config": config, "ranks": world, "step_ms": step_ms, "exchange_ms": exchange_ms,
                          "frames_per_s": world * 2 * 2 * 1e3 / step_ms, "arena_MB": opt.grads.flat.numel() * 4 / 1e6}), flush=True)
    dist.destroy_process_group()


def scaling(emit, n_gpus):
    from benchlib.launch import start_ranks
    emit("")
    emit("(b) train.train_step_dp over RCCL, synthetic batches, 384x640, 2 clips (4 frames) per rank, max_pos=4096; slowest rank's wall-clock per "
         f"step over {ITERS} iterations; exchange = HIP events around the all-reduce of the arena alone")
    emit(f"{'config':>8} {'ranks':>6} {'ms / step':>10} {'frames/s':>9} {'scaling':>8} {'arena MB':>9} {'exchange ms':>12} {'share of step':>14}")
    for name, tag in CONFIGS:
        base = None
        for ranks in [r for r in (1, 2, 4, 8) if r <= n_gpus]:
            proc = start_ranks(ranks, ["--rank_of", name], __file__, stdout=subprocess.PIPE, text=True)
            out = proc.communicate(timeout=1200)[0]
            rows = [json.loads(l) for l in out.splitlines() if l.startswith("{") and '"dp_scaling"' in l]
            if proc.returncode != 0 or not rows:
                emit(f"{tag:>8} {ranks:>6}   failed (exit status {proc.returncode})")
                continue
            r = rows[0]
            base = base or r["frames_per_s"] / r["ranks"]
            emit(f"{tag:>8} {ranks:>6} {r['step_ms']:>10.2f} {r['frames_per_s']:>9.1f} {r['frames_per_s'] / base:>8.2f} {r['arena_MB']:>9.1f} "
                 f"{r['exchange_ms']:>12.3f} {r['exchange_ms'] / r['step_ms']:>14.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_dp_step.txt"))
    ap.add_argument("--rank_of", default=None, help="(internal) run as one rank of the scaling part for this config")
    args = ap.parse_args()
    if args.rank_of:
        return rank_main(args.rank_of)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    n_gpus = torch.cuda.device_count()
    emit(f"bench_dp_step.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {n_gpus} GPU(s) visible")
    a = step_alone(emit)
    torch.cuda.synchronize()
    if n_gpus >= 2:
        scaling(emit, n_gpus)
    else:
        emit("")
        emit("(b) multi-GPU scaling: not measured, one GPU visible")
    emit("")
    for tag, ours, flat, sep in a:
        emit(f"{tag}: the finish takes {ours[0] / flat[0]:.3f} of the device time of GuardedSGD + one flat memset "
             f"({ours[0]:.1f} against {flat[0]:.1f} us; slowest groups {ours[1]:.1f} against {flat[1]:.1f})" +
             (" -- SLOWER" if ours[0] > flat[0] else ""))
        emit(f"{tag}: ... and {ours[0] / sep[0]:.3f} of GuardedSGD + foreach zero over separate gradients ({sep[0]:.1f} us)" +
             (" -- SLOWER" if ours[0] > sep[0] else ""))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
