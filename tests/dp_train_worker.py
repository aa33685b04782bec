"""One rank of the data-parallel GPU tests (tests/test_gpu_dp_train.py), started under torch.distributed.run:
    dp_train_worker.py OUT --backend gloo|nccl [--share-gpu] --parts seeded,net,overflow
Each part leaves what the test asserts on in OUT/rank{r}.pt.  Every collective has the 120 s group timeout, so a failing rank cannot hang its
peer.  Not a test module."""
import argparse
import copy
import datetime
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import optim_restate as R  # noqa: E402
from stmask_amd import layers, parallel, synthetic  # noqa: E402
from stmask_amd.config import get_cfg  # noqa: E402
from stmask_amd.model import STMask  # noqa: E402
from stmask_amd.optim import DataParallelSGD, GuardedSGD  # noqa: E402
from stmask_amd.train import LossLog, NetLoss, train_step, train_step_dp  # noqa: E402

ADA = "STMask_plus_resnet50_ada_config"
SGD = dict(lr=1e-3, momentum=0.9, weight_decay=1e-4)                   # reference config.py:402-405
MAX_POS = 256            # room for every positive of the two synthetic batches (rank 1's overflows 64)
SIZES = (1, 3, 4, 5, 0, 4095, 4096, 4097, 2 * 4096 + 5)


def gathered(t):
    """[world, ...]: t of every rank, on the host."""
    t = t.detach().cpu().contiguous()
    out = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    if dist.get_backend() == "nccl":
        dev = [torch.empty_like(t, device="cuda") for _ in out]
        dist.all_gather(dev, t.cuda())
        out = [d.cpu() for d in dev]
    else:
        dist.all_gather(out, t)
    return torch.stack(out)


def first_mismatch(named):
    """The name of the first tensor whose checksum differs between the ranks (an all-gather of the per-tensor checksums), or None."""
    sums = gathered(parallel.checksums([t for _, t in named]))
    differ = (sums != sums[0]).any(0).nonzero().flatten().tolist()
    return named[differ[0]][0] if differ else None


def part_seeded(rank, world, dev, got):
    """Rank-specific seeded gradients in the views of a small parameter set -> exchange -> step."""
    params = [torch.nn.Parameter(torch.zeros(n, device=dev).copy_(torch.from_numpy(R.seeded_values(n, 40 + i)))) for i, n in enumerate(SIZES)]
    opt = DataParallelSGD(params, guard="loss", world=world, rank=rank, **SGD)
    for i, m in enumerate(opt.momentum.views):
        m.copy_(torch.from_numpy(R.seeded_values(SIZES[i], 80 + i, scales=(1e-2, 1.0, 1e2))))
    got["seeded_p0"] = [p.detach().cpu() for p in params]
    got["seeded_m0"] = [m.cpu() for m in opt.momentum.views]
    grads = [R.seeded_values(n, 1000 * (rank + 1) + i, scales=(1.0, 1e-4, 1e2)) for i, n in enumerate(SIZES)]
    for v, g in zip(opt.grads.views, grads):
        v.copy_(torch.from_numpy(g))
    opt.grads.write_tail([torch.tensor(0.25 + rank, device=dev)])
    parallel.exchange(opt.grads)
    got["seeded_tail0"] = float(opt.grads.tail[0])
    opt.step()
    got["seeded_g"] = [torch.from_numpy(g) for g in grads]
    got["seeded_p1"] = [p.detach().cpu() for p in params]
    got["seeded_m1"] = [m.cpu() for m in opt.momentum.views]
    got["seeded_arena_after"] = opt.grads.flat[:opt.grads.tail_offset].cpu()
    got["seeded_counters"] = opt.counters()


def start_net(dev, out):
    """R50 ada as a training run starts it (tests/test_gpu_train_loop.py): the same bytes on every rank."""
    cfg = get_cfg(ADA)
    net = STMask(cfg)
    sd = synthetic.fill_state_dict(net, seed=0)
    path = os.path.join(out, f"backbone{os.environ['RANK']}.pth")
    torch.save({k: v for k, v in sd.items() if k.startswith("backbone.")}, path)
    torch.manual_seed(0)
    net.init_weights(path)
    return cfg, net.to(dev).train()


def bits_equal(a, b):
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def part_net(rank, world, dev, got, cfg, net):
    """Two train_step_dp steps of the real net, each rank on its own batch."""
    nl = NetLoss(copy.deepcopy(net), layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3, max_pos=MAX_POS))
    batch = synthetic.synthetic_train_batch(2, 128, 192, rank, device=dev)
    opt = DataParallelSGD(nl.net.parameters(), world=world, rank=rank, **SGD)
    trainer = parallel.DataParallelTrainer(nl, opt)
    local = []
    nl.register_forward_hook(lambda mod, args, out: local.append({k: float(v) for k, v in out.items()}))
    named = list(nl.net.named_parameters())
    log, after_first, logged = None, None, []
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        for step in range(2):
            losses = trainer.step(batch)
            log = log or LossLog(list(losses), capacity=8)
            log.append(losses)
            logged.append({k: float(v) for k, v in losses.items()})
            if step == 0:
                after_first = [p.detach().clone() for _, p in named]
        got["net_mismatch"] = first_mismatch(named)
        got["net_momentum_mismatch"] = first_mismatch([(n, opt.state[p]["momentum_buffer"]) for n, p in named])
        got["net_local"], got["net_logged"], got["net_counters"] = local, logged, opt.counters()
        got["net_log_rows"] = log.read() and log.rows
        got["net_keys"] = list(losses)
        got["net_arena_zero"] = not bool(opt.grads.flat[:opt.grads.tail_offset].view(torch.int32).any())
        got["net_moved"] = sum(not bits_equal(p, q) for (_, p), (_, q) in zip(named, net.named_parameters()))
        # one solo step on this rank's batch alone: what the parameters would be had nothing been exchanged
        solo = NetLoss(copy.deepcopy(net), layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3, max_pos=MAX_POS))
        train_step(solo, GuardedSGD(solo.net.parameters(), **SGD), batch)
        got["net_differs_from_solo"] = sum(not bits_equal(p, q) for p, q in zip(after_first, solo.net.parameters()))
        got["net_tensors"] = len(named)


def part_overflow(rank, world, dev, got, cfg, net):
    """Rank 1 alone gets the batch whose positive lists overflow (max_pos=1): NaN losses and gradients on that rank."""
    nl = NetLoss(copy.deepcopy(net), layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3, max_pos=1 if rank == 1 else 64))
    batch = synthetic.synthetic_train_batch(2, 128, 192, 0, device=dev)
    opt = DataParallelSGD(nl.net.parameters(), world=world, rank=rank, **SGD)
    local = []
    nl.register_forward_hook(lambda mod, args, out: local.append(float(sum(out.values()))))
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        losses = train_step_dp(nl, opt, batch)
    got["overflow_local_total"] = local[0]
    got["overflow_logged_total"] = float(sum(losses.values()))
    got["overflow_changed"] = [n for (n, p), q in zip(nl.net.named_parameters(), net.parameters()) if not bits_equal(p, q)]
    got["overflow_momentum_zero"] = not bool(opt.momentum.flat.view(torch.int32).any())
    got["overflow_counters"] = opt.counters()
    got["overflow_arena_zero"] = not bool(opt.grads.flat[:opt.grads.tail_offset].view(torch.int32).any())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--backend", default="gloo")
    ap.add_argument("--share-gpu", action="store_true")
    ap.add_argument("--parts", default="seeded,net,overflow")
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = "cuda:0" if args.share_gpu else f"cuda:{int(os.environ['LOCAL_RANK'])}"
    torch.cuda.set_device(dev)
    dist.init_process_group(args.backend, timeout=datetime.timedelta(seconds=120))
    got, parts = {"rank": rank, "world": world, "inv_world": float(np.float32(1.0) / np.float32(world))}, args.parts.split(",")
    clock = [time.perf_counter()]

    def lap(name):
        clock.append(time.perf_counter())
        got.setdefault("seconds", {})[name] = round(clock[-1] - clock[-2], 2)

    if "seeded" in parts:
        part_seeded(rank, world, dev, got)
        lap("seeded")
    if "net" in parts or "overflow" in parts:
        cfg, net = start_net(dev, args.out)
        lap("start_net")
        if "net" in parts:
            part_net(rank, world, dev, got, cfg, net)
            lap("net")
        if "overflow" in parts:
            part_overflow(rank, world, dev, got, cfg, net)
            lap("overflow")
    torch.save(got, os.path.join(args.out, f"rank{rank}.pt"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
