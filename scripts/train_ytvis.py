#!/usr/bin/env python3
"""Train on a YouTube-VIS / OVIS annotation file and its folder of frames: stmask_amd.datasets (YTVISTrainSet, TrainLoader) -> NetLoss ->
optim.GuardedSGD with the reference's defaults (lr 1e-3, momentum 0.9, weight decay 1e-4, gamma 0.1, lr_steps 150000 / 200000, warm-up from 1e-4
over 500 iterations, 250000 iterations: config.py:397-415, :625), train.lr_at each iteration.  A run that can be left alone:
  - a batch whose loss (--guard loss) or whose gradients (--guard grads) are not finite is skipped on the device and counted, where the reference
    waits for torch.isfinite(loss).item() in every iteration (train.py:314-316); --guard off always applies;
  - the loss terms go to a train.LossLog on the device every iteration and are read every 10 iterations for the printed line (last value and the
    mean over the last 100 finite values, the reference's MovingAverage) -- the one host read of the loop: the criterion runs with max_pos, the
    loader defers its status check.  --log FILE adds one JSON line per iteration, written at those reads;
  - weights are saved under the reference's names, {config name}_{epoch}_{iteration}.pth in --save_folder, every --save_interval iterations and at
    the end, with the optimizer / loader state beside them (stmask_amd.checkpoint); --keep_latest deletes the previous save as the reference does;
    Ctrl-C writes ..._{iteration}_interrupt.pth.  The reference saves at the interval only from epoch 7 on (train.py:353); that condition is not
    reproduced: every interval saves;
  - --resume PATH|latest|interrupt continues such a run, bit for bit when the sidecar is there; with a bare .pth it is the reference's resume
    (weights only, --start_iter -1 takes the iteration from the file name).
  - --extra_aug photo,expand,crop (any subset) turns the reference's ExtraAugmentation on, with the settings its training configs carry: the
    parameters are drawn on the host, the pixels are augmented inside the batch kernels.  The numpy RNG state is not
    part of a checkpoint: a resumed run continues with fresh draws, as the flip does.
  - --valid_ann FILE [--valid_img_prefix DIR] --validation_interval N: every N iterations, and at the final save, the validation split goes
    through stmask_amd.validate.validation on an InferenceTwin of the net (the net itself stays in train mode): the results JSON and, when the
    annotation file has annotations, the mAP file are written beside the weights under the reference's names -- the checkpoint's path with
    .pth replaced by .json and .txt (train.py:369, eval.py:573) -- and --log gains a line {"kind": "valid", "iteration", "metrics"}.  The
    reference also validates at iteration 100, a debugging leftover that is not reproduced.
  - --gpus N trains on N GPUs of this node, one process per GPU (stmask_amd.parallel): the parent touches no GPU
    API and starts the ranks as child processes, as bench.py --gpus N does.  --batch_size stays the GLOBAL batch (what --autoscale sees); rank r
    reads its equal share of each batch, or the slice --batch_alloc a,b,... gives it.  Every rank builds the net under the same seed, the
    weights are broadcast from rank 0 and verified, and each step is forward, backward, ONE sum all-reduce over the flat gradient arena
    (--backend nccl: RCCL; gloo: staged through the host) and the fused finish kernel of optim.DataParallelSGD; the printed loss terms are the
    mean over the ranks.  Only rank 0 prints, logs, saves and validates; while it validates the others wait on a gloo side group.  --resume
    loads the same file on every rank.  An augmented run seeds rank r's numpy stream with seed + r.  --share-gpu puts every rank on device 0
    (gloo only: the form the tests use).  --gpus 1 is the single-process path, unchanged.
Not built: overlap of the exchange with the backward pass, multi-GPU validation, more than one node.
    python scripts/train_ytvis.py ANN IMG_PREFIX [--config STMask_plus_resnet50_config] [--batch_size 4] [--iters 250000] [--backbone PATH]
                                  [--save_folder weights/] [--resume latest] [--guard loss] [--log train.jsonl] [--extra_aug photo,expand,crop]
                                  [--gpus 8 [--backend nccl] [--batch_alloc 2,2,...]]"""
import argparse
import datetime
import json
import math
import os
import random
import sys
import time

import numpy as np

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stmask_amd import checkpoint, datasets, layers, validate  # noqa: E402
from stmask_amd.config import get_cfg  # noqa: E402
from stmask_amd.extra_aug import config_from_names  # noqa: E402
from stmask_amd.model import STMask  # noqa: E402
from stmask_amd.optim import DataParallelSGD, GuardedSGD  # noqa: E402
from stmask_amd.parallel import DataParallelTrainer  # noqa: E402
from stmask_amd.preprocess import MEANS  # noqa: E402
from stmask_amd.train import LossLog, NetLoss, autoscale, lr_at, train_step, use_deterministic  # noqa: E402

READ_EVERY = 10


def parse_args(argv=None):
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
    ap.add_argument("--save_folder", default="weights/", help="where checkpoints are written and where --resume latest|interrupt looks")
    ap.add_argument("--save_interval", type=int, default=10000, help="iterations between checkpoints (0: only at the end)")
    ap.add_argument("--keep_latest", action="store_true", help="delete the previous checkpoint after each save")
    ap.add_argument("--keep_latest_interval", type=int, default=100000,
                    help="with --keep_latest, keep the saves at these intervals (a multiple of --save_interval, or 0)")
    ap.add_argument("--resume", default=None, help="a checkpoint file, 'latest' or 'interrupt'")
    ap.add_argument("--start_iter", type=int, default=-1, help="iteration to resume at; -1 takes it from the checkpoint")
    ap.add_argument("--guard", choices=["loss", "grads", "off"], default="loss", help="what makes the optimizer skip a step, on the device")
    ap.add_argument("--extra_aug", default="", help="comma list of photo, expand, crop: ExtraAugmentation with the reference's settings for each")
    ap.add_argument("--decode", choices=["host", "device"], default="host",
                    help="where the frames' JPEG files are decoded, for training batches and validation: PIL on the host, or the MI355X (stmask_amd.jpeg)")
    ap.add_argument("--decode-split", dest="decode_split", choices=["auto", "all"], default=None,
                    help="with --decode device: decode a file without restart markers at many places at once (stmask_amd.jpeg split=): every such "
                         "file, or those of jpeg.SPLIT_MIN_BYTES or more; default: one wavefront a file")
    ap.add_argument("--log", default=None, help="a file of one JSON line per iteration (appended to when resuming)")
    ap.add_argument("--valid_ann", default=None, help="annotation file of the validation split (with or without annotations)")
    ap.add_argument("--valid_img_prefix", default=None, help="folder of the validation split's frames")
    ap.add_argument("--validation_interval", type=int, default=0, help="iterations between validations (0: off)")
    ap.add_argument("--eval_slots", type=int, default=8, help="videos in flight while validating")
    ap.add_argument("--eval_planes", choices=["fp16x2", "bf16x3", "fp16x1"], default="fp16x2", help="plane format of the twin's inference graph")
    ap.add_argument("--gpus", type=int, default=1, help="ranks of a data-parallel run on this node, one process per GPU")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl", help="the gradient exchange of --gpus N > 1")
    ap.add_argument("--batch_alloc", default=None, help="comma list, one entry per rank: the clips of each global batch a rank takes (default: equal)")
    ap.add_argument("--share-gpu", action="store_true", help="every rank on device 0 (gloo only: the test form)")
    ap.add_argument("--deterministic", action="store_true",
                    help="torch.use_deterministic_algorithms(True) and MIOpen's deterministic solvers, in every rank: a bit-reproducible backward")
    args = ap.parse_args(argv)
    if args.gpus < 1:
        ap.error(f"--gpus {args.gpus}")
    if args.batch_alloc is not None:
        try:
            args.batch_alloc = tuple(int(x) for x in args.batch_alloc.split(","))
        except ValueError:
            ap.error(f"--batch_alloc {args.batch_alloc}: a comma list of integers")
        if len(args.batch_alloc) != args.gpus or min(args.batch_alloc) < 1 or sum(args.batch_alloc) != args.batch_size:
            ap.error(f"--batch_alloc {args.batch_alloc}: one positive entry per rank of --gpus {args.gpus}, summing to --batch_size {args.batch_size}")
    elif args.batch_size % args.gpus:
        ap.error(f"--batch_size {args.batch_size} does not split evenly over --gpus {args.gpus} (give --batch_alloc)")
    if args.share_gpu and args.gpus > 1 and args.backend != "gloo":
        ap.error("--share-gpu needs --backend gloo (RCCL refuses two ranks on one device)")
    return args


def make_optimizer(args, params, lr, rank=0):
    """--gpus 1: the GuardedSGD of the single-process loop; more: one rank's DataParallelSGD."""
    kw = dict(lr=lr, momentum=args.momentum, weight_decay=args.decay, guard=None if args.guard == "off" else args.guard)
    return GuardedSGD(params, **kw) if args.gpus == 1 else DataParallelSGD(params, world=args.gpus, rank=rank, **kw)


def make_loader(args, dataset, dev, rank=0):
    shard = None if args.gpus == 1 else (rank, args.batch_alloc if args.batch_alloc is not None else args.gpus)
    return datasets.TrainLoader(dataset, args.batch_size, seed=args.seed, device=dev, shard=shard)


def main(argv=None):
    args = parse_args(argv)
    rank, world, side = 0, args.gpus, None
    if world > 1 and "RANK" not in os.environ:
        # the parent of the ranks: no GPU API here
        from benchlib.launch import start_ranks
        raise SystemExit(start_ranks(world, sys.argv[1:] if argv is None else argv, __file__).wait())
    dev = "cuda:0"
    if args.deterministic:                      # past the parent's branch: this is the single process or one of the ranks
        use_deterministic()
    if world > 1:
        import torch.distributed as dist
        rank = int(os.environ["RANK"])
        if int(os.environ["WORLD_SIZE"]) != world:
            raise SystemExit(f"--gpus {world} under a launcher with WORLD_SIZE={os.environ['WORLD_SIZE']}")
        dev = "cuda:0" if args.share_gpu else f"cuda:{int(os.environ.get('LOCAL_RANK', rank))}"
        torch.cuda.set_device(dev)
        dist.init_process_group(args.backend, timeout=datetime.timedelta(minutes=10))
        # where the other ranks wait while rank 0 validates: gloo with a generous timeout (an RCCL barrier would hit the watchdog)
        side = dist.new_group(backend="gloo", timeout=datetime.timedelta(hours=24))
        np.random.seed(args.seed + rank)        # flip and ExtraAugmentation draws: each rank its own stream
        random.seed(args.seed + rank)
    chief = rank == 0

    def say(*a):
        if chief:
            print(*a, flush=True)

    def wait_for_chief():
        if side is not None:
            dist.barrier(group=side)
    lr, max_iter, lr_steps = (autoscale(args.lr, args.iters, args.lr_steps, args.batch_size) if args.autoscale
                              else (args.lr, args.iters, args.lr_steps))
    cfg = get_cfg(args.config)
    if world > 1:
        torch.manual_seed(args.seed)            # every rank builds the same net (the broadcast from rank 0 then changes nothing)
    net = STMask(cfg)
    torch.manual_seed(args.seed)
    if args.backbone:
        net.init_weights(args.backbone)
    net = net.to(dev).train()
    crit = layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3, temporal_fusion=cfg.temporal_fusion_module, max_pos=args.max_pos)
    net_loss = NetLoss(net, crit)
    opt = make_optimizer(args, net.parameters(), lr, rank)
    trainer = DataParallelTrainer(net_loss, opt) if world > 1 else None      # weights from rank 0, verified equal
    extra_aug = config_from_names(args.extra_aug, MEANS)
    loader = make_loader(args, datasets.YTVISTrainSet(args.ann, args.img_prefix, extra_aug=extra_aug, decode=args.decode,
                                                      decode_split=args.decode_split), dev, rank)
    if len(loader) == 0:
        raise SystemExit(f"{len(loader.dataset)} frame pairs do not fill one batch of {args.batch_size}")
    say(f"{len(loader.dataset)} frame pairs, {len(loader)} iterations per epoch, {math.ceil(max_iter / len(loader))} epochs" +
        (f", {world} ranks ({args.backend})" if world > 1 else ""))
    os.makedirs(args.save_folder, exist_ok=True)

    iteration = 0
    resume = args.resume
    if resume == "interrupt":
        resume = checkpoint.get_interrupt(args.save_folder)
    elif resume == "latest":
        resume = checkpoint.get_latest(args.save_folder, cfg.name)
    if resume is not None:
        got = checkpoint.load(resume, net, opt, loader)
        iteration = got["iteration"] if args.start_iter < 0 else args.start_iter
        if not got["sidecar"]:
            # the reference's resume: the weights alone; the loader continues in the epoch the iteration falls into
            loader.load_state({"seed": args.seed, "epoch": iteration // len(loader), "batch": iteration % len(loader)})
        say(f"resumed {resume} at iteration {iteration}" + ("" if got["sidecar"] else " (weights only: momentum starts at zero)"))
    elif args.start_iter > 0:
        iteration = args.start_iter
    elif args.resume is not None:
        say(f"--resume {args.resume}: nothing to resume in {args.save_folder}, starting at iteration 0")

    log_file = open(args.log, "a" if resume is not None else "w") if args.log and chief else None
    loss_log, pending, skipped_seen = None, [], opt.counters()[1]
    last_time = time.time()

    def flush():
        """The loop's host read: the rows of the LossLog since the last one -> the printed line, the JSON lines, the skipped count."""
        nonlocal skipped_seen
        if loss_log is None or not pending:
            return
        if not chief:
            pending.clear()
            return
        stats = loss_log.read()
        if log_file:
            for (it, ep, cur, elapsed), row in zip(pending, loss_log.rows):
                log_file.write(json.dumps({"type": "train", "iter": it, "epoch": ep, "lr": round(cur, 10),
                                           "loss": {k: round(v, 5) if math.isfinite(v) else repr(v) for k, v in zip(loss_log.names, row)},
                                           "elapsed": elapsed}) + "\n")
            log_file.flush()
        it, ep, cur, elapsed = pending[-1]
        print(f"[{ep:3d}] {it:7d} || " + " | ".join(f"{k}: {avg:.3f}" for k, (_, avg) in stats.items()) + f" || lr {cur:.3e} || timer: {elapsed:.3f}",
              flush=True)
        skipped = opt.counters()[1]
        if skipped > skipped_seen:
            print(f"guard: {skipped - skipped_seen} step(s) skipped since the last line, {skipped} in all", flush=True)
            skipped_seen = skipped
        pending.clear()

    def save(path):
        if not chief:
            return
        flush()
        print(f"saving {path}", flush=True)
        checkpoint.save(path, net, opt, iteration, epoch, loader)

    twin = valid_set = None
    validating = bool(args.valid_ann and args.validation_interval > 0)
    if validating and chief:
        valid_set = datasets.YTVISValSet(args.valid_ann, args.valid_img_prefix, read_ahead=8, decode=args.decode, decode_split=args.decode_split)
        twin = validate.InferenceTwin(net, planes=args.eval_planes)

    def validate_at(path):
        """The validation split under the names of the checkpoint `path`; the mAP file only when there is something to score.  Rank 0 alone
        validates; the other ranks wait for it on the side group."""
        if not validating:
            return
        if not chief:
            wait_for_chief()
            return
        try:
            validate_chief(path)
        finally:
            wait_for_chief()

    def validate_chief(path):
        flush()
        out_json, metrics_file = validate.result_paths(path)
        scored = valid_set.has_annotations
        print(f"validating -> {out_json}", flush=True)
        metrics = validate.validation(twin, valid_set, out_json, ann_file=args.valid_ann if scored else None,
                                      metrics_file=metrics_file if scored else None, n_slots=args.eval_slots, decode=args.decode)
        if log_file:
            listed = None if metrics is None else [float(v) for v in metrics]      # calc_metrics: the 12 summary numbers
            log_file.write(json.dumps({"kind": "valid", "iteration": iteration, "metrics": listed}) + "\n")
            log_file.flush()

    epoch = loader.state()["epoch"]
    try:
        while iteration < max_iter:
            epoch = loader.state()["epoch"]
            for batch in loader:
                if iteration >= max_iter:
                    break
                cur = lr_at(iteration, lr, args.gamma, lr_steps, args.lr_warmup_until, args.lr_warmup_init)
                for group in opt.param_groups:
                    group["lr"] = cur
                losses = train_step(net_loss, opt, batch) if trainer is None else trainer.step(batch)
                if chief:
                    if loss_log is None:
                        loss_log = LossLog(list(losses), capacity=4 * READ_EVERY)
                    loss_log.append(losses)
                now = time.time()
                pending.append((iteration, epoch, cur, now - last_time))
                last_time = now
                if iteration % READ_EVERY == 0:
                    flush()
                iteration += 1
                if chief and args.save_interval > 0 and iteration % args.save_interval == 0 and iteration < max_iter:
                    latest = checkpoint.get_latest(args.save_folder, cfg.name) if args.keep_latest else None
                    path = checkpoint.save_path(cfg.name, epoch, iteration, args.save_folder)
                    save(path)
                    if latest is not None and latest != path and (args.keep_latest_interval <= 0 or
                                                                  iteration % args.keep_latest_interval != args.save_interval):
                        print(f"deleting {latest}", flush=True)
                        checkpoint.remove(latest)
                if validating and iteration % args.validation_interval == 0 and iteration < max_iter:
                    validate_at(checkpoint.save_path(cfg.name, epoch, iteration, args.save_folder))
    except KeyboardInterrupt:
        say("interrupted: saving")
        if chief:
            checkpoint.remove_interrupt(args.save_folder)
        save(checkpoint.save_path(cfg.name, epoch, iteration, args.save_folder, interrupt=True))
        raise SystemExit(130)
    save(checkpoint.save_path(cfg.name, epoch, iteration, args.save_folder))
    validate_at(checkpoint.save_path(cfg.name, epoch, iteration, args.save_folder))
    if valid_set is not None:
        valid_set.close()
    if log_file:
        log_file.close()
    if world > 1:
        wait_for_chief()                # the last save is on disk before any rank leaves
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
