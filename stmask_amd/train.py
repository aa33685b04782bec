"""The reference's training step (train.py:134-150, :290-320) over this package: NetLoss ties the train-mode STMask.forward to layers.MultiBoxLoss,
train_step runs one optimizer step; lr_at and autoscale restate its learning-rate schedule (train.py:88-96, :293-302) as pure functions.  The
batches come from stmask_amd.datasets (YTVISTrainSet, TrainLoader, collate_device) or synthetic.synthetic_train_batch; scripts/train_ytvis.py
puts the pieces together with optim.GuardedSGD (the step guarded on the device), LossLog below, stmask_amd.checkpoint and the validation-mAP
hook of stmask_amd.validate.  train_step_dp is the step of one rank of a data-parallel run (stmask_amd.parallel, optim.DataParallelSGD;
scripts/train_ytvis.py --gpus N).  Not built: overlap of the gradient exchange with the backward pass, multi-GPU validation, more than one node."""
import math

import torch
import torch.nn as nn

from .optim import GuardedSGD
from .parallel import exchange


class NetLoss(nn.Module):
    """net(images) -> criterion(net, predictions, ground truth): the reference's wrapper (train.py:134-150)."""

    def __init__(self, net, criterion):
        super().__init__()
        self.net = net
        self.criterion = criterion

    def forward(self, images, gt_bboxes, gt_labels, gt_masks, gt_ids, img_meta=None):
        preds = self.net(images, img_meta)
        return self.criterion(self.net, preds, gt_bboxes, gt_labels, gt_masks, gt_ids)


def use_deterministic():
    """What --deterministic of the training scripts sets, in every rank: torch's flag, which autograd.is_deterministic() follows (the backward's
    scatters then sum in fixed point, bilinear upsampling differentiates through a gather), and MIOpen's deterministic solvers without a search."""
    torch.use_deterministic_algorithms(True)
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False


def train_step(net_loss, optimizer, batch):
    """One step on batch = (images, gt_bboxes, gt_labels, gt_masks, gt_ids[, img_meta]): zero the gradients, forward, backward through the sum of
    the loss terms, optimizer step.  A GuardedSGD is handed that sum: it skips the update on the device when the loss (or, with guard="grads", a
    gradient) is not finite.  Returns the dict of loss terms (detached 0-dim device tensors: reading them is the caller's synchronisation)."""
    optimizer.zero_grad()
    losses = net_loss(*batch)
    total = sum(losses.values())
    total.backward()
    if isinstance(optimizer, GuardedSGD):
        optimizer.step(total.detach())
    else:
        optimizer.step()
    return {k: v.detach() for k, v in losses.items()}


def train_step_dp(net_loss, optimizer, batch, loss_log=None, group=None):
    """One step of one rank, optimizer an optim.DataParallelSGD: forward on the rank's share of the batch, backward through the sum of the local
    loss terms (into the gradient arena), the tail write (slot 0 that sum, slots 1.. the terms in the criterion's key order), parallel.exchange
    -- the step's one collective -- and optimizer.step().  No host wait.  Returns the rank-MEAN loss terms (the reference's losses.mean(),
    train.py:310): the reduced tail times the fp32 value of 1 / world, 0-dim device tensors; loss_log.append gets the same dict."""
    losses = net_loss(*batch)
    keys = list(losses)
    total = sum(losses.values())
    total.backward()
    arena = optimizer.grads
    arena.write_tail([total] + [losses[k] for k in keys])
    exchange(arena, group)
    mean = arena.tail[1:1 + len(keys)] * optimizer.inv_world
    optimizer.step()
    out = {k: mean[i] for i, k in enumerate(keys)}
    if loss_log is not None:
        loss_log.append(out)
    return out


class LossLog:
    """The loss terms of the last iterations in a ring [capacity, len(keys) + 1] on the device of the first append (last column: their sum).
    append() is one stack and one row copy, no host wait; read() fetches the rows appended since the last read() in one transfer and returns
    {key: (last value, mean over the last `window` finite values)}, plus "Total" -- the reference's MovingAverage(100) (utils/functions.py), which
    ignores values that are not finite.  A mean over no finite value yet is NaN.  `rows` holds what the last read() fetched: one list per append, in
    the order of `names` (the keys, then "Total")."""

    def __init__(self, keys, capacity=1024, window=100):
        if capacity < 1 or window < 1 or not keys:
            raise ValueError(f"LossLog: keys={keys!r} capacity={capacity} window={window}")
        self.keys, self.capacity, self.window = list(keys), int(capacity), int(window)
        self.names = self.keys + ["Total"]
        self.ring = None
        self.appended = self.fetched = 0
        self.last = [math.nan] * len(self.names)
        self.rows = []
        self.recent = [[] for _ in self.names]       # the last `window` finite values of each column

    def append(self, losses):
        terms = [losses[k].detach().reshape(()) for k in self.keys]
        row = torch.stack(terms + [sum(terms)])               # the sum in train_step's order: the value the guard saw
        if self.ring is None:
            self.ring = torch.zeros(self.capacity, len(self.names), dtype=row.dtype, device=row.device)
        self.ring[self.appended % self.capacity] = row
        self.appended += 1

    def read(self):
        n = self.appended - self.fetched
        if n > self.capacity:
            raise RuntimeError(f"LossLog.read: {n} rows appended since the last read, the ring holds {self.capacity}: the oldest are overwritten")
        self.rows = []
        if n:
            at = torch.arange(self.fetched, self.appended) % self.capacity
            rows = self.ring[at.to(self.ring.device)].cpu().tolist()
            self.fetched = self.appended
            for row in rows:
                for c, v in enumerate(row):
                    if math.isfinite(v):
                        self.recent[c].append(v)
                        del self.recent[c][:-self.window]
            self.last, self.rows = rows[-1], rows
        return {name: (self.last[c], sum(self.recent[c]) / len(self.recent[c]) if self.recent[c] else math.nan)
                for c, name in enumerate(self.names)}


def lr_at(iteration, lr, gamma, lr_steps, lr_warmup_until, lr_warmup_init):
    """The learning rate the reference's loop (train.py:293-302) has set when a run started at iteration 0 reaches `iteration`: inside the warm-up
    (iteration <= lr_warmup_until) the linear ramp (lr - lr_warmup_init) * (iteration / lr_warmup_until) + lr_warmup_init, which is also what
    the optimizer keeps after it (the value at iteration == lr_warmup_until, in the reference's arithmetic); from lr_steps[k - 1] on
    lr * gamma ** k, also when resuming past several steps at once.  A step wins over the warm-up, as in the loop."""
    k = 0
    while k < len(lr_steps) and iteration >= lr_steps[k]:
        k += 1
    if k:
        return lr * (gamma ** k)
    if lr_warmup_until > 0:
        return (lr - lr_warmup_init) * (min(iteration, lr_warmup_until) / lr_warmup_until) + lr_warmup_init
    return lr


def autoscale(lr, max_iter, lr_steps, batch_size):
    """train.py:88-96 (--autoscale): the settings are written for 8 frames per step, a batch of `batch_size` clips holds 2 * batch_size.
    -> (lr, max_iter, lr_steps), in the reference's arithmetic (true division for the factor, floor division by it: floats when it scales)."""
    if batch_size * 2 != 8:
        factor = batch_size * 2 / 8
        lr *= factor
        max_iter //= factor
        lr_steps = [x // factor for x in lr_steps]
    return lr, max_iter, lr_steps
