"""The reference's training step (train.py:134-150, :290-320) over this package: NetLoss ties the train-mode STMask.forward to layers.MultiBoxLoss,
train_step runs one optimizer step; lr_at and autoscale restate its learning-rate schedule (train.py:88-96, :293-302) as pure functions.  The
batches come from stmask_amd.datasets (YTVISTrainSet, TrainLoader, collate_device) or synthetic.synthetic_train_batch; scripts/train_ytvis.py
puts the pieces together.  ExtraAugmentation, DataParallel, logging and checkpoints are not built."""
import torch.nn as nn


class NetLoss(nn.Module):
    """net(images) -> criterion(net, predictions, ground truth): the reference's wrapper (train.py:134-150)."""

    def __init__(self, net, criterion):
        super().__init__()
        self.net = net
        self.criterion = criterion

    def forward(self, images, gt_bboxes, gt_labels, gt_masks, gt_ids, img_meta=None):
        preds = self.net(images, img_meta)
        return self.criterion(self.net, preds, gt_bboxes, gt_labels, gt_masks, gt_ids)


def train_step(net_loss, optimizer, batch):
    """One step on batch = (images, gt_bboxes, gt_labels, gt_masks, gt_ids[, img_meta]): zero the gradients, forward, backward through the sum of
    the loss terms, optimizer step.  Returns the dict of loss terms (detached 0-dim device tensors: reading them is the caller's synchronisation)."""
    optimizer.zero_grad()
    losses = net_loss(*batch)
    sum(losses.values()).backward()
    optimizer.step()
    return {k: v.detach() for k, v in losses.items()}


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
