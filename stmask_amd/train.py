"""The reference's training step (train.py:134-150, :290-320) over this package: NetLoss ties the train-mode STMask.forward to layers.MultiBoxLoss,
train_step runs one optimizer step.  Dataset, augmentation, DataParallel, the learning-rate schedule and logging are not built."""
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
