"""select_neg_bboxes and ohem_conf_loss of the reference's MultiBoxLoss (layers/modules/multibox_loss.py:402-448) over csrc/conf_loss.hip: the
log-sum-exp of every prior, the hard negatives without a sort, the weights and the weighted cross entropy in 8 launches and no host
synchronisation (the reference: a global-maximum log_sum_exp, a full descending sort of all B * P scores, a boolean gather, F.cross_entropy
and three host round trips).  Conventions: include/stmask_hip.h and INTEGRATION.md section 14.

ohem_use_most_confident=True (config.py: False in every STMask config) has no form here, and neither have focal_conf_loss and
focal_conf_sigmoid_loss.  The centerness term of ohem_conf_loss (:450-455) is layers.box_center_loss (pos_loss.py)."""
import torch

from .. import autograd, ops


def select_neg_bboxes(conf_data, conf_t, negpos_ratio=3):
    """conf_data [B,P,C] or [N,C], conf_t int64 [B,P] or [N] -> float32 [B*P] of 0 / 1: the hard negatives (no gradient, no grad_fn).  Among equal
    scores at the cut the lower flattened index is chosen (the reference's unstable sort leaves that open)."""
    if conf_data.dtype != torch.float32:
        conf_data = conf_data.float()
    return ops.ohem_select_neg(conf_data, conf_t, negpos_ratio)


def ohem_conf_loss(conf_data, conf_t, negpos_ratio=3, conf_alpha=1.0, weights="reference"):
    """losses['C'] of :448 (0-dim fp32, before multibox_loss's own division by the batch size) from conf_data [B,P,C] and conf_t int64 [B,P]; the
    positives' weights 1 / max(npos_b, 1) of :159-161 are formed on the device.  weights="reference" reproduces the reference's number: its weight
    vector cat([positives' weights, negatives' weights]) meets the kept rows in prior order, so weights go by position; weights="aligned" gives
    every positive its own image's weight and every selected negative the negatives' weight.  Gradient w.r.t. conf_data only."""
    if conf_data.dtype != torch.float32:
        conf_data = conf_data.float()
    if autograd.wants_grad(conf_data):
        return autograd.ohem_conf_loss(conf_data, conf_t, negpos_ratio, conf_alpha, weights)
    return ops.ohem_conf_loss(conf_data, conf_t, negpos_ratio, conf_alpha, weights)[0]
