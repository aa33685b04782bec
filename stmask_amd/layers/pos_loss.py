"""The loss terms of the reference's MultiBoxLoss that act on the positive priors (layers/modules/multibox_loss.py) over csrc/pos_loss.hip:
losses['BIoU'] (:164-172) with losses['center'] (:450-455) in one pass, and losses['T'] (track_loss, :328-351).  Dense forms without boolean
indexing: no host synchronisation, the positives' weights 1 / max(npos_b, 1) of :159-161 are formed on the device, and nothing of size n x n is
ever built (the reference: three host round trips, decode and get_DIoU twice, a full n x n jaccard for its diagonal, and about eight n x n
temporaries for the track loss).  Conventions: include/stmask_hip.h and INTEGRATION.md section 14.

coeff_diversity_loss and semantic_segmentation_loss have no form here; track_to_segment_loss is layers/t2s_loss.py."""
import torch

from .. import autograd, ops


def box_center_loss(loc_data, priors, gt_boxes_t, conf_t, centerness_data=None, bboxiou_alpha=1.0, center_alpha=1.0):
    """(losses['BIoU'], losses['center']) as 0-dim fp32 before multibox_loss's own division by the batch size, from loc_data [B,P,4], priors [P,4]
    or [B,P,4], gt_boxes_t [B,P,4] (match_batch's), conf_t int64 [B,P] and centerness_data [B,P,1] or [B,P]; with centerness_data=None the second
    is None and its work is skipped.  use_yolo_regressors=False.  Gradients go to loc_data and centerness_data; as in the reference the DIoU
    inside losses['center'] is not detached, so that term sends gradient to loc_data as well."""
    if loc_data.dtype != torch.float32:
        loc_data = loc_data.float()
    if centerness_data is not None and centerness_data.dtype != torch.float32:
        centerness_data = centerness_data.float()
    if autograd.wants_grad(loc_data, centerness_data):
        return autograd.box_center_loss(loc_data, priors.detach().float(), gt_boxes_t.detach().float(), conf_t, centerness_data, bboxiou_alpha,
                                        center_alpha)
    biou, center, _ = ops.box_center_loss(loc_data, priors.float(), gt_boxes_t.float(), conf_t, centerness_data, bboxiou_alpha, center_alpha)
    return biou, center


def track_loss(track_data, conf_t, ids_t, track_alpha=1.0):
    """losses['T'] as a 0-dim fp32 from track_data [B,P,D] (used as given: the head has normalised it), conf_t and ids_t int64 [B,P]; ids are
    compared for equality and nothing else.  With fewer than two positives in the batch the loss is exactly 0 and the gradient all zeros (the
    reference divides 0 by 0 and returns NaN).  Gradient w.r.t. track_data only."""
    if track_data.dtype != torch.float32:
        track_data = track_data.float()
    if autograd.wants_grad(track_data):
        return autograd.track_loss(track_data, conf_t, ids_t, track_alpha)
    return ops.track_loss(track_data, conf_t, ids_t, track_alpha)
