"""Box arithmetic of the hot path on the MI355X -- mirrors the reference's layers/box_utils.py for the functions
SURVEY.md §2 row 10 marks in scope: decode (:238-283), jaccard (:37-88), center_size (:25-35), point_form (:12-22),
sanitize_coordinates(_hw) (:298-337), crop (:341-364), mask_iou (:435-447), and the front end of the training loss: match (:119-197),
encode (:200-235).

decode / jaccard / mask_iou run as hand-written HIP kernels (bit-exact vs the oracle); the tiny element-wise helpers
stay as torch ops in the reference's operand order (IEEE add / sub / mul / div are identical on CPU and GPU).
decode and jaccard take the autograd path (autograd.DecodeFunction / JaccardFunction: the same launch, the backward of
csrc/mask_backward.hip) when an input requires grad; mask_iou is binarised and has no gradient, as in the reference.
match / match_batch assign the training targets of a batch in three launches (csrc/match.hip); they compute targets only and nothing
differentiates through them.  encode runs its kernel unless an input requires grad.
"""
import torch

from .. import autograd, ops


def point_form(boxes):
    return torch.cat((boxes[:, :2] - boxes[:, 2:] / 2, boxes[:, :2] + boxes[:, 2:] / 2), 1)


def center_size(boxes):
    return torch.cat(((boxes[:, 2:] + boxes[:, :2]) / 2, boxes[:, 2:] - boxes[:, :2]), 1)


def decode(loc, priors, use_yolo_regressors=False):
    if use_yolo_regressors:
        raise NotImplementedError("use_yolo_regressors is False in every STMask config (config.py)")
    if loc.shape[0] == 0:
        return loc.new_zeros(0, 4)
    if autograd.wants_grad(loc, priors):
        return autograd.decode(loc, priors)
    return ops.decode(loc, priors)


def encode(matched, priors, use_yolo_regressors=False):
    """box_utils.py:200-235: matched [n,4] point form, priors [n,4] centre-size -> regression targets [n,4]."""
    if use_yolo_regressors:
        raise NotImplementedError("use_yolo_regressors is False in every STMask config (config.py)")
    if matched.shape[0] == 0:
        return matched.new_zeros(0, 4)
    if autograd.wants_grad(matched, priors):
        # element-wise: the torch expression in the reference's operand order, differentiated by autograd
        g_cxcy = ((matched[:, :2] + matched[:, 2:]) / 2 - priors[:, :2]) / (0.1 * priors[:, 2:])
        q = (matched[:, 2:] - matched[:, :2]) / priors[:, 2:]
        g_wh = (torch.log(q.double()).to(q.dtype) if q.dtype == torch.float32 else torch.log(q)) / 0.2     # the log in double, as the kernel
        return torch.cat([g_cxcy, g_wh], 1)
    return ops.encode(matched, priors)


def match_batch(pos_thresh, neg_thresh, gt_bboxes, gt_labels, gt_ids, priors, conf_data, use_prediction_matching=False,
                use_change_matching=False, use_yolo_regressors=False):
    """match for a whole batch from one set of launches, with no host synchronisation: lists of per-image boxes [G_b,4], labels [G_b] and
    ids [G_b], priors [P,4] or [B,P,4], conf_data [B,P,C] -> (loc_t [B,P,4], conf_t, idx_t, ids_t [B,P] int64, gt_boxes_t [B,P,4]),
    gt_boxes_t being the gather bbox[idx_t] of multibox_loss.py:142.  1 <= G_b <= 128 and G_b <= P; boxes have x2 > x1 and y2 > y1."""
    if use_prediction_matching or use_change_matching or use_yolo_regressors:
        raise NotImplementedError("use_prediction_matching, use_change_matching and use_yolo_regressors are False in every STMask config "
                                  "(config.py); match implements that path only")
    counts = [int(b.shape[0]) for b in gt_bboxes]
    if len(gt_labels) != len(counts) or len(gt_ids) != len(counts):
        raise ValueError("match_batch: gt_bboxes, gt_labels and gt_ids must list the same images")
    one = len(counts) == 1
    boxes = gt_bboxes[0] if one else torch.cat(list(gt_bboxes))
    labels = gt_labels[0] if one else torch.cat([t.reshape(-1) for t in gt_labels])
    ids = gt_ids[0] if one else torch.cat([t.reshape(-1) for t in gt_ids])
    with torch.no_grad():
        loc_t, gt_boxes_t, conf_t, idx_t, ids_t = ops.match_priors(boxes.detach(), labels, ids, counts, priors.detach(), conf_data,
                                                                   pos_thresh, neg_thresh)
    return loc_t, conf_t, idx_t, ids_t, gt_boxes_t


def match(pos_thresh, neg_thresh, bbox, labels, ids, priors, loc_data, conf_data, loc_t, conf_t, idx_t, ids_t, idx,
          use_prediction_matching=False, use_change_matching=False, use_yolo_regressors=False):
    """box_utils.py:119-197 with the reference's signature: fills row `idx` of loc_t [B,P,4], conf_t, idx_t and ids_t [B,P] in place.
    conf_data is this image's [P,C] scores (read detached); loc_data is unused (prediction matching is off in every config)."""
    if use_prediction_matching or use_change_matching or use_yolo_regressors:
        raise NotImplementedError("use_prediction_matching, use_change_matching and use_yolo_regressors are False in every STMask config "
                                  "(config.py); match implements that path only")
    P = priors.shape[0]
    rows = (loc_t[idx], conf_t[idx], idx_t[idx], ids_t[idx])
    direct = all(r.is_contiguous() and r.is_cuda for r in rows) and rows[0].dtype == torch.float32 and \
        all(r.dtype == torch.int64 for r in rows[1:])
    with torch.no_grad():
        if direct:
            gt = torch.empty(P, 4, dtype=torch.float32, device=priors.device)
            ops.match_priors(bbox.detach(), labels, ids, [bbox.shape[0]], priors.detach(), conf_data,
                             pos_thresh, neg_thresh, out=(rows[0], gt, rows[1], rows[2], rows[3]))
        else:
            loc, gt, conf, bidx, bid = ops.match_priors(bbox.detach(), labels, ids, [bbox.shape[0]], priors.detach(), conf_data,
                                                        pos_thresh, neg_thresh)
            loc_t[idx], conf_t[idx], idx_t[idx], ids_t[idx] = loc[0], conf[0], bidx[0], bid[0]


def jaccard(box_a, box_b, iscrowd=False):
    if iscrowd:
        raise NotImplementedError("iscrowd is a training-only path")
    pair = autograd.jaccard if autograd.wants_grad(box_a, box_b) else ops.jaccard
    if box_a.dim() == 3:  # batched form used by per-class Fast NMS
        return torch.stack([pair(a, b) for a, b in zip(box_a, box_b)])
    if box_a.shape[0] == 0 or box_b.shape[0] == 0:
        return box_a.new_zeros(box_a.shape[0], box_b.shape[0])
    return pair(box_a, box_b)


def sanitize_coordinates(_x1, _x2, img_size, padding=0, cast=True):
    _x1 = _x1 * img_size
    _x2 = _x2 * img_size
    if cast:
        _x1, _x2 = _x1.long(), _x2.long()
    x1, x2 = torch.min(_x1, _x2), torch.max(_x1, _x2)
    return torch.clamp(x1 - padding, min=0), torch.clamp(x2 + padding, max=img_size)


def sanitize_coordinates_hw(box, h, w):
    squeeze = box.dim() == 2
    if squeeze:
        box = box[None]
    x1, x2 = sanitize_coordinates(box[:, :, 0], box[:, :, 2], w, cast=False)
    y1, y2 = sanitize_coordinates(box[:, :, 1], box[:, :, 3], h, cast=False)
    out = torch.stack([x1, y1, x2, y2], dim=-1)
    return out[0] if squeeze else out


def crop(masks, boxes, padding=1):
    """masks [h,w,n], boxes [n,4] relative -> (crop_mask, masks * crop_mask).  The fused kernel
    (ops.lincomb_sigmoid_crop) is what the hot path uses; this torch form exists for API parity."""
    h, w, n = masks.shape
    x1, x2 = sanitize_coordinates(boxes[:, 0], boxes[:, 2], w, padding, cast=False)
    y1, y2 = sanitize_coordinates(boxes[:, 1], boxes[:, 3], h, padding, cast=False)
    cols = torch.arange(w, device=masks.device, dtype=x1.dtype).view(1, -1, 1)
    rows = torch.arange(h, device=masks.device, dtype=x1.dtype).view(-1, 1, 1)
    crop_mask = ((cols >= x1.view(1, 1, -1)) & (cols < x2.view(1, 1, -1)) & (rows >= y1.view(1, 1, -1)) &
                 (rows < y2.view(1, 1, -1))).float()
    return crop_mask, masks * crop_mask


def mask_iou(mask1, mask2, thr=0.5):
    """[n1,h,w] x [n2,h,w] -> [n1,n2].  Inputs may be soft masks or already-binarised 0/1 floats (the reference passes
    m.gt(0.5).float(), track_TF.py:85,107): both binarise identically under `> 0.5`."""
    return ops.mask_iou(mask1, mask2, thr)
