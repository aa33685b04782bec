"""The reference's training criterion (layers/modules/multibox_loss.py) on the device: lincomb_mask_loss, the batched form of losses['M']
(:544-616, :636) over csrc/mbox_loss.hip and csrc/lincomb_backward.hip, and MultiBoxLoss, the module that turns `predictions` and the ground-truth lists into the
reference's dict of losses from the device functions of this package.  The reference forms the mask term image by image -- a boolean gather
(a host round trip), a decode, a mask, an interpolation, four [n,H,W] fp32 tensors and its own backward per image; here the positives of the
whole batch are listed once on the device, one gather builds every per-row input, and the mask (generate_mask_rows' kernel), its BCE
(mask_bce_sum) and the weighted sum each run ONCE over the rows of all images.  Conventions: include/stmask_hip_train.h and INTEGRATION.md
section 14."""
import torch

from .. import autograd, ops
from .box_utils import match_batch
from .conf_loss import ohem_conf_loss
from .mask_utils import mask_bce_sum
from .pos_loss import box_center_loss, track_loss
from .t2s_loss import track_to_segment_loss


def _zero_mask_loss(mask_data, proto_data, with_status):
    """Exactly 0; under autograd it hangs on mask_data and proto_data through empty sums, so a backward runs and yields zeros."""
    z = mask_data.new_zeros((), dtype=torch.float32)
    if autograd.wants_grad(mask_data, proto_data):
        z = z + mask_data.reshape(-1)[:0].sum().float() + proto_data.reshape(-1)[:0].sum().float()
    if with_status:
        return z, torch.zeros(1, dtype=torch.int32, device=mask_data.device)
    return z


def lincomb_mask_loss(loc_data, mask_data, proto_data, priors, conf_t, idx_t, gt_masks, mask_alpha=1.0, max_pos=None, want_status=False,
                      mask_proto_crop=True, mask_proto_crop_with_pred_box=True, mask_activation="sigmoid", interpolation_mode="bilinear",
                      use_maskiou=False, use_maskiou_loss=False, mask_proto_coeff_diversity_loss=False, use_mask_scoring=False):
    """losses['M'] of multibox_loss.py:544-616, :636 as a 0-dim fp32 on the device, BEFORE multibox_loss's own division by the batch size.

    loc_data [B,P,4], mask_data [B,P,M], proto_data [B,h,w,M], priors [P,4] or [B,P,4], conf_t and idx_t int64 [B,P] (match_batch's),
    gt_masks: a list of B tensors [G_b,H,W] (uint8, bool or float32), all of one H x W.  Only the configuration every STMask config uses:
    mask_proto_crop and mask_proto_crop_with_pred_box True, sigmoid activation, bilinear interpolation, no mask-IoU terms, no coefficient
    diversity loss, no mask scoring; anything else raises NotImplementedError.

    With r over the positives (conf_t > 0) of the batch in flattened order, b(r) its image, n_b that image's positives and w_r = 1 / max(n_b, 1):
        box_r = clamp(point_form(center_size(decode(loc_r, prior_r)) with width and height * 1.2), 1e-5, 1)       (detached, IEEE fp32)
        M = mask_alpha * sum_r w_r * bce_r / max(bw_r W, 1) / max(bh_r H, 1),
    bce_r the BCE sum over all H * W pixels between mask idx_t[r] of image b(r) and the upsampled generate_mask(proto_data[b(r)], mask_data[r],
    box_r).  An idx_t outside its image's masks is clamped into range on the device: no value of conf_t or idx_t can fault.

    max_pos=None: one host read (the int32 [B+1] prefix of the per-image counts), then every stage runs over exactly n rows.  max_pos=K: no host
    synchronisation at all; every stage runs over K rows, rows past the live count are padding that contributes exact zeros to the loss and to
    every gradient; with more than K positives the loss and the gradients are NaN and the device status word is 1 (want_status=True returns
    (loss, status int32 [1])).  With K >= n the two forms agree to the last bit; n = 0 gives exactly 0.

    Gradients go to mask_data (rows that are not positive: exact zeros) and proto_data (an image without positives: exact zeros); loss and
    gradients are bit-identical from run to run.  Refused from the shapes before any launch: B or P below 1, B * P > 2^22, more than 65535
    rows, M outside {8, 32, 64}, masks of more than one size."""
    if not mask_proto_crop or not mask_proto_crop_with_pred_box or mask_activation != "sigmoid" or interpolation_mode != "bilinear" or \
            use_maskiou or use_maskiou_loss or mask_proto_coeff_diversity_loss or use_mask_scoring:
        raise NotImplementedError("every STMask config crops with the predicted box, uses the sigmoid mask activation and bilinear interpolation "
                                  "and sets use_maskiou, use_maskiou_loss, mask_proto_coeff_diversity_loss and use_mask_scoring to False "
                                  "(config.py); lincomb_mask_loss implements that path only")
    if loc_data.dim() != 3 or loc_data.shape[2] != 4:
        raise ValueError(f"lincomb_mask_loss: loc_data must be [B,P,4], got {tuple(loc_data.shape)}")
    B, P = loc_data.shape[:2]
    if mask_data.dim() != 3 or tuple(mask_data.shape[:2]) != (B, P) or proto_data.dim() != 4 or proto_data.shape[0] != B or \
            proto_data.shape[3] != mask_data.shape[2] or tuple(conf_t.shape) != (B, P) or tuple(idx_t.shape) != (B, P) or len(gt_masks) != B:
        raise ValueError(f"lincomb_mask_loss: mask_data {tuple(mask_data.shape)}, proto_data {tuple(proto_data.shape)}, conf_t "
                         f"{tuple(conf_t.shape)}, idx_t {tuple(idx_t.shape)} and {len(gt_masks)} mask tensors do not fit loc_data "
                         f"{tuple(loc_data.shape)}")
    if max_pos is not None and int(max_pos) < 1:
        raise ValueError(f"lincomb_mask_loss: max_pos={max_pos}")
    sizes = {tuple(m.shape[1:]) for m in gt_masks}
    if len(sizes) != 1 or any(m.dim() != 3 for m in gt_masks):
        raise ValueError(f"lincomb_mask_loss: the masks of a batch must be [G_b,H,W] of one size, got {sorted(sizes)}")
    (H, W), = sizes
    M = mask_data.shape[2]
    ops.mbox_check_shapes("lincomb_mask_loss", B, P, M, None if max_pos is None else int(max_pos))
    ops._dev(loc_data, mask_data, proto_data, priors, conf_t, idx_t, *gt_masks)
    counts = [int(m.shape[0]) for m in gt_masks]
    G_total = sum(counts)
    if G_total == 0:                                                    # no ground truth at all: no mask term
        return _zero_mask_loss(mask_data, proto_data, want_status)
    masks = gt_masks[0] if B == 1 else torch.cat(list(gt_masks))      # concatenated once (a copy, not a synchronisation)
    mask_offs = ops.match_offsets(counts, loc_data.device)
    if mask_data.dtype != torch.float32:
        mask_data = mask_data.float()
    if proto_data.dtype != torch.float32:
        proto_data = proto_data.float()
    priors = priors.detach().float()
    with torch.no_grad():
        prefix, state = ops.mbox_positives(conf_t, max_rows=max_pos)
        n_rows = int(prefix.cpu()[-1]) if max_pos is None else int(max_pos)       # max_pos=None: the one host read
    if n_rows == 0:
        return _zero_mask_loss(mask_data, proto_data, want_status)
    loc = loc_data.detach().float()
    if autograd.wants_grad(mask_data):
        coeff, box, img, idx, scale, n_dev, status = autograd.mbox_gather(mask_data, loc, priors, idx_t, conf_t, mask_offs, state, n_rows, G_total,
                                                                         H, W)
    else:
        rows = ops.mbox_gather(state, n_rows, loc, priors, mask_data.detach(), idx_t, mask_offs, G_total, H, W)
        coeff, box, img, idx, scale, n_dev, status = (rows[k] for k in ("coeff", "box", "img", "idx", "scale", "n_dev", "status"))
    if autograd.wants_grad(coeff, proto_data):
        pred = autograd.lincomb_mask_rows_proto(proto_data, coeff, box, img, n_dev, prefix, status)
    else:
        pred = ops.lincomb_sigmoid_crop(proto_data.detach(), coeff, box, apply_tanh=True, n_dev=n_dev, row_proto=img)
    bce = mask_bce_sum(pred, masks, idx)
    if autograd.wants_grad(bce):
        loss = autograd.mbox_reduce(bce, scale, n_dev, status, mask_alpha)
    else:
        loss = ops.mbox_reduce(bce, scale, n_dev, status, mask_alpha)
    return (loss, status) if want_status else loss


_UNBUILT = dict(use_boxiou_loss=True, train_boxes=True, train_masks=True, train_class=True, train_centerness=True, train_track=True,
                use_sigmoid_focal_loss=False, use_focal_loss=False, use_class_balanced_conf=False, use_semantic_segmentation_loss=False,
                use_maskiou=False, use_maskiou_loss=False, use_mask_scoring=False, mask_proto_loss=None, mask_proto_coeff_diversity_loss=False,
                mask_proto_crop=True, mask_proto_crop_with_pred_box=True, ohem_use_most_confident=False, use_yolo_regressors=False,
                use_prediction_matching=False, use_change_matching=False, maskshift_loss=True)


class MultiBoxLoss(torch.nn.Module):
    """The reference's MultiBoxLoss (layers/modules/multibox_loss.py:15-119) for the STMask configurations, composed of the device functions of
    this package: match_batch, box_center_loss, lincomb_mask_loss, ohem_conf_loss(weights="reference"), track_to_segment_loss and track_loss.
    No Python loop over the images, no boolean gather; the forward makes two small host reads (the prefix of the mask term's and of the shift
    loss's row lists) with max_pos=None and none at all with max_pos=K, forward and backward.

    MultiBoxLoss(num_classes, pos_threshold, neg_threshold, negpos_ratio) as the reference's constructor; the alphas default to the STMask
    configuration's values (bboxiou_alpha=5, center_alpha=20, conf_alpha=6.125, mask_alpha=6.125, track_alpha=5, boxshift_alpha=5,
    maskshift_alpha=6.125); temporal_fusion=True adds B_shift and M_shift; max_pos=K is handed to both row lists.  Flags of the reference's
    config that no STMask config sets to another value (smooth-L1 box loss, focal losses, use_class_balanced_conf, semantic segmentation, the
    mask-IoU net, mask_proto_loss, ...) may be passed by name and raise NotImplementedError unless they have the STMask value.

    forward(net, predictions, gt_bboxes, gt_labels, gt_masks, gt_ids) takes the reference's arguments -- lists of per-clip lists, folded as
    :77-80 fold them; predictions with 'loc', 'conf', 'mask_coeff', 'centerness', 'track', 'priors' ([P,4] or [B,P,4]), 'proto' and
    'T2S_concat_feat'; net.TemporalNet for the shift loss -- and returns the reference's dict {'BIoU', 'M', 'C', 'center', 'B_shift',
    'M_shift', 'T'} of 0-dim fp32 device tensors.  The divisions are the reference's: the terms of multibox_loss() are divided by the batch
    size (:213-214), the shift losses and T are not divided again.  The host NaN / inf print loop of :115-117 is not reproduced (a host read
    per term).

    What the device functions do differently from the reference, restated: losses['center'] sends gradient to loc (the reference does not
    detach smooth-L1's DIoU target, and neither does box_center_loss); losses['T'] is exactly 0, not NaN, with fewer than two positives in the
    batch; losses['C'] uses the reference's positional weights (its cat([positive weights, negative weights]) meets the kept rows in prior
    order)."""

    def __init__(self, num_classes, pos_threshold, neg_threshold, negpos_ratio, bboxiou_alpha=5.0, center_alpha=20.0, conf_alpha=6.125,
                 mask_alpha=6.125, track_alpha=5.0, boxshift_alpha=5.0, maskshift_alpha=6.125, temporal_fusion=True, max_pos=None, **flags):
        super().__init__()
        for name, value in flags.items():
            if name not in _UNBUILT:
                raise TypeError(f"MultiBoxLoss: unknown argument {name!r}")
            if value != _UNBUILT[name]:
                raise NotImplementedError(f"MultiBoxLoss: {name}={value!r}; every STMask config has {name}={_UNBUILT[name]!r} (config.py) and "
                                          "only that path is built")
        if max_pos is not None and int(max_pos) < 1:
            raise ValueError(f"MultiBoxLoss: max_pos={max_pos}")
        self.num_classes = num_classes
        self.pos_threshold, self.neg_threshold, self.negpos_ratio = pos_threshold, neg_threshold, negpos_ratio
        self.bboxiou_alpha, self.center_alpha, self.conf_alpha, self.mask_alpha = bboxiou_alpha, center_alpha, conf_alpha, mask_alpha
        self.track_alpha, self.boxshift_alpha, self.maskshift_alpha = track_alpha, boxshift_alpha, maskshift_alpha
        self.temporal_fusion, self.max_pos = bool(temporal_fusion), max_pos

    def forward(self, net, predictions, gt_bboxes, gt_labels, gt_masks, gt_ids):
        boxes_fold, labels_fold = sum(gt_bboxes, []), sum(gt_labels, [])
        masks_fold, ids_fold = sum(gt_masks, []), sum(gt_ids, [])
        loc_data, conf_data, mask_data = predictions["loc"], predictions["conf"], predictions["mask_coeff"]
        centerness_data, track_data = predictions["centerness"], predictions["track"]
        priors, proto_data = predictions["priors"], predictions["proto"]
        bs = loc_data.shape[0]
        if conf_data.shape[-1] != self.num_classes:
            raise ValueError(f"MultiBoxLoss: conf has {conf_data.shape[-1]} classes, the criterion {self.num_classes}")
        if not (len(boxes_fold) == len(labels_fold) == len(masks_fold) == len(ids_fold) == bs):
            raise ValueError(f"MultiBoxLoss: {len(boxes_fold)} / {len(labels_fold)} / {len(masks_fold)} / {len(ids_fold)} ground-truth entries "
                             f"for a batch of {bs}")
        if priors.dim() == 3 and priors.shape[0] == 1:
            priors = priors[0]
        _, conf_t, idx_t, ids_t, gt_boxes_t = match_batch(self.pos_threshold, self.neg_threshold, boxes_fold, labels_fold, ids_fold, priors,
                                                          conf_data)
        biou, center = box_center_loss(loc_data, priors, gt_boxes_t, conf_t, centerness_data, self.bboxiou_alpha, self.center_alpha)
        m = lincomb_mask_loss(loc_data, mask_data, proto_data, priors, conf_t, idx_t, masks_fold, self.mask_alpha, max_pos=self.max_pos)
        c = ohem_conf_loss(conf_data, conf_t, self.negpos_ratio, self.conf_alpha, weights="reference")
        losses = {"BIoU": biou / bs, "M": m / bs, "C": c / bs, "center": center / bs}                  # :213-214
        if self.temporal_fusion:                                                                        # :102-110
            shift = track_to_segment_loss(net.TemporalNet, predictions["T2S_concat_feat"], loc_data[::2], ids_t[::2], mask_data[::2],
                                          proto_data[1::2], priors if priors.dim() == 2 else priors[0], gt_bboxes, gt_ids, gt_masks,
                                          boxshift_alpha=self.boxshift_alpha, maskshift_alpha=self.maskshift_alpha, max_pos=self.max_pos)
            losses["B_shift"], losses["M_shift"] = shift["B_shift"], shift["M_shift"]
        losses["T"] = track_loss(track_data, conf_t, ids_t, self.track_alpha)                           # :112-113
        return losses
