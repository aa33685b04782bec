"""generate_mask (reference layers/mask_utils.py:111-128): tanh(coeff) -> proto @ coeff^T -> sigmoid -> crop -> [n,h,w],
as ONE fused gfx950 kernel (the reference: matmul + 2 activations + 8 element-wise kernels + permute copy).
When an input requires grad the call goes through autograd.LincombMaskFunction: the same launch, with the backward of
csrc/lincomb_backward.hip behind it.

mask_bce_sum and lincomb_mask_loss_image: the tail of the reference's lincomb_mask_loss (layers/modules/multibox_loss.py:594-616, and :293-317 of
track_to_segment_loss) over csrc/mask_loss.hip -- target gather, bilinear upsampling, clamp, BCE and the per-instance sum in one kernel, its adjoint
in another, nothing at target resolution in between."""
import torch

from .. import autograd, ops


def generate_mask(proto_data, mask_coeff, bbox=None, use_sipmask=False):
    if use_sipmask:
        raise NotImplementedError("use_sipmask is False in every STMask config (config.py:704)")
    if mask_coeff.shape[0] == 0:
        return proto_data.new_zeros(0, proto_data.shape[0], proto_data.shape[1])
    if autograd.wants_grad(proto_data, mask_coeff, bbox):
        return autograd.lincomb_mask(proto_data, mask_coeff, bbox, apply_tanh=True)
    return ops.lincomb_sigmoid_crop(proto_data, mask_coeff, bbox, apply_tanh=True)


def generate_mask_rows(proto_data, mask_coeff, bbox, row_proto, n_dev=None):
    """generate_mask for rows of many clips in one launch: proto_data [bs,h,w,M] (read detached), mask_coeff [n,M], bbox [n,4], row_proto int32 [n]
    (row i uses proto_data[row_proto[i]]), n_dev int32 [1] or None (rows past it are zeros) -> [n,h,w], bit-identical to per-clip generate_mask
    calls.  Gradient w.r.t. mask_coeff only (autograd.LincombRowsFunction over csrc/lincomb_backward.hip)."""
    proto_data = proto_data.detach()
    if proto_data.dim() != 4:
        raise ValueError(f"generate_mask_rows: proto_data must be [bs,h,w,M], got {tuple(proto_data.shape)}")
    if mask_coeff.shape[0] == 0:
        return proto_data.new_zeros(0, proto_data.shape[1], proto_data.shape[2])
    if autograd.wants_grad(mask_coeff):
        return autograd.lincomb_mask_rows(proto_data, mask_coeff, bbox.detach(), row_proto, n_dev)
    return ops.lincomb_sigmoid_crop(proto_data, mask_coeff, bbox, apply_tanh=True, n_dev=n_dev, row_proto=row_proto)


def mask_bce_sum(pred_masks_soft, mask_gt, idx=None):
    """pred_masks_soft [n,h,w] (generate_mask's output), mask_gt [G,H,W] uint8 / bool / float32, idx [n] int64 or None (row i uses mask i) -> [n]:
        F.binary_cross_entropy(clamp(F.interpolate(pred[None], (H, W), mode="bilinear", align_corners=False)[0], 0, 1), mask_gt[idx].float(),
                               reduction="none").sum(dim=(1, 2))
    (multibox_loss.py:575, :598-603 and the sum of :613; :293, :303-309 and :317).  The sigmoid mask activation only (every config's)."""
    if autograd.wants_grad(pred_masks_soft):
        return autograd.mask_bce(pred_masks_soft, mask_gt, idx)
    return ops.mask_bce_upsampled(pred_masks_soft, mask_gt, idx)


def lincomb_mask_loss_image(proto, coeff, boxes, masks_gt, idx, weights, crop=True, min_box=1.0):
    """One image's contribution to loss_m (multibox_loss.py:594-616): proto [h,w,M], coeff [n,M] and boxes [n,4] (point form, relative) of the image's
    positives, masks_gt [G,H,W] with idx [n] the matched mask of each positive, weights [n] -> a scalar.  generate_mask, mask_bce_sum, the division by
    the box's width and height in target pixels (each clamped to at least min_box; None: no clamp, as track_to_segment_loss :315-317), weighted sum.
    crop=False: no crop and the sum divided by H * W instead (:616)."""
    H, W = masks_gt.shape[1:]
    per_inst = mask_bce_sum(generate_mask(proto, coeff, boxes if crop else None), masks_gt, idx)
    if not crop:
        return torch.sum(weights * per_inst) / H / W
    bw, bh = (boxes[:, 2] - boxes[:, 0]) * W, (boxes[:, 3] - boxes[:, 1]) * H          # center_size's width and height
    if min_box is not None:
        bw, bh = torch.clamp(bw, min=min_box), torch.clamp(bh, min=min_box)
    return torch.sum(weights * (per_inst / bw / bh))
