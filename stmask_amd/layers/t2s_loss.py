"""The reference's track_to_segment_loss (layers/modules/multibox_loss.py:247-326, called at :102-110) over csrc/t2s_loss.hip and csrc/lincomb_backward.hip: losses['B_shift'] and
losses['M_shift'], the loss that trains TemporalNet.  The reference works clip by clip with a Python loop over the ground-truth ids, a device-to-host
read per id, boolean gathers, a list.index per positive prior, one tiny-batch TemporalNet call per clip and four fp32 [n,H,W] tensors for the mask
term.  Here the targets of the whole batch come from three launches, one gather builds every per-row input, and RoIAlign, TemporalNet, the mask
(generate_mask_rows) and its BCE (mask_bce_sum) each run ONCE over the rows of all clips.  Conventions: include/stmask_hip.h and INTEGRATION.md
section 14."""
import torch

from .. import autograd, ops
from ..mmcv_ops import roi_align
from .mask_utils import generate_mask_rows, mask_bce_sum


def _zero_losses(concat_feat, with_status):
    """Both losses exactly 0; under autograd they hang on concat_feat through an empty sum, so a backward runs and yields zeros."""
    z = concat_feat.new_zeros((), dtype=torch.float32)
    if autograd.wants_grad(concat_feat):
        z = z + concat_feat.reshape(-1)[:0].sum().float()
    out = {"B_shift": z, "M_shift": z.clone()}
    if with_status:
        out["status"] = torch.zeros(1, dtype=torch.int32, device=concat_feat.device)
    return out


def track_to_segment_loss(temporal_net, concat_feat, loc_ref, ids_t_ref, mask_coeff_ref, proto_next, priors, gt_bboxes, gt_ids, gt_masks,
                          boxshift_alpha=1.0, maskshift_alpha=1.0, pool_size=7, max_pos=None, mask_loss=True, crop=True, want_status=False):
    """{'B_shift', 'M_shift'}: 0-dim fp32 on the device, what multibox_loss.py:107-109 returns (there as shape-[1] tensors).

    temporal_net: callable [n,C,pool,pool] -> (bbox_reg [n,4], shift_coeff [n,M]) (net.TemporalNet); concat_feat [bs,C,fh,fw]
    (predictions['T2S_concat_feat']); loc_ref [bs,P,4], ids_t_ref int64 [bs,P], mask_coeff_ref [bs,P,M], proto_next [bs,h,w,M] (what :103-106
    slice; loc_ref, mask_coeff_ref and proto_next are read detached whatever is passed); priors [P,4]; gt_bboxes, gt_ids, gt_masks: lists of bs
    pairs [reference frame, next frame], as the reference's method receives them.  All masks of the batch must have one H x W.

    Prior p of clip i is shift-positive iff ids_t_ref[i,p] > 0 and that id occurs in gt_ids[i][0] and gt_ids[i][1]; with n_i of them in clip i
    and w_r = 1 / n_i:  B_shift = boxshift_alpha / bs * sum_r w_r sum_c smooth_l1(bbox_reg - encode(box_next, center_size(box_ref))),
    M_shift = maskshift_alpha / bs * sum_r w_r bce_r / (bw_r W) / (bh_r H).  A clip without shift-positives contributes exactly 0.  Deviations
    from the reference, all for data it cannot digest: ids are compared as int64; a duplicate id resolves to the last reference index and the
    first next index (the reference raises on the latter); a positive id absent from the reference frame makes the prior not shift-positive.

    max_pos=None: one host read (the int32 [bs+1] prefix of the per-clip counts), then every stage runs over exactly n rows.  max_pos=K: no host
    synchronisation at all; every stage runs over K rows, rows past the live count are padding that contributes exact zeros to both losses and
    to every gradient (they still cost TemporalNet work); if more than K priors are shift-positive both losses and the gradients are NaN and
    the device status word is 1 (want_status=True adds it to the result as 'status', int32 [1]).

    Gradients go to concat_feat (RoIAlign's backward: an fp32 atomic scatter, so that gradient is not bit-reproducible) and to whatever
    temporal_net owns, through torch.  The two losses are bit-identical from run to run."""
    if not mask_loss or not crop:
        raise NotImplementedError("maskshift_loss and mask_proto_crop are True in every temporal-fusion config (config.py); "
                                  "track_to_segment_loss implements that path only")
    if loc_ref.dim() != 3 or loc_ref.shape[2] != 4:
        raise ValueError(f"track_to_segment_loss: loc_ref must be [bs,P,4], got {tuple(loc_ref.shape)}")
    bs, P = loc_ref.shape[:2]
    if len(gt_bboxes) != bs or len(gt_ids) != bs or len(gt_masks) != bs or concat_feat.shape[0] != bs or proto_next.shape[0] != bs:
        raise ValueError(f"track_to_segment_loss: {bs} clips in loc_ref, but {len(gt_bboxes)} / {len(gt_ids)} / {len(gt_masks)} ground-truth "
                         f"pairs, concat_feat {tuple(concat_feat.shape)}, proto_next {tuple(proto_next.shape)}")
    if max_pos is not None and int(max_pos) < 1:
        raise ValueError(f"track_to_segment_loss: max_pos={max_pos}")
    sizes = {tuple(m[1].shape[1:]) for m in gt_masks}
    if len(sizes) != 1:
        raise ValueError(f"track_to_segment_loss: the masks of a batch must have one size, got {sorted(sizes)}")
    (H, W), = sizes
    priors = priors.detach().reshape(-1, 4)
    counts_ref, counts_next = [int(b[0].shape[0]) for b in gt_bboxes], [int(b[1].shape[0]) for b in gt_bboxes]
    if sum(counts_ref) == 0 or sum(counts_next) == 0:
        return _zero_losses(concat_feat, want_status)
    # the ground truth of the two frames, concatenated once (a copy, not a synchronisation)
    boxes_ref = torch.cat([b[0].reshape(-1, 4) for b in gt_bboxes]).detach().float()
    boxes_next = torch.cat([b[1].reshape(-1, 4) for b in gt_bboxes]).detach().float()
    ids_ref = torch.cat([i[0].reshape(-1) for i in gt_ids]).to(torch.int64)
    ids_next = torch.cat([i[1].reshape(-1) for i in gt_ids]).to(torch.int64)
    masks_next = gt_masks[0][1] if bs == 1 else torch.cat([m[1] for m in gt_masks])
    if masks_next.shape[0] != boxes_next.shape[0]:
        raise ValueError(f"track_to_segment_loss: {masks_next.shape[0]} next-frame masks for {boxes_next.shape[0]} boxes")
    fh, fw = concat_feat.shape[2:]
    with torch.no_grad():
        _, reg_t, idx_next, prefix, state = ops.t2s_targets(ids_t_ref, boxes_ref, ids_ref, counts_ref, boxes_next, ids_next, counts_next,
                                                            max_rows=max_pos)
        n_rows = int(prefix.cpu()[-1]) if max_pos is None else int(max_pos)           # max_pos=None: the one host read
    if n_rows == 0:
        return _zero_losses(concat_feat, want_status)
    with torch.no_grad():
        rows = ops.t2s_gather(state, n_rows, loc_ref.detach(), priors, mask_coeff_ref.detach(), reg_t, idx_next, boxes_next, fh, fw)
    feats = roi_align(concat_feat if concat_feat.dtype == torch.float32 else concat_feat.float(), rows["rois"], pool_size)
    bbox_reg, shift_coeff = temporal_net(feats)
    bbox_reg = bbox_reg.float().contiguous()
    coeff = rows["coeff"] + shift_coeff.float()
    pred = generate_mask_rows(proto_next, coeff, rows["box"], rows["clip"], rows["n_dev"])
    bce = mask_bce_sum(pred, masks_next, rows["idx"])
    args = (rows["reg"], rows["box"], rows["w"], rows["n_dev"], rows["status"], bs, H, W, boxshift_alpha, maskshift_alpha)
    if autograd.wants_grad(bbox_reg, bce):
        b_shift, m_shift = autograd.t2s_reduce(bbox_reg, bce, *args)
    else:
        b_shift, m_shift = ops.t2s_reduce(bbox_reg, args[0], bce, *args[1:])
    out = {"B_shift": b_shift, "M_shift": m_shift}
    if want_status:
        out["status"] = rows["status"]
    return out
