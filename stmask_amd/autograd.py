"""Autograd for the drop-in deformable convolution, RoIAlign and correlation (the training path of dcn_v2 / mmcv.ops /
spatial_correlation_sampler) and for the layer functions the reference's loss differentiates through -- generate_mask, decode, jaccard and
the mask loss tail mask_bce_sum, the OHEM class-confidence loss ohem_conf_loss, the positive-prior terms box_center_loss and track_loss and
the pieces of track_to_segment_loss: the row-prototype form of generate_mask and the two weighted reductions, and the pieces of the batched
mask term lincomb_mask_loss: its gather, the row-prototype mask with a prototype gradient and its reduction; and for
T2S_concat_feat of the train-mode forward in its fused form (csrc/t2s_feat.hip).

Each Function's forward is the launch the shim makes without autograd (ops.deform_conv / roi_align / corr_patch), so values under
autograd are bit-identical to the no-grad call.  Only inputs are saved: the deformable columns are recomputed in backward with the
forward's own im2col, the mask sigmoid from the prototypes and coefficients.  Backward runs the gfx950 kernels of csrc/deform_backward.hip,
csrc/temporal_backward.hip, csrc/mask_backward.hip, csrc/lincomb_backward.hip, csrc/mask_loss.hip, csrc/conf_loss.hip, csrc/pos_loss.hip, csrc/t2s_loss.hip and
csrc/mbox_loss.hip on the current stream; a gradient nobody asked for (ctx.needs_input_grad) launches nothing.  The backward kernels have no derivative of their own, so
every backward is @first_order_only: a double backward (create_graph=True, then differentiating the result) raises instead of
silently dropping the second-order term.

Deterministic mode.  Two of these backwards scatter with fp32 atomic adds -- grad_x of the deformable convolutions and
grad_feat of RoIAlign -- and torch's own bilinear-upsampling backward does too (under torch.use_deterministic_algorithms(True) torch raises, or, from
the release on that swaps in a decomposition, runs another forward whose values differ in the last bits).  With the
mode on, ops.deform_col2im and ops.roi_align_backward take the order-independent 64-bit fixed-point form of csrc/det_backward.hip, and FPN /
InterpolateModule differentiate their bilinear upsampling through UpsampleBilinearFunction, a gather.  The mode is read where the backward launch
is chosen, not when the forward ran.  Off (the default without torch's flag), every call makes exactly the launches it made before.
"""
import functools

import torch

from . import ops

_deterministic = None   # set_deterministic(): True / False, or None = follow torch's flag


def set_deterministic(mode):
    """True / False: the deterministic backward on / off.  None (the default): follow torch.are_deterministic_algorithms_enabled(), which is also
    true under torch.use_deterministic_algorithms(True, warn_only=True).  False while torch's flag is on: the atomic scatters are taken and raise
    (warn, with warn_only) as torch's own nondeterministic operators do under the flag (ops._alert_not_deterministic)."""
    global _deterministic
    if mode is not None and not isinstance(mode, bool):
        raise ValueError(f"set_deterministic: mode must be True, False or None, got {mode!r}")
    _deterministic = mode


def is_deterministic():
    """Whether a backward launched now takes the deterministic kernels."""
    return torch.are_deterministic_algorithms_enabled() if _deterministic is None else _deterministic


def wants_grad(*tensors):
    """The shims take the autograd path only when grad mode is on and some tensor input or parameter requires grad."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class _NotTwiceDifferentiable(torch.autograd.Function):
    """Identity on `grad`; the other arguments are what `grad` was computed from.  Differentiating through it raises."""

    @staticmethod
    def forward(ctx, grad, *made_from):
        return grad.view_as(grad)

    @staticmethod
    def backward(ctx, *grads):
        raise RuntimeError("stmask_amd: the drop-ins' backward kernels are not differentiable (no double backward): a gradient made with "
                           "create_graph=True cannot be differentiated again")


def first_order_only(backward):
    """For a Function.backward made of kernel launches.  torch's once_differentiable raises only when the incoming grad_out requires grad; under
    create_graph=True the gradients also depend on the saved inputs (grad_x on the weight and the offsets, ...), and a later backward through
    them would silently miss that term.  Here every returned gradient is tied to grad_out AND the saved tensors by a node that raises."""
    @functools.wraps(backward)
    def wrapper(ctx, *grad_outs):
        if not torch.is_grad_enabled():             # the usual backward pass
            return backward(ctx, *grad_outs)
        with torch.no_grad():
            outs = backward(ctx, *grad_outs)
        made_from = [t for t in (*grad_outs, *ctx.saved_tensors) if t is not None and t.requires_grad]
        if not made_from:
            return outs
        return tuple(o if o is None else _NotTwiceDifferentiable.apply(o, *made_from) for o in outs)
    return wrapper


class ModulatedDeformConvFunction(torch.autograd.Function):
    """dcn_v2 DCNv2: y = deform_conv(x, offset, mask, weight, bias).  With fused=True `offset` is DCN's raw conv_offset_mask output
    (offsets, then mask logits; the sigmoid is applied in-kernel) and `mask` is None: the gradient returned for it is the gradient
    w.r.t. those raw channels."""

    @staticmethod
    def forward(ctx, x, offset, mask, weight, bias, stride, padding, dilation, deform_groups, fused):
        ctx.conv = (stride, padding, dilation, deform_groups, fused)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, offset, mask, weight)
        if fused:
            return ops.deform_conv(x, None, None, weight, bias, stride, padding, dilation, deform_groups, fused_om=offset)
        return ops.deform_conv(x, offset, mask, weight, bias, stride, padding, dilation, deform_groups)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        x, offset, mask, weight = ctx.saved_tensors
        stride, padding, dilation, dg, fused = ctx.conv
        nx, noff, nmask, nw, nb = ctx.needs_input_grad[:5]
        need = (nx, noff, nmask and mask is not None, nw, nb and ctx.has_bias)
        if not any(need):
            return (None,) * 10
        if fused:
            gx, goff, _, gw, gb = ops.deform_conv_backward(grad_out.contiguous(), x, None, None, weight, stride, padding, dilation, dg,
                                                           fused_om=offset, need=(nx, noff, noff, nw, need[4]))
            return gx, goff, None, gw, gb, None, None, None, None, None
        gx, goff, gmask, gw, gb = ops.deform_conv_backward(grad_out.contiguous(), x, offset, mask, weight, stride, padding, dilation, dg,
                                                           need=need)
        return gx, goff, gmask, gw, gb, None, None, None, None, None


class DeformConvFunction(torch.autograd.Function):
    """mmcv DeformConv2d (v1: no mask, no bias): y = deform_conv(x, offset, None, weight)."""

    @staticmethod
    def forward(ctx, x, offset, weight, stride, padding, dilation, deform_groups):
        ctx.conv = (stride, padding, dilation, deform_groups)
        ctx.save_for_backward(x, offset, weight)
        return ops.deform_conv(x, offset, None, weight, None, stride, padding, dilation, deform_groups)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        x, offset, weight = ctx.saved_tensors
        stride, padding, dilation, dg = ctx.conv
        nx, noff, nw = ctx.needs_input_grad[:3]
        if not (nx or noff or nw):
            return (None,) * 7
        gx, goff, _, gw, _ = ops.deform_conv_backward(grad_out.contiguous(), x, offset, None, weight, stride, padding, dilation, dg,
                                                      need=(nx, noff, False, nw, False))
        return gx, goff, gw, None, None, None, None


class RoIAlignFunction(torch.autograd.Function):
    """mmcv roi_align (avg): gradient w.r.t. the feature map only (mmcv returns none for the RoIs)."""

    @staticmethod
    def forward(ctx, feat, rois, output_size, spatial_scale, sampling_ratio, aligned):
        ctx.args = (tuple(feat.shape), output_size, spatial_scale, sampling_ratio, aligned)
        ctx.save_for_backward(rois)
        return ops.roi_align(feat, rois, output_size, spatial_scale, sampling_ratio, aligned)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        (rois,) = ctx.saved_tensors
        shape, output_size, spatial_scale, sampling_ratio, aligned = ctx.args
        gfeat = ops.roi_align_backward(grad_out.contiguous(), rois, shape, output_size, spatial_scale, sampling_ratio, aligned)
        return gfeat, None, None, None, None, None


class CorrelationFunction(torch.autograd.Function):
    """spatial_correlation_sample(kernel_size=1, patch_size=P, dilation_patch=d): [B,C,H,W] x 2 -> [B,P,P,H,W]."""

    @staticmethod
    def forward(ctx, in1, in2, patch_size, dilation_patch):
        ctx.dil = dilation_patch
        ctx.save_for_backward(in1, in2)
        return ops.corr_patch(in1, in2, patch_size, dilation_patch)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        n1, n2 = ctx.needs_input_grad[:2]
        if not (n1 or n2):
            return None, None, None, None
        in1, in2 = ctx.saved_tensors
        g1, g2 = ops.corr_patch_backward(grad_out.contiguous(), in1, in2, ctx.dil, need1=n1, need2=n2)
        return g1, g2, None, None


class T2sConcatFeatFunction(torch.autograd.Function):
    """layers.t2s_concat_feat(fused=True): the interleaved fpn / t2s maps of a batch of frame pairs -> T2S_concat_feat (csrc/t2s_feat.hip).  Saved:
    the two inputs and the output, whose sign is the correlation channels' gate."""

    @staticmethod
    def forward(ctx, fpn, t2s, patch_size):
        ctx.patch_size = patch_size
        out = ops.t2s_concat_feat(fpn, t2s, patch_size)
        ctx.save_for_backward(fpn, t2s, out)
        return out

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        n_fpn, n_t2s = ctx.needs_input_grad[:2]
        if not (n_fpn or n_t2s):
            return None, None, None
        fpn, t2s, out = ctx.saved_tensors
        g_fpn, g_t2s = ops.t2s_concat_feat_backward(grad_out, out, fpn, t2s, ctx.patch_size, need_fpn=n_fpn, need_t2s=n_t2s)
        return g_fpn, g_t2s, None


class LincombMaskFunction(torch.autograd.Function):
    """generate_mask: sigmoid(proto @ tanh(coeff)^T) cropped to the boxes, [h,w,M] x [n,M] -> [n,h,w].  No gradient w.r.t. the boxes (the
    reference's crop has none)."""

    @staticmethod
    def forward(ctx, proto, coeff, boxes, apply_tanh):
        ctx.apply_tanh = apply_tanh
        ctx.save_for_backward(proto, coeff, boxes)
        return ops.lincomb_sigmoid_crop(proto, coeff, boxes, apply_tanh=apply_tanh)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        np_, nc = ctx.needs_input_grad[:2]
        if not (np_ or nc):
            return None, None, None, None
        proto, coeff, boxes = ctx.saved_tensors
        gp, gc = ops.lincomb_sigmoid_crop_backward(grad_out.contiguous(), proto, coeff, boxes, ctx.apply_tanh, need_proto=np_, need_coeff=nc)
        return gp, gc, None, None


class DecodeFunction(torch.autograd.Function):
    """box_utils.decode: loc [n,4], priors [n,4] -> point-form boxes [n,4]."""

    @staticmethod
    def forward(ctx, loc, priors):
        ctx.save_for_backward(loc, priors)
        return ops.decode(loc, priors)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_boxes):
        nl, npr = ctx.needs_input_grad[:2]
        if not (nl or npr):
            return None, None
        loc, priors = ctx.saved_tensors
        return ops.decode_backward(grad_boxes.contiguous(), loc, priors, need_loc=nl, need_priors=npr)


class JaccardFunction(torch.autograd.Function):
    """box_utils.jaccard, 2-D form: [A,4] x [B,4] -> [A,B]."""

    @staticmethod
    def forward(ctx, box_a, box_b):
        ctx.save_for_backward(box_a, box_b)
        return ops.jaccard(box_a, box_b)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        na, nb = ctx.needs_input_grad[:2]
        if not (na or nb):
            return None, None
        a, b = ctx.saved_tensors
        return ops.jaccard_backward(grad_out.contiguous(), a, b, need_a=na, need_b=nb)


class MaskBceFunction(torch.autograd.Function):
    """mask_bce_upsampled: pred [n,h,w], target [G,H,W], idx [n] or None -> loss [n].  Gradient w.r.t. pred only (the targets and the index are data)."""

    @staticmethod
    def forward(ctx, pred, target, idx):
        ctx.save_for_backward(pred, target, idx)
        return ops.mask_bce_upsampled(pred, target, idx)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        pred, target, idx = ctx.saved_tensors
        return ops.mask_bce_upsampled_backward(grad_loss.contiguous(), pred, target, idx), None, None


class OhemConfLossFunction(torch.autograd.Function):
    """ohem_conf_loss: conf_data [B,P,C], conf_t [B,P] -> losses['C'].  Saved: the inputs and the two [N] fp32 vectors lse and w, nothing of
    size N * C.  The selection is a constant of the backward; no gradient w.r.t. conf_t."""

    @staticmethod
    def forward(ctx, conf_data, conf_t, negpos_ratio, conf_alpha, weights):
        loss, lse, w = ops.ohem_conf_loss(conf_data, conf_t, negpos_ratio, conf_alpha, weights)
        ctx.args = (negpos_ratio, conf_alpha)
        ctx.save_for_backward(conf_data, conf_t, lse, w)
        return loss

    @staticmethod
    @first_order_only
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        conf_data, conf_t, lse, w = ctx.saved_tensors
        return ops.ohem_conf_loss_backward(grad_loss.contiguous(), conf_data, conf_t, lse, w, *ctx.args), None, None, None, None


class BoxCenterLossFunction(torch.autograd.Function):
    """box_center_loss: loc_data [B,P,4], centerness_data [B,P,1] or None -> (losses['BIoU'], losses['center']).  Saved: the inputs and the [B]
    int32 counts of positives.  Gradients w.r.t. loc_data and centerness_data only; losses['center'] reaches loc_data too (the reference does
    not detach smooth-L1's target)."""

    @staticmethod
    def forward(ctx, loc_data, centerness_data, priors, gt_boxes_t, conf_t, bboxiou_alpha, center_alpha):
        biou, center, npos = ops.box_center_loss(loc_data, priors, gt_boxes_t, conf_t, centerness_data, bboxiou_alpha, center_alpha)
        ctx.args = (bboxiou_alpha, center_alpha)
        ctx.save_for_backward(loc_data, centerness_data, priors, gt_boxes_t, conf_t, npos)
        if center is None:
            return biou
        return biou, center

    @staticmethod
    @first_order_only
    def backward(ctx, grad_biou, grad_center=None):
        nl, nc = ctx.needs_input_grad[:2]
        if not (nl or nc):
            return (None,) * 7
        loc_data, centerness_data, priors, gt_boxes_t, conf_t, npos = ctx.saved_tensors
        gl, gc = ops.box_center_loss_backward(grad_biou, grad_center, loc_data, priors, gt_boxes_t, conf_t, centerness_data, npos, *ctx.args,
                                              need_centerness=nc)
        return (gl if nl else None), gc, None, None, None, None, None


class TrackLossFunction(torch.autograd.Function):
    """track_loss: track_data [B,P,D], conf_t, ids_t [B,P] -> losses['T'].  Saved: the inputs, nothing of size n x n or n x D."""

    @staticmethod
    def forward(ctx, track_data, conf_t, ids_t, track_alpha):
        ctx.alpha = track_alpha
        ctx.save_for_backward(track_data, conf_t, ids_t)
        return ops.track_loss(track_data, conf_t, ids_t, track_alpha)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        track_data, conf_t, ids_t = ctx.saved_tensors
        return ops.track_loss_backward(grad_loss.contiguous(), track_data, conf_t, ids_t, ctx.alpha), None, None, None


class LincombRowsFunction(torch.autograd.Function):
    """generate_mask over the rows of many prototype sets: proto [S,h,w,M] (read detached), coeff [n,M], boxes [n,4], row_proto int32 [n],
    n_dev int32 [1] or None -> [n,h,w].  Gradient w.r.t. the coefficients only."""

    @staticmethod
    def forward(ctx, coeff, proto, boxes, row_proto, n_dev):
        ctx.save_for_backward(coeff, proto, boxes, row_proto, n_dev)
        return ops.lincomb_sigmoid_crop(proto, coeff, boxes, apply_tanh=True, n_dev=n_dev, row_proto=row_proto)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        coeff, proto, boxes, row_proto, n_dev = ctx.saved_tensors
        return ops.lincomb_rows_backward(grad_out.contiguous(), proto, coeff, boxes, row_proto, n_dev, apply_tanh=True), None, None, None, None


class T2sReduceFunction(torch.autograd.Function):
    """The two weighted sums of track_to_segment_loss: bbox_reg [n,4], bce [n] and the rows of ops.t2s_gather -> (B_shift, M_shift).  Gradients
    w.r.t. bbox_reg and bce only."""

    @staticmethod
    def forward(ctx, bbox_reg, bce, reg_rows, box_rows, w_rows, n_dev, status, bs, H, W, boxshift_alpha, maskshift_alpha):
        ctx.args = (bs, H, W, boxshift_alpha, maskshift_alpha)
        ctx.save_for_backward(bbox_reg, reg_rows, box_rows, w_rows, n_dev, status)
        return ops.t2s_reduce(bbox_reg, reg_rows, bce, box_rows, w_rows, n_dev, status, *ctx.args)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_b, grad_m):
        nr, nb = ctx.needs_input_grad[:2]
        if not (nr or nb):
            return (None,) * 12
        bbox_reg, reg_rows, box_rows, w_rows, n_dev, status = ctx.saved_tensors
        g_reg, g_bce = ops.t2s_reduce_backward(grad_b, grad_m, bbox_reg, reg_rows, box_rows, w_rows, n_dev, status, *ctx.args, need_reg=nr,
                                               need_bce=nb)
        return (g_reg, g_bce) + (None,) * 10


class MboxGatherFunction(torch.autograd.Function):
    """The gather of lincomb_mask_loss: mask_data [B,P,M] through the list of positives -> (coeff [n,M], box [n,4], img, idx, scale, n_dev,
    status) of ops.mbox_gather.  Gradient w.r.t. mask_data only, from the coefficient rows: list rows are unique, so every row of grad mask_data
    is written once and the rows that are not positive are exact zeros."""

    @staticmethod
    def forward(ctx, mask_data, loc_data, priors, idx_t, conf_t, mask_offs, state, n_rows, G_total, H, W):
        rows = ops.mbox_gather(state, n_rows, loc_data, priors, mask_data, idx_t, mask_offs, G_total, H, W)
        ctx.save_for_backward(conf_t, state, rows["n_dev"], rows["status"])
        outs = tuple(rows[k] for k in ("coeff", "box", "img", "idx", "scale", "n_dev", "status"))
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    @first_order_only
    def backward(ctx, grad_coeff, *unused):
        if not ctx.needs_input_grad[0]:
            return (None,) * 11
        conf_t, state, n_dev, status = ctx.saved_tensors
        return (ops.mbox_scatter_coeff(grad_coeff.contiguous(), conf_t, state, n_dev, status),) + (None,) * 10


class LincombRowsProtoFunction(torch.autograd.Function):
    """generate_mask over the rows of many prototype sets, the rows sorted by set: proto [S,h,w,M], coeff [n,M], boxes [n,4], row_proto int32
    [n], n_dev int32 [1], prefix int32 [S+1] (rows prefix[s] .. prefix[s+1] use set s), status int32 [1] -> [n,h,w].  Gradients w.r.t. the
    coefficients and the prototypes (both csrc/lincomb_backward.hip)."""

    @staticmethod
    def forward(ctx, coeff, proto, boxes, row_proto, n_dev, prefix, status):
        ctx.save_for_backward(coeff, proto, boxes, row_proto, n_dev, prefix, status)
        return ops.lincomb_sigmoid_crop(proto, coeff, boxes, apply_tanh=True, n_dev=n_dev, row_proto=row_proto)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        nc, np_ = ctx.needs_input_grad[:2]
        if not (nc or np_):
            return (None,) * 7
        coeff, proto, boxes, row_proto, n_dev, prefix, status = ctx.saved_tensors
        go = grad_out.contiguous()
        gc = ops.lincomb_rows_backward(go, proto, coeff, boxes, row_proto, n_dev, apply_tanh=True) if nc else None
        gp = ops.lincomb_rows_proto_backward(go, proto, coeff, boxes, prefix, status) if np_ else None
        return (gc, gp) + (None,) * 5


class MboxReduceFunction(torch.autograd.Function):
    """The weighted sum of lincomb_mask_loss: bce [n] and the scale rows of ops.mbox_gather -> losses['M'].  Gradient w.r.t. bce only."""

    @staticmethod
    def forward(ctx, bce, scale_rows, n_dev, status, mask_alpha):
        ctx.alpha = mask_alpha
        ctx.save_for_backward(scale_rows, n_dev, status)
        return ops.mbox_reduce(bce, scale_rows, n_dev, status, mask_alpha)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        scale_rows, n_dev, status = ctx.saved_tensors
        return (ops.mbox_reduce_backward(grad_loss.contiguous(), scale_rows, n_dev, status, ctx.alpha),) + (None,) * 4


class UpsampleBilinearFunction(torch.autograd.Function):
    """F.interpolate(x, size= or scale_factor=, mode="bilinear", align_corners=False) on [B,C,H,W]: the forward is the ATen kernel that call
    launches, so values are torch's bit for bit; the backward is the gather of csrc/det_backward.hip (fixed order, no atomics) instead of torch's
    atomic scatter.  Only shapes are saved.
    The kernel is called by its own name because F.interpolate itself, on a GPU tensor under torch.use_deterministic_algorithms(True), swaps it for
    a slow decomposition (torch._decomp) whose VALUES differ in the last bits from those of the kernel: with this Function the forward under the
    flag is the forward without it."""

    @staticmethod
    def forward(ctx, x, size, scale_factor):
        if (size is None) == (scale_factor is None):
            raise ValueError("upsample_bilinear: exactly one of size and scale_factor")
        if size is not None:
            out_size, factors = ([size, size] if isinstance(size, int) else list(size)), None
        else:
            out_size, factors = None, ([float(scale_factor)] * 2 if isinstance(scale_factor, (int, float)) else [float(v) for v in scale_factor])
        ctx.in_shape, ctx.scale_factor = tuple(x.shape), scale_factor
        return torch._C._nn.upsample_bilinear2d(x, out_size, False, factors)     # what F.interpolate calls (recompute_scale_factor=None)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return ops.upsample_bilinear_backward(grad_out.contiguous(), ctx.in_shape, ctx.scale_factor), None, None


def takes_upsample_kernel(x, mode, align_corners):
    """Whether FPN / InterpolateModule differentiate this interpolation through UpsampleBilinearFunction: the deterministic mode is on, the tensor is
    on the GPU, a gradient is wanted, and it is the bilinear, align_corners=False form the kernel is the adjoint of."""
    return (mode == "bilinear" and align_corners is False and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and wants_grad(x)
            and is_deterministic())


def upsample_bilinear(x, size=None, scale_factor=None):
    return UpsampleBilinearFunction.apply(x, size, scale_factor)


def modulated_deform_conv(x, offset, mask, weight, bias, stride, padding, dilation, deform_groups):
    return ModulatedDeformConvFunction.apply(x, offset, mask, weight, bias, stride, padding, dilation, deform_groups, False)


def modulated_deform_conv_fused(x, om, weight, bias, stride, padding, dilation, deform_groups):
    return ModulatedDeformConvFunction.apply(x, om, None, weight, bias, stride, padding, dilation, deform_groups, True)


def deform_conv(x, offset, weight, stride, padding, dilation, deform_groups):
    return DeformConvFunction.apply(x, offset, weight, stride, padding, dilation, deform_groups)


def roi_align(feat, rois, output_size, spatial_scale, sampling_ratio, aligned):
    return RoIAlignFunction.apply(feat, rois, output_size, spatial_scale, sampling_ratio, aligned)


def correlation(in1, in2, patch_size, dilation_patch):
    return CorrelationFunction.apply(in1, in2, patch_size, dilation_patch)


def t2s_concat_feat(fpn, t2s, patch_size=11):
    return T2sConcatFeatFunction.apply(fpn, t2s, patch_size)


def lincomb_mask(proto, coeff, boxes=None, apply_tanh=True):
    return LincombMaskFunction.apply(proto, coeff, boxes, apply_tanh)


def decode(loc, priors):
    return DecodeFunction.apply(loc, priors)


def jaccard(box_a, box_b):
    return JaccardFunction.apply(box_a, box_b)


def mask_bce(pred, target, idx=None):
    return MaskBceFunction.apply(pred, target, idx)


def ohem_conf_loss(conf_data, conf_t, negpos_ratio=3, conf_alpha=1.0, weights="reference"):
    return OhemConfLossFunction.apply(conf_data, conf_t, negpos_ratio, conf_alpha, weights)


def box_center_loss(loc_data, priors, gt_boxes_t, conf_t, centerness_data=None, bboxiou_alpha=1.0, center_alpha=1.0):
    out = BoxCenterLossFunction.apply(loc_data, centerness_data, priors, gt_boxes_t, conf_t, bboxiou_alpha, center_alpha)
    return (out, None) if centerness_data is None else out


def track_loss(track_data, conf_t, ids_t, track_alpha=1.0):
    return TrackLossFunction.apply(track_data, conf_t, ids_t, track_alpha)


def lincomb_mask_rows(proto, coeff, boxes, row_proto, n_dev=None):
    return LincombRowsFunction.apply(coeff, proto, boxes, row_proto, n_dev)


def t2s_reduce(bbox_reg, bce, reg_rows, box_rows, w_rows, n_dev, status, bs, H, W, boxshift_alpha=1.0, maskshift_alpha=1.0):
    return T2sReduceFunction.apply(bbox_reg, bce, reg_rows, box_rows, w_rows, n_dev, status, bs, H, W, boxshift_alpha, maskshift_alpha)


def mbox_gather(mask_data, loc_data, priors, idx_t, conf_t, mask_offs, state, n_rows, G_total, H, W):
    return MboxGatherFunction.apply(mask_data, loc_data, priors, idx_t, conf_t, mask_offs, state, n_rows, G_total, H, W)


def lincomb_mask_rows_proto(proto, coeff, boxes, row_proto, n_dev, prefix, status):
    return LincombRowsProtoFunction.apply(coeff, proto, boxes, row_proto, n_dev, prefix, status)


def mbox_reduce(bce, scale_rows, n_dev, status, mask_alpha=1.0):
    return MboxReduceFunction.apply(bce, scale_rows, n_dev, status, mask_alpha)
