"""T2S_concat_feat, the input of the temporal-fusion loss (reference STMask.py:291-296), from the interleaved maps of a batch of frame pairs.

Two forms of one function.  Composed: the reference's own lines over `correlate` -- four copies of the strided halves, the correlation, cat, relu;
it runs wherever `correlate` runs.  Fused: csrc/t2s_feat.hip reads the halves in place through their batch strides and writes the feature in at
most two launches, its adjoint in at most three (autograd.T2sConcatFeatFunction, include/stmask_hip_t2s_feat.h)."""
import torch
import torch.nn.functional as F

from .. import autograd, ops
from .modules import correlate


def t2s_concat_feat(fpn, t2s, patch_size=11, fused=False):
    """fpn [2 bs, C, h, w] and t2s [2 bs, Cu, h, w], the reference frame of clip b at image 2 b and the next frame at 2 b + 1 ->
    relu(cat([correlate(fpn_ref, fpn_next), t2s_ref, t2s_next], 1)) [bs, P^2 + 2 Cu, h, w]."""
    if fused:
        if autograd.wants_grad(fpn, t2s):
            return autograd.t2s_concat_feat(fpn, t2s, patch_size)
        return ops.t2s_concat_feat(fpn, t2s, patch_size)
    if fpn.dim() != 4 or t2s.dim() != 4 or fpn.shape[0] % 2 or fpn.shape[0] != t2s.shape[0]:
        raise ValueError(f"t2s_concat_feat: fpn {tuple(fpn.shape)} and t2s {tuple(t2s.shape)} must hold the two frames of every clip")
    fpn_ref, fpn_next = fpn[::2].contiguous(), fpn[1::2].contiguous()
    x_ref, x_next = t2s[::2].contiguous(), t2s[1::2].contiguous()
    x_corr = correlate(fpn_ref, fpn_next, patch_size=patch_size)
    return F.relu(torch.cat([x_corr, x_ref, x_next], dim=1))
