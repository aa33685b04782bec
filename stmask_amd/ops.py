"""Tensor-level wrappers over the C ABI (include/stmask_hip.h).

Each function takes CUDA(=HIP) torch tensors, allocates outputs with torch (device memory + stream plumbing only)
and enqueues the hand-written gfx950 kernel on the current stream.  CPU tensors are rejected: the product path has
no CPU fallback (oracle/ is test infrastructure and is never imported from here).
"""
import ctypes
import os
import warnings

import torch

from . import _lib
from ._lib import DeformGeom, StmError, c_p, call


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise StmError("stmask_amd ops need tensors on the MI355X (got a CPU tensor); there is no CPU fallback")


def _f32c(t):
    if t.dtype != torch.float32:
        raise StmError(f"expected float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _p(t):
    return c_p(t.data_ptr()) if t is not None else c_p(0)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """The current HIP stream of the current device as a C pointer.  torch.cuda.current_stream() builds a Stream object through four Python layers
    (8 us a call, ~22 calls per single-stream step: 16 % of it, profiles/r06_prof_host_clips1.txt); the raw getter is one C call."""
    if _raw_stream is not None:
        return c_p(_raw_stream(torch.cuda.current_device()))
    return c_p(torch.cuda.current_stream().cuda_stream)


def conv_out_hw(H, W, kh, kw, sh, sw, ph, pw, dh, dw):
    return ((H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1)


def _geom(x, kernel_size, stride, padding, dilation, dg):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
    B, C, H, W = x.shape
    Ho, Wo = conv_out_hw(H, W, kh, kw, sh, sw, ph, pw, dh, dw)
    return DeformGeom(B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, dg, Ho, Wo)


def _offset_mask_views(offset, mask, g, fused_om):
    """Returns (off_tensor, off_bstride, mask_tensor_or_None, mask_ptr, mask_bstride)."""
    K, HWo = g.kh * g.kw, g.Ho * g.Wo
    if fused_om is not None:
        # raw conv_offset_mask output [B, dg*3K, Ho, Wo]: dcn_v2 chunks it into (o1, o2, mask) and uses
        # cat(o1, o2) as the offset, i.e. channels [0, 2*dg*K) are the offsets and [2*dg*K, 3*dg*K) the mask logits
        om = _f32c(fused_om)
        if tuple(om.shape) != (g.B, g.dg * 3 * K, g.Ho, g.Wo):
            raise StmError(f"conv_offset_mask output {tuple(om.shape)} != {(g.B, g.dg * 3 * K, g.Ho, g.Wo)}")
        bs = g.dg * 3 * K * HWo
        return om, bs, om, om.data_ptr() + 4 * g.dg * 2 * K * HWo, bs
    offset = _f32c(offset)
    if tuple(offset.shape) != (g.B, g.dg * 2 * K, g.Ho, g.Wo):
        raise StmError(f"offset shape {tuple(offset.shape)} != {(g.B, g.dg * 2 * K, g.Ho, g.Wo)}")
    if mask is not None:
        mask = _f32c(mask)
        if tuple(mask.shape) != (g.B, g.dg * K, g.Ho, g.Wo):
            raise StmError(f"mask shape {tuple(mask.shape)} != {(g.B, g.dg * K, g.Ho, g.Wo)}")
        return offset, g.dg * 2 * K * HWo, mask, mask.data_ptr(), g.dg * K * HWo
    return offset, g.dg * 2 * K * HWo, None, 0, 0


def deform_im2col(x, offset, mask, kernel_size, stride=1, padding=0, dilation=1, deform_groups=1, variant=0,
                  fused_om=None, mask_is_logit=False, out=None):
    """Modulated deformable im2col -> cols [B, C*kh*kw, Ho*Wo] (mask=None -> v1)."""
    _dev(x, offset, mask, fused_om)
    x = _f32c(x)
    g = _geom(x, kernel_size, stride, padding, dilation, deform_groups)
    off, obs, mk, mk_ptr, mbs = _offset_mask_views(offset, mask, g, fused_om)
    cols = out if out is not None else torch.empty(g.B, g.C * g.kh * g.kw, g.Ho * g.Wo, device=x.device, dtype=torch.float32)
    call("stm_deform_im2col_f32", _p(x), _p(off), obs, c_p(mk_ptr), mbs, 1 if (mask_is_logit or fused_om is not None) else 0, _p(cols),
         ctypes.byref(g), variant, _stream())
    return cols


_ws_cache = {}
_ws_scope = None   # a dict owned by a pipeline while it captures HIP graphs (workspace_scope)


class workspace_scope:
    """`with workspace_scope(store):` -- every _workspace() request inside comes from `store` (keyed by device and tag, not by
    stream) and the owner of `store` keeps the buffers alive.  BatchedClipPipeline captures its trunk graphs under one: the
    scratch pointers baked into a graph (split-K partial sums, column buffers) then belong to the pipeline, not to the
    throw-away capture stream's slot of the global cache -- PyTorch recycles stream handles from a pool of 32, so a later
    pipeline could otherwise be handed the same (device, stream) key, outgrow the buffer and free it under a live graph.
    A buffer that must grow inside a scope is retired into the store, never freed."""

    def __init__(self, store):
        self.store = store

    def __enter__(self):
        global _ws_scope
        self.saved, _ws_scope = _ws_scope, self.store
        return self.store

    def __exit__(self, *exc):
        global _ws_scope
        _ws_scope = self.saved
        return False


_ws_branch = ""    # suffix of every workspace tag while a side branch of the trunk runs (workspace_branch)


class workspace_branch:
    """`with workspace_branch("proto"):` -- scratch requested inside gets its own buffers (tag + suffix).  PlanarGraph runs independent parts of the
    trunk on a second stream while a HIP graph is captured; inside a workspace_scope scratch is keyed by tag, not by stream, so two branches that
    both park split-K partial sums would otherwise share one buffer."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        global _ws_branch
        self.saved, _ws_branch = _ws_branch, "/" + self.name
        return self

    def __exit__(self, *exc):
        global _ws_branch
        _ws_branch = self.saved
        return False


def _workspace(nbytes, device, tag="ws"):
    """Grow-only scratch buffer per (device, stream, tag) -- or per (device, tag) of the active workspace_scope
    (cols buffers are GBs at large batch: never allocated per call)."""
    tag = tag + _ws_branch
    if _ws_scope is not None:
        key = (device.index, tag)
        buf = _ws_scope.get(key)
        if buf is None or buf.numel() < nbytes:
            if buf is not None:
                _ws_scope.setdefault("retired", []).append(buf)     # a captured graph may still write into it
            buf = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
            _ws_scope[key] = buf
        return buf
    key = (device.index, torch.cuda.current_stream().cuda_stream, tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


_im2col_timing = None  # when a list: (start_event, end_event, algorithmic_bytes) per im2col launch (bench.py roofline)


def im2col_timing(enable):
    """bench.py: time every im2col launch of deform_conv with HIP events on the launch stream (live roofline)."""
    global _im2col_timing
    old = _im2col_timing
    _im2col_timing = [] if enable else None
    return old


_fused_dcn_timing = None  # when a list: (start_event, end_event, algorithmic bytes, algorithmic flops, MFMA products per product) per fused DCN launch


def fused_dcn_timing(enable):
    """bench.py: time every stm_deform_conv_fused_planar_f32 launch with HIP events on the launch stream (live roofline)."""
    global _fused_dcn_timing
    old = _fused_dcn_timing
    _fused_dcn_timing = [] if enable else None
    return old


_conv_timing = None  # when a list: (start_event, end_event, algorithmic_flops) per planar-conv launch (bench.py roofline)


def conv_timing(enable):
    """bench.py: time every stm_conv2d_planar_f32 launch with HIP events on the launch stream (live MFMA roofline)."""
    global _conv_timing
    old = _conv_timing
    _conv_timing = [] if enable else None
    return old


def im2col_algorithmic_bytes(g, has_mask):
    """4 * (C*Hin*Win + (3K | 2K)*dg*Ho*Wo + C*K*Ho*Wo) per image."""
    K, HWo = g.kh * g.kw, g.Ho * g.Wo
    return 4 * g.B * (g.C * g.H * g.W + (3 if has_mask else 2) * K * g.dg * HWo + g.C * K * HWo)


def deform_conv(x, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, deform_groups=1, relu=False,
                fused_om=None, mask_is_logit=False):
    """Deformable convolution forward: hand-written im2col + fp32 MFMA GEMM (+bias, +ReLU) -> [B,O,Ho,Wo]."""
    _dev(x, offset, mask, weight, bias, fused_om)
    x, weight = _f32c(x), _f32c(weight)
    O, Cw, kh, kw = weight.shape
    if Cw != x.shape[1]:
        raise StmError("groups != 1 is outside the hot path (STM_EUNSUPPORTED)")
    g = _geom(x, (kh, kw), stride, padding, dilation, deform_groups)
    off, obs, mk, mk_ptr, mbs = _offset_mask_views(offset, mask, g, fused_om)
    bias = _f32c(bias) if bias is not None else None
    y = torch.empty(g.B, O, g.Ho, g.Wo, device=x.device, dtype=torch.float32)
    need = _lib.lib().stm_deform_conv_workspace_bytes(ctypes.byref(g))
    ws = _workspace(need, x.device, "cols")
    if _im2col_timing is not None:  # same two kernels, launched separately so the im2col can be bracketed by events
        logit = 1 if (mask_is_logit or fused_om is not None) else 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call("stm_deform_im2col_f32", _p(x), _p(off), obs, c_p(mk_ptr), mbs, logit, _p(ws), ctypes.byref(g), 0, _stream())
        e1.record()
        _im2col_timing.append((e0, e1, im2col_algorithmic_bytes(g, mk_ptr != 0)))
        CK, HWo = g.C * g.kh * g.kw, g.Ho * g.Wo
        cols_bytes = (g.B * CK * HWo * 4 + 255) // 256 * 256   # same split of the workspace as stm_deform_conv_fwd_f32
        part = ws[cols_bytes:]
        call("stm_gemm_bias_ws_f32", _p(weight), _p(ws), _p(bias), _p(y), O, HWo, CK, g.B, CK * HWo, O * HWo, 1 if relu else 0, _p(part),
             part.numel(), _stream())
        return y
    call("stm_deform_conv_fwd_f32", _p(x), _p(off), obs, c_p(mk_ptr), mbs, 1 if (mask_is_logit or fused_om is not None) else 0, _p(weight),
         _p(bias), _p(y), O, 1 if relu else 0, ctypes.byref(g), _p(ws), ws.numel(), _stream())
    return y


def gemm_bias(A, Bm, bias=None, relu=False):
    """C[b] = A[M,K] @ B[b][K,N] (+bias[m]) on the fp32 MFMA pipe.  Bm is [K,N] or [batch,K,N]."""
    _dev(A, Bm, bias)
    A, Bm = _f32c(A), _f32c(Bm)
    squeeze = Bm.dim() == 2
    if squeeze:
        Bm = Bm[None]
    batch, K, N = Bm.shape
    M = A.shape[0]
    assert A.shape[1] == K
    C = torch.empty(batch, M, N, device=A.device, dtype=torch.float32)
    ws = _workspace(_lib.lib().stm_gemm_workspace_bytes(M, N, batch), A.device, "gemm")
    call("stm_gemm_bias_ws_f32", _p(A), _p(Bm), _p(_f32c(bias) if bias is not None else None), _p(C), M, N, K, batch, K * N, M * N,
         1 if relu else 0, _p(ws), ws.numel(), _stream())
    return C[0] if squeeze else C


def deform_sample_planar(x_pix, B, H, W, C, offsets, kernel_size, padding, out, out_off, fmt=0):
    """mmcv DeformConv2d's sampling half (no mask, stride 1, one deformable group) for the planar graph: x_pix fp32
    [B*H*W, ld >= C] (a channel slice of a wider pixel-major tensor: only the row stride must be a multiple of 4 floats),
    offsets fp32 [B*H*W, 2*kh*kw] pixel-major -> columns written at pixels [out_off, out_off + B*H*W) of the planes
    out [P, kh*kw*C/32, N, 32] (K index = tap*C + channel).  stm_deform_sample_planar_f32."""
    _dev(x_pix, offsets, out)
    if x_pix.dtype != torch.float32 or x_pix.dim() != 2 or x_pix.stride(1) != 1 or x_pix.shape[0] != B * H * W or x_pix.shape[1] != C:
        raise StmError(f"deform_sample_planar: x must be fp32 [B*H*W, C] with unit channel stride, got {tuple(x_pix.shape)} {x_pix.stride()}")
    offsets = _f32c(offsets)
    kh, kw = _pair(kernel_size)
    ph, pw = _pair(padding)
    if offsets.shape[0] != B * H * W or offsets.shape[1] != 2 * kh * kw:
        raise StmError(f"deform_sample_planar: offsets {tuple(offsets.shape)} != {(B * H * W, 2 * kh * kw)}")
    if out.dim() != 4 or out.shape[1] * 32 != kh * kw * C or not out.is_contiguous():
        raise StmError(f"deform_sample_planar: planes {tuple(out.shape)} do not hold {kh * kw * C} column channels")
    g = DeformGeom(B, C, H, W, kh, kw, 1, 1, ph, pw, 1, 1, 1, H, W)
    call("stm_deform_sample_planar_f32", _p(x_pix), x_pix.stride(0), _p(offsets), offsets.shape[1], 0, _p(out), out.shape[2], out_off, 0,
         ctypes.byref(g), fmt, _stream())
    return out


def fcb_ali_offsets(loc, kh, kw):
    """Featurealign.py:46-69: loc [B,4,H,W] -> offsets [B,2*kh*kw,H,W]."""
    _dev(loc)
    loc = _f32c(loc)
    B, four, H, W = loc.shape
    assert four == 4
    off = torch.empty(B, 2 * kh * kw, H, W, device=loc.device, dtype=torch.float32)
    call("stm_fcb_ali_offsets_f32", _p(loc), _p(off), B, H, W, kh, kw, _stream())
    return off


def corr_patch(f1, f2, patch_size=11, dilation_patch=1, scale=1.0, leaky_slope=1.0):
    """spatial_correlation_sample(kernel_size=1, stride=1, padding=0) -> [B,P,P,H,W] (optionally scaled + leaky)."""
    _dev(f1, f2)
    f1, f2 = _f32c(f1), _f32c(f2)
    if f1.shape != f2.shape:
        raise StmError(f"correlation inputs differ in shape: {tuple(f1.shape)} vs {tuple(f2.shape)}")
    B, C, H, W = f1.shape
    out = torch.empty(B, patch_size, patch_size, H, W, device=f1.device, dtype=torch.float32)
    call("stm_corr_patch_f32", _p(f1), _p(f2), _p(out), B, C, H, W, patch_size, dilation_patch, scale, leaky_slope, _stream())
    return out


def corr_patch_nhwc(f1, f2, patch_size=11, scale=1.0, leaky_slope=1.0, ld=None):
    """corr_patch with the displacement channels last: [B, H, W, ld] (ld >= P*P, default P*P rounded up to 8; channels past P*P are
    not written) -- the layout roi_align_planes(corr_nhwc=...) gathers from.  f1 / f2 are [B, C, H, W] tensors in either memory
    format: channels_last ones (the trunk's outputs) are read in place."""
    _dev(f1, f2)
    if f1.shape != f2.shape:
        raise StmError(f"correlation inputs differ in shape: {tuple(f1.shape)} vs {tuple(f2.shape)}")
    B, C, H, W = f1.shape
    cl = (f1.dtype == f2.dtype == torch.float32 and C > 1 and f1.is_contiguous(memory_format=torch.channels_last)
          and f2.is_contiguous(memory_format=torch.channels_last) and not f1.is_contiguous())
    if not cl:
        f1, f2 = _f32c(f1), _f32c(f2)
    ld = ld or -(-patch_size * patch_size // 8) * 8
    out = torch.empty(B, H, W, ld, device=f1.device, dtype=torch.float32)
    call("stm_corr_patch_nhwc_f32", _p(f1), _p(f2), _p(out), B, C, H, W, patch_size, 1, scale, leaky_slope, ld, 1 if cl else 0, _stream())
    return out


def roi_align(feat, rois, output_size, spatial_scale=1.0, sampling_ratio=0, aligned=True):
    _dev(feat, rois)
    feat, rois = _f32c(feat), _f32c(rois)
    ph, pw = _pair(output_size)
    B, C, H, W = feat.shape
    n = rois.shape[0]
    if n and rois.shape[1] != 5:
        raise StmError("rois must be [n,5] = (batch, x1, y1, x2, y2)")
    out = torch.empty(n, C, ph, pw, device=feat.device, dtype=torch.float32)
    call("stm_roi_align_avg_f32", _p(feat), _p(rois), _p(out), B, C, H, W, n, ph, pw, spatial_scale, sampling_ratio, 1 if aligned else 0, _stream())
    return out


def _deterministic():
    from . import autograd     # autograd imports this module
    return autograd.is_deterministic()


def _alert_not_deterministic(name):
    """What every torch operator without a deterministic implementation does under torch.use_deterministic_algorithms(True), for the two fp32
    atomic scatters: they are reached under the flag only when autograd.set_deterministic(False) switched the fixed-point kernels off, and then
    they say so the way torch's own operators do -- a RuntimeError, or a warning with warn_only=True -- instead of running unnoticed.  (torch's flag
    knows nothing of this library's kernels, and from torch 2.10 on it no longer stops such a step itself: bilinear F.interpolate runs as a
    decomposition there.)  Without torch's flag nothing is checked and nothing changes."""
    if not torch.are_deterministic_algorithms_enabled():
        return
    msg = (f"{name} does not have a deterministic implementation, but you set 'torch.use_deterministic_algorithms(True)' and switched its "
           "deterministic replacement off with stmask_amd.autograd.set_deterministic(False).  Leave the mode at None (or True) to take the "
           "fixed-point kernel, or pass warn_only=True to torch.use_deterministic_algorithms to run the atomic one with a warning.")
    if torch.is_deterministic_algorithms_warn_only_enabled():
        warnings.warn(msg)
    else:
        raise RuntimeError(msg)


def _det_workspace(out):
    """The int64 accumulator of a deterministic scatter into `out` and its two words of state (csrc/det_backward.h), as a tensor: the caching
    allocator hands it back to the next layer's backward.  The library clears it."""
    return torch.empty(out.numel() + 1, device=out.device, dtype=torch.int64)


def upsample_bilinear_backward(grad_out, in_shape, scale_factor=None):
    """grad of F.interpolate(x [B,C,h,w], size= or scale_factor=, mode="bilinear", align_corners=False) w.r.t. x from grad_out [B,C,H,W]: a gather
    in a fixed order (csrc/det_backward.hip).  scale_factor: what the forward was given (a number, a pair or None for the size= form)."""
    _dev(grad_out)
    go = _f32c(grad_out)
    B, C, h, w = in_shape
    if go.dim() != 4 or tuple(go.shape[:2]) != (B, C):
        raise StmError(f"upsample_bilinear_backward: grad_out {tuple(go.shape)} does not belong to an input {tuple(in_shape)}")
    if scale_factor is None:
        sf_h = sf_w = 0.0       # the library takes in / out
    elif isinstance(scale_factor, (int, float)):
        sf_h = sf_w = float(scale_factor)
    else:
        sf_h, sf_w = (float(v) for v in scale_factor)
    gin = torch.empty(B, C, h, w, device=go.device, dtype=torch.float32)
    _lib.private_call("stm_upsample_bilinear_backward_f32", _p(go), _p(gin), B * C, h, w, go.shape[2], go.shape[3], sf_h, sf_w, _stream())
    return gin


def deform_col2im(grad_cols, offset, mask, g, fused_om=None):
    """grad_x [B,C,H,W] of deform_im2col from the column gradient grad_cols [B, C*kh*kw, Ho*Wo]: an fp32 atomic scatter, or under
    autograd.is_deterministic() the same terms summed in 64-bit fixed point (csrc/det_backward.hip; the workspace is 8 bytes per element of grad_x)."""
    _dev(grad_cols, offset, mask, fused_om)
    grad_cols = _f32c(grad_cols)
    off, obs, _, mk_ptr, mbs = _offset_mask_views(offset, mask, g, fused_om)
    if _deterministic():
        gx = torch.empty(g.B, g.C, g.H, g.W, device=grad_cols.device, dtype=torch.float32)
        ws = _det_workspace(gx)
        _lib.private_call("stm_deform_col2im_det_f32", _p(grad_cols), _p(off), obs, c_p(mk_ptr), mbs, 1 if fused_om is not None else 0, _p(gx),
                          ctypes.byref(g), _p(ws), 8 * ws.numel(), _stream())
        return gx
    _alert_not_deterministic("stm_deform_col2im_f32")
    gx = torch.zeros(g.B, g.C, g.H, g.W, device=grad_cols.device, dtype=torch.float32)
    call("stm_deform_col2im_f32", _p(grad_cols), _p(off), obs, c_p(mk_ptr), mbs, 1 if fused_om is not None else 0, _p(gx), ctypes.byref(g), _stream())
    return gx


def deform_col2im_coord(grad_cols, x, offset, mask, g, fused_om=None, want_offset=True, want_mask=True):
    """(grad_offset, grad_mask) of deform_im2col (deterministic).  With fused_om: one tensor shaped like it, the offset channels followed
    by the gradient w.r.t. the mask LOGITS (channels a part that was not asked for stay 0)."""
    _dev(grad_cols, x, offset, mask, fused_om)
    grad_cols, x = _f32c(grad_cols), _f32c(x)
    off, obs, _, mk_ptr, mbs = _offset_mask_views(offset, mask, g, fused_om)
    K, HWo = g.kh * g.kw, g.Ho * g.Wo
    if fused_om is not None:
        gom = torch.zeros_like(off) if not (want_offset and want_mask) else torch.empty_like(off)
        bs = g.dg * 3 * K * HWo
        call("stm_deform_col2im_coord_f32", _p(grad_cols), _p(x), _p(off), obs, c_p(mk_ptr), mbs, 1, _p(gom) if want_offset else c_p(0), bs,
             c_p(gom.data_ptr() + 4 * g.dg * 2 * K * HWo) if want_mask else c_p(0), bs, ctypes.byref(g), _stream())
        return gom
    goff = torch.empty(g.B, g.dg * 2 * K, g.Ho, g.Wo, device=x.device, dtype=torch.float32) if want_offset else None
    gmask = torch.empty(g.B, g.dg * K, g.Ho, g.Wo, device=x.device, dtype=torch.float32) if (want_mask and mk_ptr) else None
    if goff is None and gmask is None:
        return None, None
    call("stm_deform_col2im_coord_f32", _p(grad_cols), _p(x), _p(off), obs, c_p(mk_ptr), mbs, 0, _p(goff), g.dg * 2 * K * HWo, _p(gmask),
         g.dg * K * HWo, ctypes.byref(g), _stream())
    return goff, gmask


def deform_conv_backward(grad_out, x, offset, mask, weight, stride=1, padding=0, dilation=1, deform_groups=1, fused_om=None,
                         need=(True, True, True, True, True)):
    """Gradients of deform_conv (relu=False) -> (grad_x, grad_offset, grad_mask, grad_weight, grad_bias); need[i] False -> None, nothing
    launched for it.  With fused_om, grad_offset is the gradient w.r.t. the whole raw conv_offset_mask output and grad_mask is None.
    The columns are recomputed with the forward's im2col; the two dense products run on the library's fp32 GEMM (fixed order):
    grad_cols = W^T grad_out, grad_weight = sum_b grad_out_b cols_b^T; grad_bias is torch's sum of grad_out."""
    need_x, need_off, need_mask, need_w, need_b = need
    _dev(grad_out, x, offset, mask, weight, fused_om)
    x, weight = _f32c(x), _f32c(weight)
    go = _f32c(grad_out)
    O, C, kh, kw = weight.shape
    g = _geom(x, (kh, kw), stride, padding, dilation, deform_groups)
    CK, HWo = C * kh * kw, g.Ho * g.Wo
    if tuple(go.shape) != (g.B, O, g.Ho, g.Wo):
        raise StmError(f"deform_conv_backward: grad_out {tuple(go.shape)} != {(g.B, O, g.Ho, g.Wo)}")
    gx = goff = gmask = gw = gb = None
    if need_b:
        gb = go.sum((0, 2, 3))
    if need_w:
        cols = deform_im2col(x, offset, mask, (kh, kw), stride, padding, dilation, deform_groups, fused_om=fused_om)
        # grad_weight^T [CK, O] = cols [CK, B*HWo] . grad_out^T [B*HWo, O]
        a = cols[0] if g.B == 1 else cols.permute(1, 0, 2).reshape(CK, g.B * HWo)
        bm = go.view(g.B, O, HWo).permute(0, 2, 1).reshape(g.B * HWo, O)
        gw = gemm_bias(a.contiguous(), bm.contiguous()).t().reshape(O, C, kh, kw).contiguous()
        del cols, a
    if need_x or need_off or need_mask:
        gcols = gemm_bias(weight.view(O, CK).t().contiguous(), go.view(g.B, O, HWo))        # [B, CK, HWo]
        if need_x:
            gx = deform_col2im(gcols, offset, mask, g, fused_om)
        if need_off or (need_mask and (mask is not None or fused_om is not None)):
            if fused_om is not None:
                goff = deform_col2im_coord(gcols, x, None, None, g, fused_om, want_offset=need_off, want_mask=need_mask)
            else:
                goff, gmask = deform_col2im_coord(gcols, x, offset, mask, g, None, want_offset=need_off, want_mask=need_mask)
    return gx, goff, gmask, gw, gb


def roi_align_backward(grad_out, rois, feat_shape, output_size, spatial_scale=1.0, sampling_ratio=0, aligned=True):
    """grad_feat of roi_align: an fp32 atomic scatter, or under autograd.is_deterministic() the same terms summed in 64-bit fixed point
    (csrc/det_backward.hip); no gradient w.r.t. rois."""
    _dev(grad_out, rois)
    go, rois = _f32c(grad_out), _f32c(rois)
    ph, pw = _pair(output_size)
    B, C, H, W = feat_shape
    n = rois.shape[0]
    if tuple(go.shape) != (n, C, ph, pw):
        raise StmError(f"roi_align_backward: grad_out {tuple(go.shape)} != {(n, C, ph, pw)}")
    if _deterministic():
        gfeat = torch.empty(B, C, H, W, device=go.device, dtype=torch.float32)
        ws = _det_workspace(gfeat)
        _lib.private_call("stm_roi_align_backward_det_f32", _p(go), _p(rois), _p(gfeat), B, C, H, W, n, ph, pw, spatial_scale, sampling_ratio,
                          1 if aligned else 0, _p(ws), 8 * ws.numel(), _stream())
        return gfeat
    _alert_not_deterministic("stm_roi_align_backward_f32")
    gfeat = torch.zeros(B, C, H, W, device=go.device, dtype=torch.float32)
    call("stm_roi_align_backward_f32", _p(go), _p(rois), _p(gfeat), B, C, H, W, n, ph, pw, spatial_scale, sampling_ratio, 1 if aligned else 0,
         _stream())
    return gfeat


def corr_patch_backward(grad_out, f1, f2, dilation_patch=1, need1=True, need2=True):
    """(grad_f1, grad_f2) of corr_patch(scale=1, leaky_slope=1); a gradient not needed is None and not computed."""
    _dev(grad_out, f1, f2)
    go, f1, f2 = _f32c(grad_out), _f32c(f1), _f32c(f2)
    B, C, H, W = f1.shape
    P = go.shape[1]
    if tuple(go.shape) != (B, P, P, H, W) or f2.shape != f1.shape:
        raise StmError(f"corr_patch_backward: grad_out {tuple(go.shape)} does not match inputs {tuple(f1.shape)}")
    g1 = torch.empty_like(f1) if need1 else None
    g2 = torch.empty_like(f2) if need2 else None
    if g1 is None and g2 is None:
        return None, None
    call("stm_corr_backward_f32", _p(go), _p(f1), _p(f2), _p(g1), _p(g2), B, C, H, W, P, dilation_patch, _stream())
    return g1, g2


def t2s_check_shapes(who, fpn, t2s, patch_size):
    """What include/stmask_hip_t2s_feat.h refuses, and what its contiguous fp32 layout asks of the tensors, raised from the shapes before anything
    touches the device.  Returns (bs, C, Cu, H, W)."""
    if fpn.dim() != 4 or t2s.dim() != 4:
        raise StmError(f"{who}: fpn {tuple(fpn.shape)} and t2s {tuple(t2s.shape)} must be [2 bs, C, h, w] and [2 bs, Cu, h, w]")
    n, C, H, W = fpn.shape
    if n < 2 or n % 2:
        raise StmError(f"{who}: {n} images; the two frames of every clip are expected (an even count)")
    if t2s.shape[0] != n or tuple(t2s.shape[2:]) != (H, W):
        raise StmError(f"{who}: t2s {tuple(t2s.shape)} does not fit fpn {tuple(fpn.shape)}")
    if fpn.dtype != torch.float32 or t2s.dtype != torch.float32:
        raise StmError(f"{who}: expected float32, got {fpn.dtype} and {t2s.dtype}")
    if fpn.device != t2s.device:
        raise StmError(f"{who}: fpn on {fpn.device}, t2s on {t2s.device}")
    P, Cu = int(patch_size), t2s.shape[1]
    if P < 1 or P % 2 == 0:
        raise StmError(f"{who}: patch size {patch_size} must be odd and positive")
    if min(C, Cu, H, W) < 1:
        raise StmError(f"{who}: empty maps {tuple(fpn.shape)} / {tuple(t2s.shape)}")
    if not fpn.is_contiguous() or not t2s.is_contiguous():
        raise StmError(f"{who}: fpn and t2s must be contiguous (the halves are read in place through the batch stride)")
    if max(P * P, C, Cu) * H * W >= 1 << 31:
        raise StmError(f"{who}: P*P*h*w, C*h*w and Cu*h*w must stay below 2^31")
    return n // 2, C, Cu, H, W


def t2s_concat_feat(fpn, t2s, patch_size=11):
    """T2S_concat_feat of STMask.py:291-296 in two launches (stm_t2s_feat_forward_f32): fpn [2 bs, C, h, w], t2s [2 bs, Cu, h, w], the reference frame
    of clip b at image 2 b, the next frame at 2 b + 1 -> [bs, P*P + 2 Cu, h, w].  No workspace, no host synchronisation."""
    bs, C, Cu, H, W = t2s_check_shapes("t2s_concat_feat", fpn, t2s, patch_size)
    _dev(fpn, t2s)
    out = torch.empty(bs, patch_size * patch_size + 2 * Cu, H, W, device=fpn.device, dtype=torch.float32)
    call("stm_t2s_feat_forward_f32", _p(fpn), _p(t2s), _p(out), bs, C, Cu, H, W, int(patch_size), _stream())
    return out


def t2s_concat_feat_backward(grad_out, out, fpn, t2s, patch_size=11, need_fpn=True, need_t2s=True):
    """(grad_fpn, grad_t2s) of t2s_concat_feat from grad_out and the saved inputs and output (stm_t2s_feat_backward_f32: two launches for grad_fpn,
    one for grad_t2s); a gradient not needed is None and not computed."""
    bs, C, Cu, H, W = t2s_check_shapes("t2s_concat_feat_backward", fpn, t2s, patch_size)
    _dev(grad_out, out, fpn, t2s)
    go = _f32c(grad_out)
    if tuple(go.shape) != (bs, patch_size * patch_size + 2 * Cu, H, W) or out.shape != go.shape or out.dtype != torch.float32 or \
            not out.is_contiguous():
        raise StmError(f"t2s_concat_feat_backward: grad_out {tuple(go.shape)} / out {tuple(out.shape)} do not match the inputs")
    if not (need_fpn or need_t2s):
        return None, None
    g_fpn = torch.empty_like(fpn) if need_fpn else None
    g_t2s = torch.empty_like(t2s) if need_t2s else None
    call("stm_t2s_feat_backward_f32", _p(go), _p(out), _p(fpn), _p(t2s), _p(g_fpn), _p(g_t2s), bs, C, Cu, H, W, int(patch_size), _stream())
    return g_fpn, g_t2s


def decode(loc, priors):
    """box_utils.py:238-283, bit-exact vs the oracle."""
    _dev(loc, priors)
    loc, priors = _f32c(loc), _f32c(priors)
    boxes = torch.empty_like(loc)
    call("stm_decode_boxes_f32", _p(loc), _p(priors), _p(boxes), loc.shape[0], _stream())
    return boxes


def decode_backward(grad_boxes, loc, priors, need_loc=True, need_priors=False):
    """(grad_loc, grad_priors) of decode; a gradient not needed is None and not computed."""
    _dev(grad_boxes, loc, priors)
    gb, loc, priors = _f32c(grad_boxes), _f32c(loc), _f32c(priors)
    if gb.shape != loc.shape or priors.shape != loc.shape:
        raise StmError(f"decode_backward: grad_boxes {tuple(gb.shape)}, loc {tuple(loc.shape)} and priors {tuple(priors.shape)} differ")
    gl = torch.empty_like(loc) if need_loc else None
    gp = torch.empty_like(priors) if need_priors else None
    if gl is None and gp is None:
        return None, None
    call("stm_decode_boxes_backward_f32", _p(gb), _p(loc), _p(priors), _p(gl), _p(gp), loc.shape[0], _stream())
    return gl, gp


def generate_candidates(loc, priors, conf, thresh=0.05):
    """TF_utils.py:54-82 core.  loc [B,N,4], priors [N,4], conf [B,N,ncls] soft-maxed ->
    keep_idx [B,N] (first count[b] valid, ascending), cand_box [B,N,4], count [B] (device int32)."""
    _dev(loc, priors, conf)
    loc, priors, conf = _f32c(loc), _f32c(priors), _f32c(conf)
    B, N, ncls = conf.shape
    keep_idx = torch.empty(B, N, dtype=torch.int64, device=conf.device)
    cand_box = torch.empty(B, N, 4, dtype=torch.float32, device=conf.device)
    count = torch.empty(B, dtype=torch.int32, device=conf.device)
    call("stm_generate_candidates_f32", _p(loc), _p(priors), _p(conf), N, ncls, thresh, B, _p(keep_idx), _p(cand_box), _p(count), _stream())
    return keep_idx, cand_box, count


NMS_LDS_KEYS = 16384   # keys the one-workgroup Fast NMS sorts in LDS (csrc/postproc.hip NMS_MAX_KEYS)


def cc_fast_nms(conf, boxes, centerness, iou_thr=0.5, top_k=200, k_dev=None):
    """detection_TF.py:85-134 on candidate rows.  conf [K,ncls] or [B,K,ncls].  Returns padded
    (idx [B,top_k] int64, cls, score, box [B,top_k,4], count [B] int32) -- all on device, no sync."""
    _dev(conf, boxes, centerness)
    conf, boxes = _f32c(conf), _f32c(boxes)
    squeeze = conf.dim() == 2
    if squeeze:
        conf, boxes = conf[None], boxes[None]
        centerness = centerness[None] if centerness is not None else None
    B, K, ncls = conf.shape
    cen = _f32c(centerness) if centerness is not None else None
    dev = conf.device
    idx = torch.empty(B, top_k, dtype=torch.int64, device=dev)
    cls = torch.empty(B, top_k, dtype=torch.int64, device=dev)
    sc = torch.empty(B, top_k, dtype=torch.float32, device=dev)
    bx = torch.empty(B, top_k, 4, dtype=torch.float32, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    if K > NMS_LDS_KEYS and k_dev is None:
        # more candidate rows than the one-workgroup LDS sort holds: scores to a workspace, exact top-k select in the kernel
        ws = _workspace(_lib.lib().stm_cc_fast_nms_workspace_bytes(K, B), dev, "ccnms")
        call("stm_cc_fast_nms_ws_f32", _p(conf), _p(boxes), _p(cen), K, ncls, iou_thr, top_k, B, _p(idx), _p(cls), _p(sc), _p(bx), _p(cnt), _p(ws),
             ws.numel(), _stream())
    else:
        call("stm_cc_fast_nms_f32", _p(conf), _p(boxes), _p(cen), K, ncls, _p(k_dev), iou_thr, top_k, B, _p(idx), _p(cls), _p(sc), _p(bx), _p(cnt),
             _stream())
    if squeeze:
        return idx[0], cls[0], sc[0], bx[0], cnt[0]
    return idx, cls, sc, bx, cnt


def detect_cc(loc, priors, conf, centerness, conf_thresh=0.05, iou_thr=0.5, top_k=200, logits=False):
    """Fused generate_candidate + cc_fast_nms (STMask.py:317-320) with no host sync.
    loc [B,N,4], priors [N,4], conf [B,N,ncls] soft-maxed (logits=True: the raw class logits, soft-maxed per row inside the kernel:
    stm_detect_cc_logits_f32), centerness [B,N] or [B,N,1] -> (prior_idx [B,top_k], cls, score, box [B,top_k,4], count [B])."""
    _dev(loc, priors, conf, centerness)
    loc, priors, conf = _f32c(loc), _f32c(priors), _f32c(conf)
    B, N, ncls = conf.shape
    cen = _f32c(centerness.reshape(B, N)) if centerness is not None else None
    dev = conf.device
    idx = torch.empty(B, top_k, dtype=torch.int64, device=dev)
    cls = torch.empty(B, top_k, dtype=torch.int64, device=dev)
    sc = torch.empty(B, top_k, dtype=torch.float32, device=dev)
    bx = torch.empty(B, top_k, 4, dtype=torch.float32, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    need = _lib.lib().stm_detect_cc_workspace_bytes(N, B)
    ws = _workspace(need, dev, "detect")
    call("stm_detect_cc_logits_f32" if logits else "stm_detect_cc_f32", _p(loc), _p(priors), _p(conf), _p(cen), N, ncls, conf_thresh, iou_thr,
         top_k, B, _p(idx), _p(cls), _p(sc), _p(bx), _p(cnt), _p(ws), ws.numel(), _stream())
    return idx, cls, sc, bx, cnt


def fast_nms(conf, boxes, centerness, iou_thr=0.5, top_k=200, conf_thresh=0.05, max_det=100, k_dev=None):
    """detection_TF.py:136-204 (per-class).  Returns padded (idx, cls, score, box, count)."""
    _dev(conf, boxes, centerness)
    conf, boxes = _f32c(conf), _f32c(boxes)
    K, ncls = conf.shape
    cen = _f32c(centerness) if centerness is not None else None
    dev = conf.device
    idx = torch.empty(max_det, dtype=torch.int64, device=dev)
    cls = torch.empty(max_det, dtype=torch.int64, device=dev)
    sc = torch.empty(max_det, dtype=torch.float32, device=dev)
    bx = torch.empty(max_det, 4, dtype=torch.float32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    need = _lib.lib().stm_fast_nms_workspace_bytes(K, ncls, top_k)
    ws = _workspace(need, dev, "pcnms")
    call("stm_fast_nms_f32", _p(conf), _p(boxes), _p(cen), K, ncls, _p(k_dev), iou_thr, top_k, conf_thresh, max_det, _p(idx), _p(cls), _p(sc), _p(bx),
         _p(cnt), _p(ws), ws.numel(), _stream())
    return idx, cls, sc, bx, cnt[0]


def detect_pc(loc, priors, conf, centerness, conf_thresh=0.05, iou_thr=0.5, top_k=200, max_det=100):
    """generate_candidate + per-class Fast NMS (detection_TF.py:136-204) for a whole frame batch with no host sync: the candidate pass
    (stm_generate_candidates_f32) leaves keep lists, compacted boxes and counts on the device, and ONE launch pair of stm_fast_nms_batched_f32 runs
    every frame's 40 class sorts through the keep lists.  loc [B,N,4], priors [N,4], conf [B,N,ncls] SOFT-MAXED, centerness [B,N] or [B,N,1] ->
    (prior_idx [B,max_det], cls, score, box [B,max_det,4], count [B]), the layout detect_cc returns."""
    _dev(loc, priors, conf, centerness)
    loc, priors, conf = _f32c(loc), _f32c(priors), _f32c(conf)
    B, N, ncls = conf.shape
    cen = _f32c(centerness.reshape(B, N)) if centerness is not None else None
    dev = conf.device
    if N > NMS_LDS_KEYS:
        raise StmError(f"detect_pc: {N} priors exceed the {NMS_LDS_KEYS} keys of the per-class LDS sort (use the per-frame layer API)")
    keep_idx, cand_box, count = generate_candidates(loc, priors, conf, conf_thresh)
    idx = torch.empty(B, max_det, dtype=torch.int64, device=dev)
    cls = torch.empty(B, max_det, dtype=torch.int64, device=dev)
    sc = torch.empty(B, max_det, dtype=torch.float32, device=dev)
    bx = torch.empty(B, max_det, 4, dtype=torch.float32, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    ws = _workspace(_lib.lib().stm_fast_nms_batched_workspace_bytes(N, ncls, top_k, B), dev, "pcnms_b")
    call("stm_fast_nms_batched_f32", _p(conf), N * ncls, _p(keep_idx), _p(cand_box), _p(cen), N, N, ncls, _p(count), iou_thr, top_k, conf_thresh,
         max_det, B, _p(idx), _p(cls), _p(sc), _p(bx), _p(cnt), _p(ws), ws.numel(), _stream())
    return idx, cls, sc, bx, cnt


def encode(matched, priors):
    """box_utils.py:200-235 (use_yolo_regressors=False): matched [n,4] point form, priors [n,4] centre-size -> [n,4].  Columns 0-1 are the
    reference's fp32 arithmetic bit for bit; the log of columns 2-3 is evaluated in double and rounded once."""
    _dev(matched, priors)
    matched, priors = _f32c(matched), _f32c(priors)
    if matched.dim() != 2 or matched.shape[1] != 4 or priors.shape != matched.shape:
        raise StmError(f"encode: matched {tuple(matched.shape)} and priors {tuple(priors.shape)} must both be [n, 4]")
    out = torch.empty_like(matched)
    call("stm_encode_boxes_f32", _p(matched), _p(priors), _p(out), matched.shape[0], _stream())
    return out


_match_offsets = {}   # (device index, G) -> int32 [0, G] on the device, for the one-image form (G <= 128: bounded)


def match_offsets(counts, device):
    """Per-image box counts (Python ints) -> the int32 [B+1] row offsets on the device, without a host synchronisation: the one-image form is
    cached, a batch goes through pinned memory and an asynchronous copy."""
    if len(counts) == 1:
        key = (device.index, counts[0])
        t = _match_offsets.get(key)
        if t is None:
            t = _match_offsets[key] = torch.tensor([0, counts[0]], dtype=torch.int32, device=device)
        return t
    acc = [0]
    for c in counts:
        acc.append(acc[-1] + int(c))
    return torch.tensor(acc, dtype=torch.int32).pin_memory().to(device, non_blocking=True)


def match_priors(boxes, labels, ids, counts, priors, conf, pos_thresh, neg_thresh, out=None, offsets=None, want_status=False):
    """box_utils.py:119-197 for a whole batch in three launches (stm_match_priors_f32; conventions in include/stmask_hip.h and INTEGRATION.md
    section 14).  boxes [G_total,4] fp32 point form, labels / ids [G_total] int64, counts: the per-image numbers of boxes (Python ints, from the
    callers' tensor shapes), priors [P,4] or [B,P,4], conf [B,P,C] (read detached).  out: optional (loc_t, gt_boxes_t, conf_t, idx_t, ids_t) to
    fill -- contiguous fp32 [B,P,4] x 2 and int64 [B,P] x 3.  Returns that tuple, plus the device int32 [B] status word with want_status."""
    _dev(boxes, labels, ids, priors, conf)
    counts = [int(c) for c in counts]
    B, G_total, G_max = len(counts), sum(counts), max(counts) if counts else 0
    conf = conf.detach()
    boxes, priors, conf = _f32c(boxes), _f32c(priors), _f32c(conf)
    if conf.dim() == 2:
        conf = conf[None]
    if conf.dim() != 3 or conf.shape[0] != B:
        raise StmError(f"match_priors: conf {tuple(conf.shape)} for {B} images (expected [B, P, C])")
    P, C = conf.shape[1], conf.shape[2]
    if tuple(boxes.shape) != (G_total, 4) or labels.shape[0] != G_total or ids.shape[0] != G_total:
        raise StmError(f"match_priors: boxes {tuple(boxes.shape)}, labels {tuple(labels.shape)}, ids {tuple(ids.shape)} for {G_total} boxes")
    if tuple(priors.shape) not in ((P, 4), (B, P, 4)):
        raise StmError(f"match_priors: priors {tuple(priors.shape)} for P={P}, B={B}")
    labels, ids = labels.to(torch.int64).contiguous(), ids.to(torch.int64).contiguous()
    dev = conf.device
    if offsets is None:
        offsets = match_offsets(counts, dev)
    if out is None:
        out = (torch.empty(B, P, 4, dtype=torch.float32, device=dev), torch.empty(B, P, 4, dtype=torch.float32, device=dev),
               torch.empty(B, P, dtype=torch.int64, device=dev), torch.empty(B, P, dtype=torch.int64, device=dev),
               torch.empty(B, P, dtype=torch.int64, device=dev))
    else:
        for t, dt, shp in zip(out, (torch.float32,) * 2 + (torch.int64,) * 3, ((B, P, 4),) * 2 + ((B, P),) * 3):
            if t.dtype != dt or t.numel() != B * P * (4 if len(shp) == 3 else 1) or not t.is_contiguous() or t.device != dev:
                raise StmError(f"match_priors: output {tuple(t.shape)} {t.dtype} must be contiguous {dt} with the elements of {shp}")
    status = torch.empty(B, dtype=torch.int32, device=dev) if want_status else None
    nbytes = _lib.lib().stm_match_workspace_bytes(B, P, G_total, G_max)
    ws = _workspace(nbytes, dev, "match")
    call("stm_match_priors_f32", _p(boxes), _p(labels), _p(ids), _p(offsets), B, G_total, G_max, _p(priors), 1 if priors.dim() == 3 else 0, P,
         _p(conf), C, float(pos_thresh), float(neg_thresh), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _p(out[4]), _p(status), _p(ws), nbytes,
         _stream())
    return tuple(out) + ((status,) if want_status else ())


def jaccard(a, b):
    """box_utils.py:60-88 (2-D form), bit-exact."""
    _dev(a, b)
    a, b = _f32c(a), _f32c(b)
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
    call("stm_jaccard_f32", _p(a), a.shape[0], _p(b), b.shape[0], _p(out), _stream())
    return out


def jaccard_backward(grad_out, a, b, need_a=True, need_b=True):
    """(grad_a, grad_b) of jaccard (2-D form); fixed-order sums, no atomics.  Ties: INTEGRATION.md section 14."""
    _dev(grad_out, a, b)
    go, a, b = _f32c(grad_out), _f32c(a), _f32c(b)
    if tuple(go.shape) != (a.shape[0], b.shape[0]):
        raise StmError(f"jaccard_backward: grad_out {tuple(go.shape)} != {(a.shape[0], b.shape[0])}")
    ga = torch.empty_like(a) if need_a else None
    gb = torch.empty_like(b) if need_b else None
    if ga is None and gb is None:
        return None, None
    call("stm_jaccard_backward_f32", _p(go), _p(a), a.shape[0], _p(b), b.shape[0], _p(ga), _p(gb), _stream())
    return ga, gb


def lincomb_sigmoid_crop_bits(proto, coeff, boxes, row_proto, thr=0.5, apply_tanh=True):
    """lincomb_sigmoid_crop that also returns the binarised masks (value > thr) bit-packed, [n, ceil(h*w/64)] int64 words -- the
    form mask_iou_bits consumes, produced in the pass that writes the soft masks instead of a second read of them."""
    _dev(proto, coeff, boxes, row_proto)
    proto, coeff = _f32c(proto), _f32c(coeff)
    assert proto.dim() == 4 and row_proto.dtype == torch.int32 and row_proto.numel() == coeff.shape[0]
    h, w, m = proto.shape[1:]
    n = coeff.shape[0]
    out = torch.empty(n, h, w, dtype=torch.float32, device=proto.device)
    bits = torch.empty(n, (h * w + 63) // 64, dtype=torch.int64, device=proto.device)
    call("stm_lincomb_sigmoid_crop_bits_f32", _p(proto), _p(coeff), _p(_f32c(boxes)), _p(out), h, w, m, n, 1 if apply_tanh else 0, c_p(0),
         _p(row_proto), _p(bits), thr, _stream())
    return out, bits


def mask_iou_bits(bits1, bits2, hw, group1=None, group2=None):
    """box_utils.py:435-447 on bit-packed binary masks (lincomb_sigmoid_crop_bits) -> [n1, n2]; groups as in mask_iou."""
    _dev(bits1, bits2, group1, group2)
    n1, n2 = bits1.shape[0], bits2.shape[0]
    if n1 == 0 or n2 == 0:
        return torch.zeros(n1, n2, dtype=torch.float32, device=bits1.device)
    out = torch.empty(n1, n2, dtype=torch.float32, device=bits1.device)     # (the kernel writes every element: zeros for pairs of different groups)
    if bits1.dtype != torch.int64 or bits2.dtype != torch.int64 or bits1.shape[1] != (hw + 63) // 64 or bits2.shape[1] != bits1.shape[1]:
        raise StmError("mask_iou_bits: bit tables must be int64 [n, ceil(hw / 64)]")
    call("stm_mask_iou_bits_f32", _p(bits1.contiguous()), n1, _p(bits2.contiguous()), n2, hw, _p(out),
         _p(group1.contiguous()) if group1 is not None else c_p(0), _p(group2.contiguous()) if group2 is not None else c_p(0), _stream())
    return out


def lincomb_sigmoid_crop(proto, coeff, boxes=None, apply_tanh=True, n_dev=None, row_proto=None):
    """generate_mask (mask_utils.py:111-128) + crop.  proto [h,w,m], coeff [n,m], boxes [n,4] -> [n,h,w].
    With row_proto (int32 [n]) proto is [P,h,w,m] and row i uses proto[row_proto[i]] (rows of many clips, one launch)."""
    _dev(proto, coeff, boxes, row_proto)
    proto, coeff = _f32c(proto), _f32c(coeff)
    if row_proto is not None:
        assert proto.dim() == 4 and row_proto.dtype == torch.int32 and row_proto.numel() == coeff.shape[0]
        h, w, m = proto.shape[1:]
    else:
        h, w, m = proto.shape
    n = coeff.shape[0]
    bx = _f32c(boxes) if boxes is not None else None
    out = torch.empty(n, h, w, dtype=torch.float32, device=proto.device)
    call("stm_lincomb_sigmoid_crop_f32", _p(proto), _p(coeff), _p(bx), _p(out), h, w, m, n, 1 if apply_tanh else 0, _p(n_dev), _p(row_proto),
         _stream())
    return out


def lincomb_sigmoid_crop_backward(grad_out, proto, coeff, boxes=None, apply_tanh=True, need_proto=True, need_coeff=True):
    """(grad_proto, grad_coeff) of lincomb_sigmoid_crop(proto [h,w,m], coeff [n,m], boxes [n,4] or None); only the inputs are read (the
    sigmoid is recomputed), both sums run in a fixed order.  A gradient not needed is None and not computed; none w.r.t. the boxes."""
    _dev(grad_out, proto, coeff, boxes)
    go, proto, coeff = _f32c(grad_out), _f32c(proto), _f32c(coeff)
    h, w, m = proto.shape
    n = coeff.shape[0]
    if tuple(go.shape) != (n, h, w) or coeff.shape[1] != m or (boxes is not None and tuple(boxes.shape) != (n, 4)):
        raise StmError(f"lincomb_sigmoid_crop_backward: grad_out {tuple(go.shape)}, proto {tuple(proto.shape)}, coeff {tuple(coeff.shape)} do not match")
    gp = torch.empty_like(proto) if need_proto else None
    gc = torch.empty_like(coeff) if need_coeff else None
    if gp is None and gc is None:
        return None, None
    bx = _f32c(boxes) if boxes is not None else None
    need = _lib.lib().stm_lincomb_backward_workspace_bytes(n, h, w, m)
    ws = _workspace(need, proto.device, "lcb")
    call("stm_lincomb_backward_f32", _p(go), _p(proto), _p(coeff), _p(bx), _p(gp), _p(gc), h, w, m, n, 1 if apply_tanh else 0, _p(ws), ws.numel(),
         _stream())
    return gp, gc


def _mask_bce_args(who, pred, target, idx, grad_loss=None):
    """Shapes and dtypes of the mask loss tail, checked before anything touches the device: (pred, target as bytes or fp32, idx, is_f32)."""
    if pred.dtype != torch.float32 or pred.dim() != 3:
        raise StmError(f"{who}: pred must be float32 [n,h,w], got {pred.dtype} {tuple(pred.shape)}")
    if target.dtype not in (torch.uint8, torch.bool, torch.float32) or target.dim() != 3:
        raise StmError(f"{who}: target must be uint8, bool or float32 [G,H,W], got {target.dtype} {tuple(target.shape)}")
    n, h, w = pred.shape
    G, H, W = target.shape
    if h > H or w > W:
        raise StmError(f"{who}: pred {h}x{w} is larger than the target {H}x{W} (downsampling is not supported)")
    if idx is None:
        if G != n:
            raise StmError(f"{who}: without idx row i uses target i, but pred has {n} rows and target {G}")
    elif idx.dtype != torch.int64 or idx.dim() != 1 or idx.numel() != n:
        raise StmError(f"{who}: idx must be int64 [{n}], got {idx.dtype} {tuple(idx.shape)}")
    if grad_loss is not None and (grad_loss.dtype != torch.float32 or tuple(grad_loss.shape) != (n,)):
        raise StmError(f"{who}: grad_loss must be float32 [{n}], got {grad_loss.dtype} {tuple(grad_loss.shape)}")
    _dev(pred, target, idx, grad_loss)
    target = target if target.is_contiguous() else target.contiguous()
    if target.dtype == torch.bool:
        target = target.view(torch.uint8)
    return _f32c(pred), target, (idx if idx is None or idx.is_contiguous() else idx.contiguous()), target.dtype == torch.float32


def mask_bce_upsampled(pred, target, idx=None):
    """The tail of lincomb_mask_loss (multibox_loss.py:575, :598-603, the sum of :613): pred [n,h,w] soft masks, target [G,H,W] uint8 / bool / float32,
    idx [n] int64 (the target row of each instance; None: row i uses target i) -> loss [n], the per-instance sum over all H * W pixels of the BCE
    between the target and the bilinearly upsampled (align_corners=False), clamped prediction.  Nothing at target resolution is materialised."""
    pred, target, idx, is_f32 = _mask_bce_args("mask_bce_upsampled", pred, target, idx)
    n, h, w = pred.shape
    G, H, W = target.shape
    loss = torch.empty(n, dtype=torch.float32, device=pred.device)
    if n == 0:
        return loss
    need = _lib.lib().stm_mask_bce_workspace_bytes(n, H, W)
    ws = _workspace(need, pred.device, "mbce")
    call("stm_mask_bce_upsampled_f32", _p(pred), _p(target), 1 if is_f32 else 0, _p(idx), _p(loss), n, h, w, G, H, W, _p(ws), ws.numel(), _stream())
    return loss


def mask_bce_upsampled_backward(grad_loss, pred, target, idx=None):
    """grad_pred [n,h,w] of mask_bce_upsampled: grad_loss [n] times the gather of weight * (pc - t) / max(pc (1 - pc), 1e-12) over the target pixels
    that sample each prediction pixel (0 where the upsampled value left [0, 1]); fixed-order sums, no atomics."""
    pred, target, idx, is_f32 = _mask_bce_args("mask_bce_upsampled_backward", pred, target, idx, grad_loss)
    n, h, w = pred.shape
    G, H, W = target.shape
    grad_pred = torch.empty_like(pred)
    if n == 0:
        return grad_pred
    call("stm_mask_bce_upsampled_backward_f32", _p(_f32c(grad_loss)), _p(pred), _p(target), 1 if is_f32 else 0, _p(idx), _p(grad_pred), n, h, w, G, H,
         W, _stream())
    return grad_pred


def _ohem_args(who, conf_data, conf_t, negpos_ratio):
    """Shapes and dtypes of the OHEM confidence loss, checked before anything touches the device: (x [N,C] fp32 contiguous and 16-byte aligned,
    t [N] int64 contiguous, B, P, C, ratio)."""
    if conf_data.dim() not in (2, 3):
        raise StmError(f"{who}: conf_data must be [B,P,C] or [N,C], got {tuple(conf_data.shape)}")
    C = conf_data.shape[-1]
    N = conf_data.numel() // C if C else 0
    if conf_t.dtype != torch.int64 or conf_t.dim() not in (1, 2) or conf_t.numel() != N:
        raise StmError(f"{who}: conf_t must be int64 with the {N} priors of conf_data {tuple(conf_data.shape)}, got {conf_t.dtype} "
                       f"{tuple(conf_t.shape)}")
    B = conf_data.shape[0] if conf_data.dim() == 3 else (conf_t.shape[0] if conf_t.dim() == 2 else 1)
    if N == 0 or N % B:
        raise StmError(f"{who}: {N} priors do not split into {B} images")
    if int(negpos_ratio) != negpos_ratio or negpos_ratio < 1:
        raise StmError(f"{who}: negpos_ratio must be a positive integer, got {negpos_ratio}")
    _dev(conf_data, conf_t)
    x = _f32c(conf_data).view(N, C)
    if x.data_ptr() % 16:
        x = x.clone()
    return x, conf_t.contiguous().view(N), B, N // B, C, int(negpos_ratio)


def ohem_select_neg(conf_data, conf_t, negpos_ratio=3):
    """multibox_loss.py:402-426 without the sort: float32 [B*P], 1 where the prior is a selected hard negative (stm_ohem_select_neg_f32; the
    conventions are in include/stmask_hip.h and INTEGRATION.md section 14).  7 launches, no host synchronisation."""
    x, t, B, P, C, ratio = _ohem_args("ohem_select_neg", conf_data.detach(), conf_t, negpos_ratio)
    neg = torch.empty(B * P, dtype=torch.float32, device=x.device)
    nbytes = _lib.lib().stm_ohem_conf_workspace_bytes(B, P, C)
    ws = _workspace(nbytes, x.device, "ohem")
    call("stm_ohem_select_neg_f32", _p(x), _p(t), _p(neg), B, P, C, ratio, _p(ws), ws.numel(), _stream())
    return neg


OHEM_WEIGHTS = {"reference": 0, "aligned": 1}


def ohem_conf_loss(conf_data, conf_t, negpos_ratio=3, conf_alpha=1.0, weights="reference"):
    """losses['C'] of multibox_loss.py:428-448 -> (loss 0-dim fp32, lse [N] fp32, w [N] fp32); lse and w are what the backward needs besides the
    inputs.  8 launches, no host synchronisation (stm_ohem_conf_loss_f32)."""
    if weights not in OHEM_WEIGHTS:
        raise StmError(f"ohem_conf_loss: weights must be 'reference' or 'aligned', got {weights!r}")
    x, t, B, P, C, ratio = _ohem_args("ohem_conf_loss", conf_data, conf_t, negpos_ratio)
    dev = x.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    lse = torch.empty(B * P, dtype=torch.float32, device=dev)
    w = torch.empty(B * P, dtype=torch.float32, device=dev)
    nbytes = _lib.lib().stm_ohem_conf_workspace_bytes(B, P, C)
    ws = _workspace(nbytes, dev, "ohem")
    call("stm_ohem_conf_loss_f32", _p(x), _p(t), _p(loss), _p(lse), _p(w), B, P, C, ratio, float(conf_alpha), OHEM_WEIGHTS[weights], _p(ws),
         ws.numel(), _stream())
    return loss, lse, w


def ohem_conf_loss_backward(grad_loss, conf_data, conf_t, lse, w, negpos_ratio=3, conf_alpha=1.0):
    """grad_conf (conf_data's shape) of ohem_conf_loss: grad_loss (a 0-dim device tensor) * conf_alpha / (negpos_ratio + 1) * w_i *
    (softmax(x_i) - onehot(t_i)); rows with w_i = 0 are written as zeros.  One launch."""
    x, t, B, P, C, ratio = _ohem_args("ohem_conf_loss_backward", conf_data, conf_t, negpos_ratio)
    N = B * P
    _dev(grad_loss, lse, w)
    if grad_loss.dtype != torch.float32 or grad_loss.numel() != 1:
        raise StmError(f"ohem_conf_loss_backward: grad_loss must be one float32, got {grad_loss.dtype} {tuple(grad_loss.shape)}")
    if lse.dtype != torch.float32 or w.dtype != torch.float32 or lse.numel() != N or w.numel() != N:
        raise StmError(f"ohem_conf_loss_backward: lse and w must be float32 [{N}]")
    grad = torch.empty(conf_data.shape, dtype=torch.float32, device=x.device)
    call("stm_ohem_conf_loss_backward_f32", _p(grad_loss.contiguous()), _p(x), _p(t), _p(lse.contiguous()), _p(w.contiguous()), _p(grad), B, P, C,
         ratio, float(conf_alpha), _stream())
    return grad


def _box_center_args(who, loc_data, priors, gt_boxes_t, conf_t, centerness_data):
    """Shapes and dtypes of the box / centerness loss, checked before anything touches the device: (loc, priors, per_image, gt, conf_t,
    centerness [B,P] or None, B, P), the boxes fp32, contiguous and 16-byte aligned."""
    if loc_data.dim() != 3 or loc_data.shape[-1] != 4:
        raise StmError(f"{who}: loc_data must be [B,P,4], got {tuple(loc_data.shape)}")
    B, P = loc_data.shape[:2]
    if tuple(priors.shape) not in ((P, 4), (B, P, 4)):
        raise StmError(f"{who}: priors must be [{P},4] or [{B},{P},4], got {tuple(priors.shape)}")
    if tuple(gt_boxes_t.shape) != (B, P, 4):
        raise StmError(f"{who}: gt_boxes_t must be [{B},{P},4], got {tuple(gt_boxes_t.shape)}")
    if conf_t.dtype != torch.int64 or tuple(conf_t.shape) != (B, P):
        raise StmError(f"{who}: conf_t must be int64 [{B},{P}], got {conf_t.dtype} {tuple(conf_t.shape)}")
    if centerness_data is not None and tuple(centerness_data.shape) not in ((B, P), (B, P, 1)):
        raise StmError(f"{who}: centerness_data must be [{B},{P},1] or [{B},{P}], got {tuple(centerness_data.shape)}")
    if B * P == 0:
        raise StmError(f"{who}: no priors in loc_data {tuple(loc_data.shape)}")
    _dev(loc_data, priors, gt_boxes_t, conf_t, centerness_data)

    def box(t):
        t = _f32c(t)
        return t.clone() if t.data_ptr() % 16 else t
    cent = _f32c(centerness_data).view(B, P) if centerness_data is not None else None
    return box(loc_data), box(priors), 1 if priors.dim() == 3 else 0, box(gt_boxes_t), conf_t.contiguous(), cent, B, P


def box_center_loss(loc_data, priors, gt_boxes_t, conf_t, centerness_data=None, bboxiou_alpha=1.0, center_alpha=1.0):
    """losses['BIoU'] (multibox_loss.py:164-172) and losses['center'] (:450-455) -> (biou, center or None, npos int32 [B]); npos is what the
    backward needs besides the inputs.  2 launches, no host synchronisation (stm_box_center_loss_f32)."""
    loc, pri, per_img, gt, t, cent, B, P = _box_center_args("box_center_loss", loc_data, priors, gt_boxes_t, conf_t, centerness_data)
    dev = loc.device
    biou = torch.empty((), dtype=torch.float32, device=dev)
    center = torch.empty((), dtype=torch.float32, device=dev) if cent is not None else None
    npos = torch.empty(B, dtype=torch.int32, device=dev)
    ws = _workspace(_lib.lib().stm_box_center_workspace_bytes(B, P), dev, "bcl")
    call("stm_box_center_loss_f32", _p(loc), _p(pri), per_img, _p(gt), _p(t), _p(cent), _p(biou), _p(center), _p(npos), B, P, float(bboxiou_alpha),
         float(center_alpha), _p(ws), ws.numel(), _stream())
    return biou, center, npos


def box_center_loss_backward(grad_biou, grad_center, loc_data, priors, gt_boxes_t, conf_t, centerness_data, npos, bboxiou_alpha=1.0,
                             center_alpha=1.0, need_centerness=True):
    """(grad_loc, grad_centerness or None) of box_center_loss from the two incoming gradients (0-dim device tensors; None: zero): exact zeros
    outside the positives, decode and DIoU recomputed inside.  One launch."""
    loc, pri, per_img, gt, t, cent, B, P = _box_center_args("box_center_loss_backward", loc_data, priors, gt_boxes_t, conf_t, centerness_data)
    _dev(grad_biou, grad_center, npos)
    for name, g in (("grad_biou", grad_biou), ("grad_center", grad_center)):
        if g is not None and (g.dtype != torch.float32 or g.numel() != 1):
            raise StmError(f"box_center_loss_backward: {name} must be one float32, got {g.dtype} {tuple(g.shape)}")
    if npos.dtype != torch.int32 or npos.numel() != B:
        raise StmError(f"box_center_loss_backward: npos must be int32 [{B}]")
    grad_loc = torch.empty(B, P, 4, dtype=torch.float32, device=loc.device)
    grad_cent = torch.empty(centerness_data.shape, dtype=torch.float32, device=loc.device) if cent is not None and need_centerness else None
    call("stm_box_center_loss_backward_f32", _p(grad_biou), _p(grad_center), _p(loc), _p(pri), per_img, _p(gt), _p(t), _p(cent),
         _p(npos.contiguous()), _p(grad_loc), _p(grad_cent), B, P, float(bboxiou_alpha), float(center_alpha), _stream())
    return grad_loc, grad_cent


def _track_args(who, track_data, conf_t, ids_t):
    if track_data.dim() != 3:
        raise StmError(f"{who}: track_data must be [B,P,D], got {tuple(track_data.shape)}")
    B, P, D = track_data.shape
    for name, t in (("conf_t", conf_t), ("ids_t", ids_t)):
        if t.dtype != torch.int64 or tuple(t.shape) != (B, P):
            raise StmError(f"{who}: {name} must be int64 [{B},{P}], got {t.dtype} {tuple(t.shape)}")
    if B * P == 0:
        raise StmError(f"{who}: no priors in track_data {tuple(track_data.shape)}")
    _dev(track_data, conf_t, ids_t)
    return _f32c(track_data), conf_t.contiguous(), ids_t.contiguous(), B, P, D


def track_loss(track_data, conf_t, ids_t, track_alpha=1.0):
    """losses['T'] of multibox_loss.py:328-351 -> 0-dim fp32; nothing else is kept for the backward.  5 launches, no host synchronisation
    (stm_track_loss_f32)."""
    x, t, ids, B, P, D = _track_args("track_loss", track_data, conf_t, ids_t)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    ws = _workspace(_lib.lib().stm_track_loss_workspace_bytes(B, P, D), x.device, "trl")
    call("stm_track_loss_f32", _p(x), _p(t), _p(ids), _p(loss), B, P, D, float(track_alpha), _p(ws), ws.numel(), _stream())
    return loss


def track_loss_backward(grad_loss, track_data, conf_t, ids_t, track_alpha=1.0):
    """grad_track [B,P,D] of track_loss: the list of positives is rebuilt, the rows that are not positive are zeros.  5 launches."""
    x, t, ids, B, P, D = _track_args("track_loss_backward", track_data, conf_t, ids_t)
    _dev(grad_loss)
    if grad_loss.dtype != torch.float32 or grad_loss.numel() != 1:
        raise StmError(f"track_loss_backward: grad_loss must be one float32, got {grad_loss.dtype} {tuple(grad_loss.shape)}")
    grad = torch.empty(B, P, D, dtype=torch.float32, device=x.device)
    ws = _workspace(_lib.lib().stm_track_loss_workspace_bytes(B, P, D), x.device, "trl")
    call("stm_track_loss_backward_f32", _p(grad_loss.contiguous()), _p(x), _p(t), _p(ids), _p(grad), B, P, D, float(track_alpha), _p(ws), ws.numel(),
         _stream())
    return grad


def _t2s_frames(who, boxes, ids, counts, B, dev):
    counts = [int(c) for c in counts]
    G = sum(counts)
    if len(counts) != B:
        raise StmError(f"{who}: {len(counts)} per-clip box counts for {B} clips")
    if boxes.dtype != torch.float32 or tuple(boxes.shape) != (G, 4) or ids.dtype != torch.int64 or tuple(ids.shape) != (G,):
        raise StmError(f"{who}: boxes {boxes.dtype} {tuple(boxes.shape)} / ids {ids.dtype} {tuple(ids.shape)} for {G} boxes (float32 [G,4], int64 [G])")
    _dev(boxes, ids)
    return boxes.contiguous(), ids.contiguous(), counts, G, (max(counts) if counts else 0)


def t2s_targets(ids_t, boxes_ref, ids_ref, counts_ref, boxes_next, ids_next, counts_next, max_rows=None, offsets=None):
    """The targets of track_to_segment_loss (multibox_loss.py:253-271, :291) for a batch in three launches (stm_t2s_targets_f32).  ids_t int64
    [B,P]; the boxes (fp32 [G,4] point form) and ids (int64 [G]) of the reference and the next frames of all clips concatenated, counts_*: the
    per-clip numbers of boxes (Python ints).  Returns (pos_t int64 [B,P], reg_t [B,P,4], idx_next int64 [B,P], prefix int32 [B+1], state); state
    holds the ordered list of the shift-positive rows for t2s_gather.  No host synchronisation."""
    if ids_t.dtype != torch.int64 or ids_t.dim() != 2 or ids_t.numel() == 0:
        raise StmError(f"t2s_targets: ids_t must be a non-empty int64 [B,P], got {ids_t.dtype} {tuple(ids_t.shape)}")
    _dev(ids_t)
    B, P = ids_t.shape
    dev = ids_t.device
    boxes_ref, ids_ref, counts_ref, Gr, Gr_max = _t2s_frames("t2s_targets", boxes_ref, ids_ref, counts_ref, B, dev)
    boxes_next, ids_next, counts_next, Gn, Gn_max = _t2s_frames("t2s_targets", boxes_next, ids_next, counts_next, B, dev)
    if offsets is None:
        acc = [[0], [0]]
        for a, counts in zip(acc, (counts_ref, counts_next)):
            for c in counts:
                a.append(a[-1] + c)
        both = torch.tensor(acc, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)      # one asynchronous copy, no synchronisation
        offsets = (both[0], both[1])
    ids_t = ids_t.contiguous()
    pos_t = torch.empty(B, P, dtype=torch.int64, device=dev)
    reg_t = torch.empty(B, P, 4, dtype=torch.float32, device=dev)
    idx_next = torch.empty(B, P, dtype=torch.int64, device=dev)
    prefix = torch.empty(B + 1, dtype=torch.int32, device=dev)
    nbytes = _lib.lib().stm_t2s_workspace_bytes(B, P)
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)           # kept by the caller until the gather has run: not the shared scratch
    call("stm_t2s_targets_f32", _p(ids_t), _p(boxes_ref), _p(ids_ref), _p(offsets[0]), Gr, Gr_max, _p(boxes_next), _p(ids_next), _p(offsets[1]), Gn,
         Gn_max, _p(pos_t), _p(reg_t), _p(idx_next), _p(prefix), B, P, int(max_rows) if max_rows else 0, _p(ws), ws.numel(), _stream())
    return pos_t, reg_t, idx_next, prefix, ws


def t2s_gather(state, n_rows, loc_ref, priors, coeff_ref, reg_t, idx_next, boxes_next, feat_h, feat_w):
    """n_rows rows through t2s_targets' list in one launch (stm_t2s_gather_f32) -> dict of rois [n,5], reg [n,4], coeff [n,M], box [n,4], idx
    int64 [n], clip int32 [n], w [n], n_dev int32 [1] (min(live count, n_rows)), status int32 [1] (1: more shift-positives than the cap given to
    t2s_targets).  Rows past the live count are padding.  No host synchronisation."""
    _dev(state, loc_ref, priors, coeff_ref, reg_t, idx_next, boxes_next)
    loc_ref, priors, coeff_ref = _f32c(loc_ref), _f32c(priors), _f32c(coeff_ref)
    if loc_ref.dim() != 3 or loc_ref.shape[2] != 4:
        raise StmError(f"t2s_gather: loc_ref must be [B,P,4], got {tuple(loc_ref.shape)}")
    B, P = loc_ref.shape[:2]
    if tuple(priors.shape) != (P, 4) or coeff_ref.dim() != 3 or tuple(coeff_ref.shape[:2]) != (B, P) or tuple(reg_t.shape) != (B, P, 4) or \
            tuple(idx_next.shape) != (B, P) or idx_next.dtype != torch.int64 or boxes_next.dim() != 2 or boxes_next.shape[0] < 1:
        raise StmError(f"t2s_gather: priors {tuple(priors.shape)}, coeff_ref {tuple(coeff_ref.shape)}, reg_t {tuple(reg_t.shape)}, idx_next "
                       f"{tuple(idx_next.shape)}, boxes_next {tuple(boxes_next.shape)} do not fit loc_ref {tuple(loc_ref.shape)}")
    M = coeff_ref.shape[2]
    n = int(n_rows)
    dev = loc_ref.device
    f32 = dict(dtype=torch.float32, device=dev)
    out = dict(rois=torch.empty(n, 5, **f32), reg=torch.empty(n, 4, **f32), coeff=torch.empty(n, M, **f32), box=torch.empty(n, 4, **f32),
               idx=torch.empty(n, dtype=torch.int64, device=dev), clip=torch.empty(n, dtype=torch.int32, device=dev), w=torch.empty(n, **f32),
               n_dev=torch.empty(1, dtype=torch.int32, device=dev), status=torch.empty(1, dtype=torch.int32, device=dev))
    call("stm_t2s_gather_f32", _p(loc_ref), _p(priors), _p(coeff_ref), _p(_f32c(reg_t)), _p(idx_next.contiguous()), _p(_f32c(boxes_next)),
         boxes_next.shape[0], _p(out["rois"]), _p(out["reg"]), _p(out["coeff"]), _p(out["box"]), _p(out["idx"]), _p(out["clip"]), _p(out["w"]),
         _p(out["n_dev"]), _p(out["status"]), n, B, P, M, feat_h, feat_w, _p(state), state.numel(), _stream())
    return out


def _t2s_rows(who, bbox_reg, reg_rows, bce, box_rows, w_rows, n_dev, status):
    n = bbox_reg.shape[0]
    for name, t, shp in (("bbox_reg", bbox_reg, (n, 4)), ("reg_rows", reg_rows, (n, 4)), ("bce", bce, (n,)), ("box_rows", box_rows, (n, 4)),
                         ("w_rows", w_rows, (n,))):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shp):
            raise StmError(f"{who}: {name} must be float32 {shp}, got {t.dtype} {tuple(t.shape)}")
    if n < 1 or n_dev.dtype != torch.int32 or status.dtype != torch.int32:
        raise StmError(f"{who}: {n} rows, n_dev {n_dev.dtype}, status {status.dtype}")
    _dev(bbox_reg, reg_rows, bce, box_rows, w_rows, n_dev, status)
    return n


def t2s_reduce(bbox_reg, reg_rows, bce, box_rows, w_rows, n_dev, status, bs, H, W, boxshift_alpha=1.0, maskshift_alpha=1.0):
    """(B_shift, M_shift) as 0-dim fp32 from the rows of t2s_gather, TemporalNet's bbox_reg [n,4] and the mask BCE sums bce [n]
    (stm_t2s_reduce_f32: one launch, sums in double in a fixed order)."""
    n = _t2s_rows("t2s_reduce", bbox_reg, reg_rows, bce, box_rows, w_rows, n_dev, status)
    b = torch.empty((), dtype=torch.float32, device=bbox_reg.device)
    m = torch.empty((), dtype=torch.float32, device=bbox_reg.device)
    call("stm_t2s_reduce_f32", _p(bbox_reg.contiguous()), _p(reg_rows.contiguous()), _p(bce.contiguous()), _p(box_rows.contiguous()),
         _p(w_rows.contiguous()), _p(n_dev), _p(status), _p(b), _p(m), n, bs, H, W, float(boxshift_alpha), float(maskshift_alpha), _stream())
    return b, m


def t2s_reduce_backward(grad_b, grad_m, bbox_reg, reg_rows, box_rows, w_rows, n_dev, status, bs, H, W, boxshift_alpha=1.0, maskshift_alpha=1.0,
                        need_reg=True, need_bce=True):
    """(grad_bbox_reg [n,4], grad_bce [n]) of t2s_reduce, written (stm_t2s_reduce_backward_f32: one launch); grad_b / grad_m: one fp32 each or
    None (zero)."""
    n = _t2s_rows("t2s_reduce_backward", bbox_reg, reg_rows, None, box_rows, w_rows, n_dev, status)
    _dev(grad_b, grad_m)
    for g in (grad_b, grad_m):
        if g is not None and (g.dtype != torch.float32 or g.numel() != 1):
            raise StmError(f"t2s_reduce_backward: a loss gradient must be one float32, got {g.dtype} {tuple(g.shape)}")
    g_reg = torch.empty(n, 4, dtype=torch.float32, device=bbox_reg.device) if need_reg else None
    g_bce = torch.empty(n, dtype=torch.float32, device=bbox_reg.device) if need_bce else None
    call("stm_t2s_reduce_backward_f32", _p(grad_b.contiguous() if grad_b is not None else None),
         _p(grad_m.contiguous() if grad_m is not None else None), _p(bbox_reg.contiguous()), _p(reg_rows.contiguous()), _p(box_rows.contiguous()),
         _p(w_rows.contiguous()), _p(n_dev), _p(status), _p(g_reg), _p(g_bce), n, bs, H, W, float(boxshift_alpha), float(maskshift_alpha), _stream())
    return g_reg, g_bce


def lincomb_rows_backward(grad_out, proto, coeff, boxes, row_proto, n_dev=None, apply_tanh=True):
    """grad_coeff [n,M] of lincomb_sigmoid_crop in its row_proto / n_dev form: proto [S,h,w,M], row i uses proto[row_proto[i]].  Two launches,
    fixed-order sums, no atomics (stm_lincomb_rows_backward_f32); no gradient w.r.t. the prototypes or the boxes."""
    _dev(grad_out, proto, coeff, boxes, row_proto, n_dev)
    go, proto, coeff = _f32c(grad_out), _f32c(proto), _f32c(coeff)
    if proto.dim() != 4:
        raise StmError(f"lincomb_rows_backward: proto must be [S,h,w,M], got {tuple(proto.shape)}")
    S, h, w, m = proto.shape
    n = coeff.shape[0]
    if tuple(go.shape) != (n, h, w) or coeff.shape[1] != m or (boxes is not None and tuple(boxes.shape) != (n, 4)) or \
            (row_proto is not None and (row_proto.dtype != torch.int32 or row_proto.numel() != n)) or (row_proto is None and S != 1) or \
            (n_dev is not None and n_dev.dtype != torch.int32):
        raise StmError(f"lincomb_rows_backward: grad_out {tuple(go.shape)}, proto {tuple(proto.shape)}, coeff {tuple(coeff.shape)}, boxes / "
                       "row_proto / n_dev do not match")
    gc = torch.empty_like(coeff)
    if n == 0:
        return gc
    bx = _f32c(boxes) if boxes is not None else None
    rp = row_proto.contiguous() if row_proto is not None else None
    need = _lib.lib().stm_lincomb_rows_backward_workspace_bytes(n, h, w, m)
    ws = _workspace(need, proto.device, "lcrb")
    call("stm_lincomb_rows_backward_f32", _p(go), _p(proto), S, _p(coeff), _p(bx), _p(rp), _p(n_dev), _p(gc), h, w, m, n, 1 if apply_tanh else 0,
         _p(ws), ws.numel(), _stream())
    return gc


def mbox_check_shapes(who, B, P, M=None, n_rows=None):
    """What include/stmask_hip_train.h refuses from the shapes, raised before anything touches the device."""
    if B < 1 or P < 1:
        raise StmError(f"{who}: B={B} P={P}")
    if B * P > 1 << 22:
        raise StmError(f"{who}: B*P={B * P} > {1 << 22} rows")
    if M is not None and M not in (8, 32, 64):
        raise StmError(f"{who}: mask_dim {M} not in {{8,32,64}}")
    if n_rows is not None and not 1 <= n_rows <= 65535:
        raise StmError(f"{who}: {n_rows} rows (1 to 65535)")


def mbox_positives(conf_t, max_rows=None):
    """The ordered list of the positives (conf_t > 0) of a batch in three launches (stm_mbox_positives): conf_t int64 [B,P] -> (prefix int32
    [B+1], the exclusive prefix of the per-image counts with prefix[B] = n, and the list state for mbox_gather / mbox_scatter_coeff).  No host
    synchronisation."""
    if conf_t.dtype != torch.int64 or conf_t.dim() != 2:
        raise StmError(f"mbox_positives: conf_t must be int64 [B,P], got {conf_t.dtype} {tuple(conf_t.shape)}")
    B, P = conf_t.shape
    mbox_check_shapes("mbox_positives", B, P, n_rows=None if max_rows is None else int(max_rows))
    _dev(conf_t)
    dev = conf_t.device
    prefix = torch.empty(B + 1, dtype=torch.int32, device=dev)
    nbytes = _lib.lib().stm_mbox_workspace_bytes(B, P)
    state = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)        # kept by the caller until the scatter has run: not the shared scratch
    call("stm_mbox_positives", _p(conf_t.contiguous()), _p(prefix), B, P, int(max_rows) if max_rows else 0, _p(state), state.numel(), _stream())
    return prefix, state


def mbox_gather(state, n_rows, loc_data, priors, mask_data, idx_t, mask_offs, G_total, H, W):
    """n_rows rows through mbox_positives' list in one launch (stm_mbox_gather_f32) -> dict of coeff [n,M], box [n,4] (the crop box of
    multibox_loss.py:559-563), img int32 [n], idx int64 [n] (row of the concatenated masks), scale [n] (w_r / max(bw W, 1) / max(bh H, 1)),
    n_dev int32 [1], status int32 [1].  Rows past the live count are padding.  No host synchronisation."""
    if loc_data.dim() != 3 or loc_data.shape[2] != 4 or mask_data.dim() != 3:
        raise StmError(f"mbox_gather: loc_data {tuple(loc_data.shape)} / mask_data {tuple(mask_data.shape)} must be [B,P,4] / [B,P,M]")
    B, P = loc_data.shape[:2]
    M = mask_data.shape[2]
    n = int(n_rows)
    mbox_check_shapes("mbox_gather", B, P, M, n)
    if tuple(mask_data.shape[:2]) != (B, P) or tuple(priors.shape) not in ((P, 4), (B, P, 4)) or tuple(idx_t.shape) != (B, P) or \
            idx_t.dtype != torch.int64 or mask_offs.dtype != torch.int32 or mask_offs.numel() != B + 1 or G_total < 1:
        raise StmError(f"mbox_gather: priors {tuple(priors.shape)}, mask_data {tuple(mask_data.shape)}, idx_t {idx_t.dtype} {tuple(idx_t.shape)}, "
                       f"mask_offs {mask_offs.dtype} {tuple(mask_offs.shape)}, {G_total} masks do not fit loc_data {tuple(loc_data.shape)}")
    _dev(state, loc_data, priors, mask_data, idx_t, mask_offs)
    loc_data, priors, mask_data = _f32c(loc_data), _f32c(priors), _f32c(mask_data)
    dev = loc_data.device
    f32 = dict(dtype=torch.float32, device=dev)
    out = dict(coeff=torch.empty(n, M, **f32), box=torch.empty(n, 4, **f32), img=torch.empty(n, dtype=torch.int32, device=dev),
               idx=torch.empty(n, dtype=torch.int64, device=dev), scale=torch.empty(n, **f32),
               n_dev=torch.empty(1, dtype=torch.int32, device=dev), status=torch.empty(1, dtype=torch.int32, device=dev))
    call("stm_mbox_gather_f32", _p(loc_data), _p(priors), 1 if priors.dim() == 3 else 0, _p(mask_data), _p(idx_t.contiguous()), _p(mask_offs),
         int(G_total), _p(out["coeff"]), _p(out["box"]), _p(out["img"]), _p(out["idx"]), _p(out["scale"]), _p(out["n_dev"]), _p(out["status"]), n,
         B, P, M, int(H), int(W), _p(state), state.numel(), _stream())
    return out


def _mbox_rows(who, scale_rows, n_dev, status, other=None):
    n = scale_rows.shape[0]
    for name, t in (("scale_rows", scale_rows), ("bce", other)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (n,)):
            raise StmError(f"{who}: {name} must be float32 [{n}], got {t.dtype} {tuple(t.shape)}")
    if n_dev.dtype != torch.int32 or status.dtype != torch.int32:
        raise StmError(f"{who}: n_dev {n_dev.dtype}, status {status.dtype}")
    mbox_check_shapes(who, 1, 1, n_rows=n)
    _dev(scale_rows, n_dev, status, other)
    return n


def mbox_reduce(bce, scale_rows, n_dev, status, mask_alpha=1.0):
    """losses['M'] before the division by the batch size, 0-dim fp32: mask_alpha * sum_r scale_r bce_r (stm_mbox_reduce_f32: one launch, products
    and sums in double in a fixed order)."""
    n = _mbox_rows("mbox_reduce", scale_rows, n_dev, status, bce)
    loss = torch.empty((), dtype=torch.float32, device=bce.device)
    call("stm_mbox_reduce_f32", _p(bce.contiguous()), _p(scale_rows.contiguous()), _p(n_dev), _p(status), _p(loss), n, float(mask_alpha), _stream())
    return loss


def mbox_reduce_backward(grad_loss, scale_rows, n_dev, status, mask_alpha=1.0):
    """grad_bce [n] of mbox_reduce, written (stm_mbox_reduce_backward_f32: one launch)."""
    n = _mbox_rows("mbox_reduce_backward", scale_rows, n_dev, status)
    _dev(grad_loss)
    if grad_loss.dtype != torch.float32 or grad_loss.numel() != 1:
        raise StmError(f"mbox_reduce_backward: grad_loss must be one float32, got {grad_loss.dtype} {tuple(grad_loss.shape)}")
    g_bce = torch.empty(n, dtype=torch.float32, device=scale_rows.device)
    call("stm_mbox_reduce_backward_f32", _p(grad_loss.contiguous()), _p(scale_rows.contiguous()), _p(n_dev), _p(status), _p(g_bce), n,
         float(mask_alpha), _stream())
    return g_bce


def lincomb_rows_proto_backward(grad_out, proto, coeff, boxes, prefix, status=None):
    """grad_proto [S,h,w,M] of lincomb_sigmoid_crop in its row_proto form with the rows sorted by prototype set: rows prefix[s] .. prefix[s+1]
    (int32 [S+1] on the device) use proto[s].  One or two launches, fixed-order sums, no atomics (stm_lincomb_rows_proto_backward_f32); a set
    without rows gets exact zeros; status int32 [1]: NaN everywhere when it is not 0."""
    _dev(grad_out, proto, coeff, boxes, prefix, status)
    go, proto, coeff, boxes = _f32c(grad_out), _f32c(proto), _f32c(coeff), _f32c(boxes)
    if proto.dim() != 4:
        raise StmError(f"lincomb_rows_proto_backward: proto must be [S,h,w,M], got {tuple(proto.shape)}")
    S, h, w, m = proto.shape
    n = coeff.shape[0]
    mbox_check_shapes("lincomb_rows_proto_backward", 1, 1, m, n)
    if tuple(go.shape) != (n, h, w) or coeff.shape[1] != m or tuple(boxes.shape) != (n, 4) or prefix.dtype != torch.int32 or \
            prefix.numel() != S + 1 or (status is not None and status.dtype != torch.int32):
        raise StmError(f"lincomb_rows_proto_backward: grad_out {tuple(go.shape)}, proto {tuple(proto.shape)}, coeff {tuple(coeff.shape)}, boxes / "
                       "prefix / status do not match")
    gp = torch.empty_like(proto)
    need = _lib.lib().stm_lincomb_rows_proto_backward_workspace_bytes(S, h, w, m)
    ws = _workspace(need, proto.device, "lcrp")
    call("stm_lincomb_rows_proto_backward_f32", _p(go), _p(proto), S, _p(coeff), _p(boxes), _p(prefix.contiguous()), _p(status), _p(gp), h, w, m, n,
         _p(ws), ws.numel(), _stream())
    return gp


def mbox_scatter_coeff(grad_rows, conf_t, state, n_dev, status):
    """grad mask_data [B,P,M] from the gradient of mbox_gather's coefficient rows: one launch, no atomics (stm_mbox_scatter_coeff_f32); rows
    that are not positive are exact zeros."""
    _dev(grad_rows, conf_t, state, n_dev, status)
    grad_rows = _f32c(grad_rows)
    B, P = conf_t.shape
    n, M = grad_rows.shape
    mbox_check_shapes("mbox_scatter_coeff", B, P, M, n)
    grad = torch.empty(B, P, M, dtype=torch.float32, device=grad_rows.device)
    call("stm_mbox_scatter_coeff_f32", _p(grad_rows), _p(conf_t.contiguous()), _p(n_dev), _p(status), _p(grad), n, B, P, M, _p(state),
         state.numel(), _stream())
    return grad


def mask_iou(m1, m2, thr=0.5, group1=None, group2=None):
    """box_utils.py:435-447 on (m > thr).  m1 [n1,h,w], m2 [n2,h,w] soft masks -> [n1,n2].  group1 / group2 (int32, any
    order; sorted rows skip whole workgroups): only pairs of the same group are computed, the others stay 0 (stm_mask_iou_grouped_f32)."""
    _dev(m1, m2, group1, group2)
    m1, m2 = _f32c(m1), _f32c(m2)
    n1, n2 = m1.shape[0], m2.shape[0]
    out = torch.zeros(n1, n2, dtype=torch.float32, device=m1.device)
    if n1 == 0 or n2 == 0:
        return out
    hw = m1[0].numel()
    need = _lib.lib().stm_mask_iou_workspace_bytes(n1, n2, hw)
    ws = _workspace(need, m1.device, "miou")
    if group1 is not None:
        if group1.dtype != torch.int32 or group2.dtype != torch.int32 or group1.numel() != n1 or group2.numel() != n2:
            raise StmError("mask_iou: group arrays must be int32 of lengths n1 and n2")
        call("stm_mask_iou_grouped_f32", _p(m1), n1, _p(m2), n2, hw, thr, _p(out), _p(group1.contiguous()), _p(group2.contiguous()), _p(ws),
             ws.numel(), _stream())
        return out
    call("stm_mask_iou_f32", _p(m1), n1, _p(m2), n2, hw, thr, _p(out), _p(ws), ws.numel(), _stream())
    return out


def bias_act_(y, bias, residual=None, relu=True):
    """In place y = act(y + bias[c] (+ residual)) for a 4-D activation in NCHW-contiguous or channels_last layout
    (fused BN-folded conv epilogue).  Returns y."""
    _dev(y, bias, residual)
    if y.dtype != torch.float32 or y.dim() != 4:
        raise StmError("bias_act_ expects a 4-D float32 activation")
    B, C, H, W = y.shape
    if y.is_contiguous():
        inner = H * W
    elif y.is_contiguous(memory_format=torch.channels_last):
        inner = 1
    else:
        raise StmError("bias_act_: activation must be NCHW-contiguous or channels_last")
    if residual is not None:
        if residual.shape != y.shape or residual.stride() != y.stride():
            residual = residual.contiguous(memory_format=torch.channels_last if inner == 1 else torch.contiguous_format)
    call("stm_bias_act_f32", _p(y), _p(_f32c(bias)), _p(residual), y.numel(), C, inner, 1 if relu else 0, _stream())
    return y


def mask_resize_rle(masks, crop_h, crop_w, out_h, out_w, thr=0.5, max_runs=4096):
    """Mask leg of postprocess_ytbvis on the device: [n,mh,mw] soft masks -> (counts [n,max_runs] int32, n_runs [n] int32)
    = COCO run lengths of the un-padded, bilinearly resized, thresholded masks (column-major)."""
    _dev(masks)
    masks = _f32c(masks)
    n, mh, mw = masks.shape
    counts = torch.zeros(n, max_runs, dtype=torch.int32, device=masks.device)
    n_runs = torch.zeros(n, dtype=torch.int32, device=masks.device)
    if n == 0:
        return counts, n_runs
    need = _lib.lib().stm_mask_rle_workspace_bytes(n, out_h, out_w, max_runs)
    ws = _workspace(need, masks.device, "rle")
    call("stm_mask_resize_rle_f32", _p(masks), n, mh, mw, crop_h, crop_w, out_h, out_w, thr, _p(counts), max_runs, _p(n_runs), _p(ws), ws.numel(),
         _stream())
    return counts, n_runs


def output_frames(frames):
    """[(crop_h, crop_w, out_h, out_w, s_w, s_h)] (s_w = img_w / pad_w, s_h = img_h / pad_h as Python floats) -> the stm_output_frame array of
    output_stage_multi.  The fp32 values are the ones torch itself forms on the device from a Python float: a comparison rounds it to fp32,
    tensor / float multiplies by the fp32 reciprocal of that fp32 value."""
    import numpy as np
    arr = (_lib.OutputFrame * max(1, len(frames)))()
    one = np.float32(1.0)
    for i, (crop_h, crop_w, out_h, out_w, s_w, s_h) in enumerate(frames):
        sw, sh = np.float32(s_w), np.float32(s_h)
        arr[i] = _lib.OutputFrame(int(crop_h), int(crop_w), int(out_h), int(out_w), float(sw), float(sh), float(one / sw), float(one / sh))
    return arr


def output_stage_bytes(n, arena_bytes):
    """Bytes of the step buffer of n rows: header | n records | arena."""
    return ctypes.sizeof(_lib.OutputHeader) + n * ctypes.sizeof(_lib.OutputRow) + int(arena_bytes)


def output_stage_multi(masks, frame_of_row, score, cls, box_id, box, frames, row_keep=None, score_threshold=0.0, thr=0.5, max_runs=4096,
                       out=None, arena_bytes=None, workspace=None):
    """The output stage of a whole step (stm_output_stage_multi_f32, include/stmask_hip_output.h): masks [N,mh,mw] fp32 and, per row,
    frame_of_row int32, score fp32, cls / box_id int32 or int64, box [N,4] fp32 normalised, row_keep uint8 / bool or None; frames: a list of
    (crop_h, crop_w, out_h, out_w, s_w, s_h) or what output_frames made of one.  -> the step buffer, uint8 on the device: stm_output_header |
    N stm_output_row | string arena (`out`, or a new tensor with arena_bytes of arena).  No host wait."""
    _dev(masks, frame_of_row, score, cls, box_id, box, row_keep, out, workspace)
    masks, score, box = _f32c(masks), _f32c(score), _f32c(box)
    if masks.dim() != 3 or box.dim() != 2 or box.shape[1] != 4:
        raise StmError(f"output_stage_multi: masks must be [N,mh,mw] and box [N,4], got {tuple(masks.shape)} and {tuple(box.shape)}")
    n, mh, mw = masks.shape
    if frame_of_row.dtype != torch.int32:
        raise StmError(f"output_stage_multi: frame_of_row must be int32, got {frame_of_row.dtype}")
    for name, t in (("cls", cls), ("box_id", box_id)):
        if t.dtype not in (torch.int32, torch.int64):
            raise StmError(f"output_stage_multi: {name} must be int32 or int64, got {t.dtype}")
    if row_keep is not None:
        if row_keep.dtype not in (torch.uint8, torch.bool):
            raise StmError(f"output_stage_multi: row_keep must be uint8 or bool, got {row_keep.dtype}")
        row_keep = row_keep.contiguous()
    frame_of_row, cls, box_id = frame_of_row.contiguous(), cls.contiguous(), box_id.contiguous()
    if any(t.numel() != n for t in (frame_of_row, score, cls, box_id) + (() if row_keep is None else (row_keep,))) or box.shape[0] != n:
        raise StmError(f"output_stage_multi: every per-row tensor must have {n} rows")
    n_frames = len(frames)
    if not isinstance(frames, ctypes.Array):
        frames = output_frames(frames)
    if out is None:
        out = torch.empty(output_stage_bytes(n, max(4096, 1024 * n) if arena_bytes is None else arena_bytes), dtype=torch.uint8, device=masks.device)
    if out.dtype != torch.uint8 or not out.is_contiguous():
        raise StmError("output_stage_multi: out must be a contiguous uint8 tensor")
    if n == 0:
        out[:ctypes.sizeof(_lib.OutputHeader)].zero_()          # (the library launches nothing for no rows: an empty header says so)
        return out
    max_px = max((int(f.out_h) * int(f.out_w) for f in frames[:n_frames]), default=0)
    ws = workspace if workspace is not None else _workspace(_lib.lib().stm_output_stage_workspace_bytes(n, max_px, max_runs), masks.device, "outstage")
    call("stm_output_stage_multi_f32", _p(masks), n, mh, mw, _p(frame_of_row), _p(score), _p(cls), int(cls.dtype == torch.int64), _p(box_id),
         int(box_id.dtype == torch.int64), _p(box), _p(row_keep), ctypes.cast(frames, c_p), n_frames, float(score_threshold), float(thr),
         int(max_runs), _p(out), out.numel(), _p(ws), ws.numel(), _stream())
    return out


def conv_pack_weights(weight, planes=3, tile_n=128, fmt=0, wscale=None):
    """OIHW fp32 weights -> the pre-split, pre-tiled image the convolution kernels stream (done once per layer).
    tile_n = 64 packs for the 128 x 64-tile planar kernel (stm_conv_geom.tile_n must say so too).
    fmt = 1 / 2: two / one fp16 plane(s) of weight * wscale (power of two bringing max |w| to ~2^10) -> returns
    (packed, 1 / wscale)."""
    _dev(weight)
    weight = _f32c(weight)
    O, C, kh, kw = weight.shape
    if fmt >= 1:
        planes = 2 if fmt == 1 else 1
    nbytes = _lib.lib().stm_conv_packed_weight_bytes_tiled(O, C, kh, kw, planes, tile_n)
    if nbytes == 0:
        raise StmError(f"conv_pack_weights: unsupported weight shape {tuple(weight.shape)} (Cin must be a multiple of 32)")
    packed = torch.empty(nbytes, device=weight.device, dtype=torch.uint8)
    if fmt >= 1:
        import math
        if wscale is None:          # (given: several weight tensors packed under one scale, e.g. the sub-kernels of a window set)
            wmax = float(weight.abs().max())
            wscale = 2.0 ** (10 - math.floor(math.log2(wmax))) if wmax > 0 else 1.0
        call("stm_conv_pack_weights_fmt_f32", _p(weight), _p(packed), O, C, kh, kw, tile_n, fmt, wscale, _stream())
        return packed, 1.0 / wscale
    call("stm_conv_pack_weights_tiled_f32", _p(weight), _p(packed), O, C, kh, kw, planes, tile_n, _stream())
    return packed


def layer_geom(C, O, kh, kw, sh, sw, ph, pw, planes, groups, group_cout=None):
    """ConvGeom of a plain layer: what PlanarConv knows of itself before it sees an input (C per group; group_cout: real channels of padded groups)."""
    g = _lib.ConvGeom()
    g.C, g.Cout, g.kh, g.kw, g.sh, g.sw, g.ph, g.pw, g.planes, g.groups = C, O, kh, kw, sh, sw, ph, pw, planes, groups
    for i, c in enumerate(group_cout or ()):
        g.group_cout[i] = c
    return g


def _window_set(xp, packed_list, windows, B, H, W, C, O, out_h, out_w, out_scale, out_f32=None, out_planes=None):
    """(ConvGeom, weight pointers, ConvWindow array) of a window set: fp16x2 planes, stride 1, 256 x 128 tiles, windows[i] = (kh, kw, ph, pw, Ho, Wo,
    y0, x0) of the out_h x out_w output image.  The one place that writes these fields: conv2d_planar_windows, conv2d_planar_windows_pool and
    PlanarConv.window_segments (which adds its groups) launch what it returns."""
    n = len(windows)
    g = _lib.ConvGeom()
    g.B, g.H, g.W, g.C, g.Cout, g.sh, g.sw, g.planes, g.fmt, g.tile_n = B, H, W, C, O, 1, 1, 2, 1, 128
    g.kh, g.kw, g.Ho, g.Wo = windows[0][0], windows[0][1], windows[0][4], windows[0][5]
    g.win_h, g.win_w = out_h, out_w
    g.out_scale = out_scale
    g.x_np, g.x_plane_stride = xp.shape[2], xp.shape[1] * xp.shape[2] * 32
    if out_planes is not None:
        g.out_np, g.out_plane_stride = out_planes.shape[2], out_planes.shape[1] * out_planes.shape[2] * 32
    if out_f32 is not None:
        g.out_ld = out_f32.shape[-1]
    wins = (_lib.ConvWindow * n)()
    for i, wv in enumerate(windows):
        wins[i].kh, wins[i].kw, wins[i].ph, wins[i].pw, wins[i].Ho, wins[i].Wo, wins[i].y0, wins[i].x0 = wv
    return g, (ctypes.c_void_p * n)(*[p.data_ptr() for p in packed_list]), wins


def conv2d_planar_windows(xp, packed_list, windows, bias, B, H, W, C, O, out_h, out_w, out_scale, relu=True, out_f32=None, out_planes=None):
    """stm_conv2d_planar_windows_f32: several window launches of one fp16x2 layer as one grid.  xp [2, C/32, >= B*H*W, 32]; packed_list[i] /
    windows[i] = (kh, kw, ph, pw, Ho, Wo, y0, x0): sub-kernel weights (conv_pack_weights(..., tile_n=128, fmt=1, wscale=common)) and window of
    the out_h x out_w output image; out_f32 [B*out_h*out_w, O] and / or out_planes [2, O/32, B*out_h*out_w, 32] are written in place."""
    _dev(xp)
    if out_f32 is None and out_planes is None:
        raise StmError("conv2d_planar_windows: no output given")
    g, ptrs, wins = _window_set(xp, packed_list, windows, B, H, W, C, O, out_h, out_w, out_scale, out_f32, out_planes)
    call("stm_conv2d_planar_windows_f32", _p(xp), ptrs, wins, len(windows), _p(bias) if bias is not None else None,
         _p(out_f32) if out_f32 is not None else None, _p(out_planes) if out_planes is not None else None, ctypes.byref(g), 1 if relu else 0, _stream())
    return out_f32 if out_f32 is not None else out_planes


def conv2d_planar_windows_pool(xp, packed_list, windows, bias, B, H, W, C, O, out_h, out_w, out_scale, pool_fix):
    """stm_conv2d_planar_windows_pool_f32: the window set of conv2d_planar_windows with ReLU and the average pool over each out_h x out_w image in
    the epilogue: pool_fix [>= B, O] int64 (32.32 fixed point, zero before the first use) receives the pooled SUMS; nothing is written per pixel."""
    _dev(xp)
    if pool_fix.dtype != torch.int64 or pool_fix.dim() != 2 or pool_fix.shape[0] < B or pool_fix.shape[1] != O or not pool_fix.is_contiguous():
        raise StmError("conv2d_planar_windows_pool: pool_fix must be a contiguous int64 [>= B, O] tensor")
    g, ptrs, wins = _window_set(xp, packed_list, windows, B, H, W, C, O, out_h, out_w, out_scale)
    call("stm_conv2d_planar_windows_pool_f32", _p(xp), ptrs, wins, len(windows), _p(bias) if bias is not None else None, _p(pool_fix), ctypes.byref(g),
         _stream())
    return pool_fix


def temporal_pool_fc(pool_fix, n, npix, weight, bias, n_first=None, clear=True, want_pooled=False):
    """stm_temporal_pool_fc_f32: mean = pool_fix / 2^32 / npix, y = mean @ weight.t() + bias for the first n rows of pool_fix [>= n, C] (int64
    fixed-point sums of conv2d_planar_windows_pool); zeroes the consumed rows when clear.  Returns y [n, n_out] -- or, with n_first, the two
    contiguous blocks (y[:, :n_first], y[:, n_first:]) -- and the means [n, C] when want_pooled."""
    _dev(pool_fix, weight)
    if pool_fix.dtype != torch.int64 or pool_fix.dim() != 2 or not pool_fix.is_contiguous() or pool_fix.shape[0] < n or n < 0:
        raise StmError(f"temporal_pool_fc: pool_fix must be contiguous int64 [>= {n}, C], got {pool_fix.dtype} {tuple(pool_fix.shape)}")
    if weight.dim() != 2 or weight.shape[1] != pool_fix.shape[1] or (bias is not None and bias.numel() != weight.shape[0]):
        raise StmError(f"temporal_pool_fc: weight {tuple(weight.shape)} / bias do not match C = {pool_fix.shape[1]}")
    C, n_out = pool_fix.shape[1], weight.shape[0]
    weight = _f32c(weight)
    dev = pool_fix.device
    nf = n_out if n_first is None else int(n_first)
    out = torch.empty(n, nf, device=dev, dtype=torch.float32)
    out2 = torch.empty(n, n_out - nf, device=dev, dtype=torch.float32) if n_first is not None else None
    pooled = torch.empty(n, C, device=dev, dtype=torch.float32) if want_pooled else None
    call("stm_temporal_pool_fc_f32", _p(pool_fix), n, C, npix, _p(weight), _p(_f32c(bias)) if bias is not None else None, n_out, nf, _p(out),
         _p(out2) if out2 is not None else None, _p(pooled) if pooled is not None else None, 1 if clear else 0, _stream())
    res = (out, out2) if n_first is not None else (out,)
    if want_pooled:
        res = res + (pooled,)
    return res if len(res) > 1 else res[0]


def conv_kxr_supported(O, C, kh, kw, stride, padding, groups, group_cout, fmt, max_tiles=4):
    """Layers the kx-reuse narrow-output kernel (csrc/conv_kxr.hip, stm_conv2d_planar_kxr_f32) takes: stride 1, same padding,
    kw = 3 or 5, fp16 plane formats, at most 16 * max_tiles real output channels per group, at most 4 groups, and a three-stage
    LDS ring that fits (the library refuses the others)."""
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    if fmt not in (1, 2) or (sh, sw) != (1, 1) or kw not in (3, 5) or not (1 <= kh <= 8) or 2 * ph != kh - 1 or 2 * pw != kw - 1:
        return False
    if C % 32 or groups < 1 or groups > 4 or O % groups:
        return False
    cg = O // groups
    real = [(group_cout[i] if group_cout and 0 < group_cout[i] < cg else cg) for i in range(groups)]
    npl = 2 if fmt == 1 else 1
    for r in real:
        nc = -(-r // 16)
        if nc > max_tiles or 16 * nc > cg or cg % 4:       # whole 16-channel tiles are written: they must fit the group's row stride
            return False
        # csrc/conv_kxr.hip kx_pt / kx_depth: some tile of 64 * pt pixels (pt = 4, 3, 2) must leave room for three stages
        if 3 * (npl * (64 * 2 + 16) * 64 + kw * npl * nc * 1024) > 160 * 1024:
            return False
    return True


def conv_kxr_tile_pixels(kw, fmt, channel_tiles):
    """Flat pixels of a workgroup tile of the kx-reuse kernel for kw, the plane format and a group of channel_tiles 16-channel tiles (0: not
    taken).  A centre-window launch covers tile_pixels // kw images per tile."""
    return int(_lib.lib().stm_conv_kxr_tile_pixels(kw, fmt, channel_tiles))


def conv_pack_weights_kxr(weight, geom, wscale=None):
    """OIHW fp32 weights (grouped layers: group g = rows [g * O / groups, ...)) -> the image stm_conv2d_planar_kxr_f32 streams;
    geom: a ConvGeom with C (per group), Cout, kh, kw, groups, group_cout, fmt set.  Returns (packed, 1 / wscale)."""
    _dev(weight)
    weight = _f32c(weight)
    nbytes = _lib.lib().stm_conv_kxr_packed_bytes(ctypes.byref(geom))
    if nbytes == 0:
        raise StmError("conv_pack_weights_kxr: " + _lib.lib().stm_last_error_string().decode(errors="replace"))
    packed = torch.empty(nbytes, device=weight.device, dtype=torch.uint8)
    if wscale is None:          # (given: a layer that holds some of the groups of another one and must round its weights as that one does)
        wscale = _pow2_wscale(weight)
    call("stm_conv_pack_weights_kxr_f32", _p(weight), _p(packed), ctypes.byref(geom), wscale, _stream())
    return packed, 1.0 / wscale


def _pow2_wscale(weight):
    import math
    wmax = float(weight.abs().max())
    return 2.0 ** (10 - math.floor(math.log2(wmax))) if wmax > 0 else 1.0


def chain_pack_tail(w3, w1_next=None, wds=None):
    """conv3 [256, 64(,1,1)] and (optionally) the next block's conv1 [64, 256(,1,1)] -> the tail image of stm_bottleneck_chain_f32; with
    wds [256, 64(,1,1)] (the projection shortcut of a stage's first block) the image of stm_bottleneck_chain_proj_f32.
    Returns (packed, out_scale3, out_scale1)."""
    _dev(w3)
    w3 = _f32c(w3.reshape(256, 64))
    if wds is not None:
        wds = _f32c(wds.reshape(256, 64))
    ws3 = _pow2_wscale(torch.cat([w3, wds], 1) if wds is not None else w3)
    ws1 = 1.0
    if w1_next is not None:
        w1_next = _f32c(w1_next.reshape(64, 256))
        ws1 = _pow2_wscale(w1_next)
    L = _lib.lib()
    packed = torch.zeros(L.stm_chain_tail_weight_bytes_proj() if wds is not None else L.stm_chain_tail_weight_bytes(), device=w3.device, dtype=torch.uint8)
    pw1 = _p(w1_next) if w1_next is not None else None
    if wds is not None:
        call("stm_chain_pack_tail_proj_f32", _p(w3), _p(wds), pw1, _p(packed), ws3, ws1, _stream())
    else:
        call("stm_chain_pack_tail_f32", _p(w3), pw1, _p(packed), ws3, ws1, _stream())
    return packed, 1.0 / ws3, 1.0 / ws1


def bottleneck_chain(mid1, x, w2_packed, tail_packed, b2, b3, b1_next, scales, B, H, W, y=None, z=None, want_z=True, proj=False):
    """csrc/conv_chain.hip: mid1 [2, 2, BHW, 32] and x [2, 8, BHW, 32] fp16 planes -> (y [2, 8, BHW, 32], z [2, 2, BHW, 32] or None):
    relu(conv3(relu(conv2(mid1))) + x) and the next block's relu(conv1(y)) in one launch (reference backbone.py:38-58).  proj=True: x is
    the 64-channel input [2, 2, BHW, 32] of a stage's first block and the shortcut its projection (tail from chain_pack_tail(..., wds=))."""
    _dev(mid1)
    n = B * H * W
    xs = 2 if proj else 8
    if tuple(mid1.shape) != (2, 2, n, 32) or tuple(x.shape) != (2, xs, n, 32) or mid1.dtype != torch.float16 or x.dtype != torch.float16:
        raise StmError(f"bottleneck_chain: planes {tuple(mid1.shape)} / {tuple(x.shape)} do not match [2, 2, {n}, 32] / [2, {xs}, {n}, 32] fp16")
    if not (mid1.is_contiguous() and x.is_contiguous()):
        raise StmError("bottleneck_chain: planes must be dense")
    if y is None:
        y = torch.empty(2, 8, n, 32, device=mid1.device, dtype=torch.float16)
    if want_z and z is None:
        z = torch.empty(2, 2, n, 32, device=mid1.device, dtype=torch.float16)
    s2, s3, s1 = scales
    call("stm_bottleneck_chain_proj_f32" if proj else "stm_bottleneck_chain_f32", _p(mid1), _p(x), _p(y), _p(z) if want_z else None, _p(w2_packed),
         _p(tail_packed), _p(b2) if b2 is not None else None, _p(b3) if b3 is not None else None,
         _p(b1_next) if (want_z and b1_next is not None) else None, s2, s3, s1, B, H, W, _stream())
    return y, (z if want_z else None)


def plane_layout(fmt):
    """(number of planes, element type) of a planar format: 0 = bf16 x 3, 1 = fp16 x 2, 2 = fp16 x 1 (include/stmask_hip.h)."""
    if fmt == 0:
        return 3, torch.bfloat16
    if fmt in (1, 2):
        return (2 if fmt == 1 else 1), torch.float16
    raise StmError(f"unknown planar format {fmt}")


def _empty_planes(fmt, slabs, n, device):
    P, dt = plane_layout(fmt)
    return torch.empty(P, slabs, n, 32, device=device, dtype=dt)


def split_planes(x, fmt=0):
    """fp32 NHWC tensor [..., C] (C % 32 == 0) -> planes [P, C/32, N, 32] (N = product of the leading dims) whose fp32 sum is
    x: fmt 0 = three bf16 planes (exact), fmt 1 = two fp16 planes (22 bits; |x| < 65504).  Channel-slab-major: see
    include/stmask_hip.h."""
    _dev(x)
    x = _f32c(x)
    C = x.shape[-1]
    N = x.numel() // C
    if C % 32:
        raise StmError(f"split_planes: channel count {C} is not a multiple of 32")
    planes = _empty_planes(fmt, C // 32, N, x.device)
    call("stm_split_planes_fmt_f32", _p(x), _p(planes), N, C, fmt, _stream())
    return planes


F16_LOW_SCALE = 2048.0   # fp16 plane format: x = h + l / 2048 (include/stmask_hip.h, stm_conv_geom.fmt)

_range_flags = {}


def planar_range_flag():
    """The sticky fp16-range flag of this device (stm_planar_set_range_flag): an int32 tensor of one element that every
    producer of fp16 planes sets to 1 when it meets |x| > 65504, inf or nan.  Registered with the library on first use."""
    dev = torch.cuda.current_device()
    flag = _range_flags.get(dev)
    if flag is None:
        flag = torch.zeros(1, device=f"cuda:{dev}", dtype=torch.int32)
        with torch.cuda.device(dev):         # the library keeps one flag per device: register on the device that owns it
            call("stm_planar_set_range_flag", _p(flag))
        _range_flags[dev] = flag
    return flag


class RangeError(StmError):
    """An activation left the range of the fp16 plane formats (the sticky device flag of stm_planar_set_range_flag was found set).  The batched
    pipeline catches it, rebuilds the inference graph with bf16x3 planes (any fp32 range) and repeats the step."""


RANGE_MESSAGE = ("an activation left the range of the {} planar format (|x| > 65504, inf or nan): results of this step are "
                 "invalid; build the graph with optimize_for_inference(net, planar=True, planes='bf16x3')")
# the plane format of the graph attached last (fuse.attach_planar), named in the message.  Process-global like planar.set_format:
# with nets of different formats in one process the message names the last one attached, not necessarily the one that raised
_range_format = "fp16x2"


def set_range_format(planes):
    global _range_format
    _range_format = planes


def range_message():
    return RANGE_MESSAGE.format(_range_format)


def check_planar_range():
    """Synchronising check of the flag (callers with a host read of their own fold the flag into it instead)."""
    flag = _range_flags.get(torch.cuda.current_device())
    if flag is not None and int(flag.item()):
        flag.zero_()
        raise RangeError(range_message())


def counts_to_host(cnt, extra=None):
    """cnt.tolist() for an integer device tensor -- the host read every detection step does -- with the fp16 range flag
    of the device (if a fp16 planar graph registered one) riding in the same copy.  Raises StmError when the flag is set.
    extra: an fp32 tensor that travels in the same copy (the Fast-NMS scores the tracker's host logic needs); returns
    (counts, extra as a flat numpy array) then."""
    flag = _range_flags.get(cnt.device.index) if cnt.is_cuda else None
    if flag is None and extra is None:
        return cnt.tolist()
    parts = [cnt.reshape(-1).to(torch.int32)]
    if flag is not None:
        parts.append(flag)
    if extra is not None:
        parts.append(extra.reshape(-1).view(torch.int32))
    host = torch.cat(parts).cpu()
    n = cnt.numel()
    if flag is not None and int(host[n]):
        flag.zero_()
        raise RangeError(range_message())
    counts = host[:n].tolist()
    if extra is None:
        return counts
    return counts, host[n + (1 if flag is not None else 0):].view(torch.float32).numpy()


# ---- tracker bookkeeping of the batched pipeline (csrc/tracker.hip) -----------------------------------------------------
def gather_detections(idx, cls, score, box, cnt, mask_coeff, track, centerness, D):
    """Fast-NMS survivors of detect_cc ([B,top_k] slots, device counts) -> concatenated detection rows (dict of [D, ...]
    tensors: box, class, score, mask_coeff, track, centerness, clip).  D = sum of the counts as read by the host."""
    _dev(idx, cls, score, box, cnt, mask_coeff, track, centerness)
    B, top_k = idx.shape
    N, mdim, edim = mask_coeff.shape[1], mask_coeff.shape[2], track.shape[2]
    dev = idx.device
    out = {"box": torch.empty(D, 4, device=dev), "class": torch.empty(D, dtype=torch.int64, device=dev), "score": torch.empty(D, device=dev),
           "mask_coeff": torch.empty(D, mdim, device=dev), "track": torch.empty(D, edim, device=dev), "centerness": torch.empty(D, device=dev),
           "clip": torch.empty(D, dtype=torch.int32, device=dev)}
    cen = _f32c(centerness.reshape(B, N)) if centerness is not None else None
    call("stm_gather_detections_f32", _p(idx), _p(cls), _p(_f32c(score)), _p(_f32c(box)), _p(cnt), _p(_f32c(mask_coeff)), _p(_f32c(track)), _p(cen),
         B, top_k, N, mdim, edim, D, _p(out["box"]), _p(out["class"]), _p(out["score"]), _p(out["mask_coeff"]), _p(out["track"]),
         _p(out["centerness"]), _p(out["clip"]), _stream())
    return out


def shift_rois(box, clip, feat_h, feat_w):
    """CandidateShift's RoIs: [n, 5] = (clip, x1, y1, x2, y2 in feature-map pixels, order-fixed and clamped)."""
    _dev(box, clip)
    n = box.shape[0]
    rois = torch.empty(n, 5, device=box.device)
    call("stm_shift_rois_f32", _p(_f32c(box)), _p(clip), _p(rois), n, feat_h, feat_w, _stream())
    return rois


def shift_apply_(loc_shift, coeff_shift, box, mask_coeff, score, decay=0.95):
    """In place: box = decode(loc_shift, center_size(box)); mask_coeff += coeff_shift; score *= decay (TF_utils.py:40-48)."""
    _dev(loc_shift, coeff_shift, box, mask_coeff, score)
    for t in (box, mask_coeff, score):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise StmError("shift_apply_: box / mask_coeff / score must be contiguous fp32 (modified in place)")
    call("stm_shift_apply_f32", _p(_f32c(loc_shift)), _p(_f32c(coeff_shift)), _p(box), _p(mask_coeff), _p(score), box.shape[0], mask_coeff.shape[1],
         decay, _stream())


def match_scores(cos, miou, det_box, prev_box, det_score, det_cls, prev_cls, det_clip, prev_offsets, match_coeff, dummy_iou=0.3):
    """compute_comp_scores + argmax over [dummy | prev rows of the same clip] -> int32 [D]: 0 = new instance, 1 + prev row."""
    _dev(cos, miou, det_box, prev_box, det_score, det_cls, prev_cls, det_clip, prev_offsets)
    D, Pn = det_box.shape[0], prev_box.shape[0]
    match = torch.empty(D, dtype=torch.int32, device=det_box.device)
    c4 = (ctypes.c_float * 4)(*[float(v) for v in match_coeff])
    call("stm_match_scores_f32", _p(_f32c(cos)), _p(_f32c(miou)), _p(_f32c(det_box)), _p(_f32c(prev_box)), _p(_f32c(det_score)), _p(det_cls),
         _p(prev_cls), _p(det_clip), _p(prev_offsets), D, Pn, c4, dummy_iou, _p(match), _stream())
    return match


def match_scores_embed(det_track, prev_track, miou, det_box, prev_box, det_score, det_cls, prev_cls, det_clip, prev_offsets, match_coeff,
                       dummy_iou=0.3):
    """match_scores with the cosine term computed in the kernel from the track embeddings (same-clip pairs only): no [D, Pn]
    matrix product in front of it."""
    _dev(det_track, prev_track, miou, det_box, prev_box, det_score, det_cls, prev_cls, det_clip, prev_offsets)
    D, Pn = det_box.shape[0], prev_box.shape[0]
    match = torch.empty(D, dtype=torch.int32, device=det_box.device)
    c4 = (ctypes.c_float * 4)(*[float(v) for v in match_coeff])
    call("stm_match_scores_embed_f32", _p(_f32c(det_track)), _p(_f32c(prev_track)), det_track.shape[1], _p(_f32c(miou)), _p(_f32c(det_box)),
         _p(_f32c(prev_box)), _p(_f32c(det_score)), _p(det_cls), _p(prev_cls), _p(det_clip), _p(prev_offsets), D, Pn, c4, dummy_iou, _p(match),
         _stream())
    return match


def gather_rows2(a_rows, b_rows, plan, n_a):
    """out_t[r] = plan[r] < n_a ? a_t[plan[r]] : b_t[plan[r] - n_a] for lists of row tensors (<= 8 per launch); plan int32."""
    _dev(plan, *a_rows, *b_rows)
    if plan.dtype != torch.int32:
        raise StmError("gather_rows2: plan must be int32")
    R = plan.shape[0]
    outs = []
    for i in range(0, len(a_rows), 8):
        aa, bb = [t.contiguous() for t in a_rows[i:i + 8]], [t.contiguous() for t in b_rows[i:i + 8]]
        oo = [torch.empty((R,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in aa]
        n = len(aa)
        rb = [t[0].numel() * t.element_size() if t.shape[0] else (bb[k][0].numel() * bb[k].element_size()) for k, t in enumerate(aa)]
        pa = (ctypes.c_void_p * n)(*[t.data_ptr() for t in aa])
        pb = (ctypes.c_void_p * n)(*[t.data_ptr() for t in bb])
        po = (ctypes.c_void_p * n)(*[t.data_ptr() for t in oo])
        prb = (ctypes.c_int * n)(*rb)
        call("stm_gather_rows2", pa, pb, po, prb, n, _p(plan), R, n_a, _stream())
        outs += oo
    return outs


def pack_tracked(mask, score, tracked, offsets, box, cls, mask_coeff, B, top_k, cols, max_age=10, score_thr=0.05):
    """Keep rule of track_TF.py:158-165 + scatter into the fixed-shape [B, top_k, cols] detection rows (stmask_amd.dist layout)."""
    _dev(mask, score, tracked, offsets, box, cls, mask_coeff)
    n = box.shape[0]
    out = torch.empty(B, top_k, cols, device=offsets.device, dtype=torch.float32)
    keep = torch.empty(max(n, 1), dtype=torch.int32, device=offsets.device)
    hw = mask[0].numel() if n else 1
    call("stm_pack_tracked_f32", _p(_f32c(mask)) if n else c_p(0), _p(score), _p(tracked), _p(offsets), _p(box), _p(cls), _p(mask_coeff), n, hw, B,
         top_k, cols, mask_coeff.shape[1] if n else cols - 8, max_age, score_thr, _p(keep), _p(out), _stream())
    return out


def pack_tracked_bits(bits, score, tracked, offsets, box, cls, mask_coeff, B, top_k, cols, max_age=10, score_thr=0.05):
    """pack_tracked with the keep rule's pixel count taken from the masks' bit words [n, words] (lincomb_sigmoid_crop_bits)."""
    _dev(bits, score, tracked, offsets, box, cls, mask_coeff)
    n = box.shape[0]
    out = torch.empty(B, top_k, cols, device=offsets.device, dtype=torch.float32)
    keep = torch.empty(max(n, 1), dtype=torch.int32, device=offsets.device)
    if n and (bits.dtype != torch.int64 or bits.shape[0] != n or not bits.is_contiguous()):
        raise StmError("pack_tracked_bits: bits must be contiguous int64 words [n, words]")
    call("stm_pack_tracked_bits_f32", _p(bits) if n else c_p(0), bits.shape[1] if n else 1, _p(score), _p(tracked), _p(offsets), _p(box), _p(cls),
         _p(mask_coeff), n, B, top_k, cols, mask_coeff.shape[1] if n else cols - 8, max_age, score_thr, _p(keep), _p(out), _stream())
    return out


def _i32c(who, *ts):
    for t in ts:
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise StmError(f"{who}: expected contiguous int32 tensors, got {t.dtype}")


# ---- the tracker's decisions on the device (csrc/track_resolve.hip, include/stmask_hip_tracker.h) ----------------------------------------
def track_resolve_tf(match, det_score, det_count, prev_offsets, prev_tm, n_prev, n_det, cap=0):
    """track_host.match_tf on the device, for all clips in one launch -> (plan, new offsets [B + 1], new counters), the plan and the counters
    at the capacity n_prev + n_det: indices into cat(tracked rows, detection rows) clip after clip, compact from entry 0, then zeros (index 0
    is a valid row, so gather_rows2 may run over the whole plan; new offsets[B] says how many rows are real).  match int32 [n_det] (0 or 1 +
    the tracked row) or None = all 0; det_score fp32 [n_det]; det_count int32 [B]; prev_offsets int32 [B + 1]; prev_tm int32 [n_prev] (None
    when n_prev is 0).  No host read."""
    _dev(match, det_score, det_count, prev_offsets, prev_tm)
    _i32c("track_resolve_tf", match, det_count, prev_offsets, prev_tm)
    B, dev = det_count.shape[0], det_count.device
    if prev_offsets.shape[0] != B + 1 or (match is not None and match.shape[0] != n_det) or (n_det and det_score.shape[0] != n_det) or (
            n_prev and prev_tm.shape[0] < n_prev):
        raise StmError("track_resolve_tf: tensor sizes do not fit n_prev / n_det / the clip count")
    plan = torch.empty(n_prev + n_det, dtype=torch.int32, device=dev)
    new_tm = torch.empty(n_prev + n_det, dtype=torch.int32, device=dev)
    new_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    call("stm_track_resolve_tf", _p(match), _p(_f32c(det_score)) if n_det else c_p(0), _p(det_count), _p(prev_offsets), _p(prev_tm) if n_prev else c_p(0),
         B, n_prev, n_det, int(cap), _p(plan), _p(new_off), _p(new_tm), _stream())
    return plan, new_off, new_tm


def track_drop_plan(offsets, drop, n_keep):
    """track_host.keep_rows on the device -> (rows that stay int32 [n_keep], new offsets [B + 1]).  offsets int32 [B + 1]; drop int32 [B]
    (non-zero: the clip's rows leave); n_keep: the kept clips' rows in all (the host knows every clip's row count)."""
    _dev(offsets, drop)
    _i32c("track_drop_plan", offsets, drop)
    B = drop.shape[0]
    if offsets.shape[0] != B + 1:
        raise StmError("track_drop_plan: offsets must hold one entry more than drop")
    keep = torch.empty(n_keep, dtype=torch.int32, device=offsets.device)
    new_off = torch.empty(B + 1, dtype=torch.int32, device=offsets.device)
    call("stm_track_drop_plan", _p(offsets), _p(drop), B, n_keep, _p(keep), _p(new_off), _stream())
    return keep, new_off


def resize_bilinear_planes(x_nhwc, size, fmt=0):
    """F.interpolate(x, size=size, mode="bilinear", align_corners=False) of an fp32 NHWC tensor [B,H,W,C], returned as planes
    [P, C/32, B*Ho*Wo, 32] (split_planes' format) without the fp32 intermediate."""
    _dev(x_nhwc)
    x = _f32c(x_nhwc)
    B, H, W, C = x.shape
    Ho, Wo = size
    if C % 32:
        raise StmError(f"resize_bilinear_planes: channel count {C} is not a multiple of 32")
    planes = _empty_planes(fmt, C // 32, B * Ho * Wo, x.device)
    call("stm_resize_bilinear_planes_f32", _p(x), _p(planes), B, H, W, C, Ho, Wo, fmt, _stream())
    return planes


def bias_relu_maxpool_planes(x_nhwc, bias, fmt=0):
    """relu(max_pool2d(x, 3, 2, 1) + bias) of an fp32 NHWC tensor [B,H,W,C] (the ResNet stem's convolution output), returned as
    planes [P, C/32, B*Ho*Wo, 32] plus (Ho, Wo)."""
    _dev(x_nhwc, bias)
    x = _f32c(x_nhwc)
    B, H, W, C = x.shape
    if C % 32:
        raise StmError(f"bias_relu_maxpool_planes: channel count {C} is not a multiple of 32")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    planes = _empty_planes(fmt, C // 32, B * Ho * Wo, x.device)
    call("stm_bias_relu_maxpool_planes_f32", _p(x), _p(_f32c(bias)) if bias is not None else c_p(0), _p(planes), B, H, W, C, fmt, _stream())
    return planes, (Ho, Wo)


def roi_align_planes(t2s_prev_nhwc, t2s_nhwc, corr, rois, output_size=7, fmt=0, corr_nhwc=0):
    """relu(cat([corr, T2S_prev, T2S], 1)) -> roi_align(output_size, aligned, adaptive grid) as planes
    [P, Cpad/32, n*ph*pw, 32] with channel order [T2S_prev | T2S | corr | zero padding] (stm_roi_align_planes_f32).  corr is
    [B, Cc, H, W], or with corr_nhwc = Cc the channels-last [B, H, W, ld] of corr_patch_nhwc."""
    _dev(t2s_prev_nhwc, t2s_nhwc, corr, rois)
    a, b, c, rois = _f32c(t2s_prev_nhwc), _f32c(t2s_nhwc), _f32c(corr), _f32c(rois)
    B, H, W, C1 = a.shape
    ok = (tuple(c.shape[:3]) == (B, H, W) and c.shape[3] >= corr_nhwc) if corr_nhwc else (c.shape[0] == B and tuple(c.shape[2:]) == (H, W))
    if tuple(b.shape) != (B, H, W, C1) or not ok:
        raise StmError(f"roi_align_planes: shapes {tuple(a.shape)}, {tuple(b.shape)}, {tuple(c.shape)} do not match")
    Cc, n = (corr_nhwc or c.shape[1]), rois.shape[0]
    ph, pw = _pair(output_size)
    cpad = -(-(2 * C1 + Cc) // 32) * 32
    planes = _empty_planes(fmt, cpad // 32, n * ph * pw, a.device)
    if n:
        call("stm_roi_align_planes_nhwc_f32", _p(a), _p(b), _p(c), c.shape[3] if corr_nhwc else 0, _p(rois), _p(planes), B, H, W, C1, Cc, n, ph, pw,
             fmt, _stream())
    return planes


def stem_rows_planes(x_nhwc, kw, sw, pw, fmt=0):
    """fp32 frame [B,H,W,Cin] (kw*Cin <= 32) -> planes R [P, 1, B*H*Wo, 32]: the kw*Cin contiguous values one kernel row reads for
    each output column (stm_stem_rows_planes_f32); returns (planes, Wo)."""
    _dev(x_nhwc)
    x = _f32c(x_nhwc)
    B, H, W, Cin = x.shape
    Wo = (W + 2 * pw - kw) // sw + 1
    planes = _empty_planes(fmt, 1, B * H * Wo, x.device)
    call("stm_stem_rows_planes_f32", _p(x), _p(planes), B, H, W, Cin, kw, sw, pw, fmt, _stream())
    return planes, Wo


def stem_pack_weights(weight, fmt):
    """conv1 weights [64, 3, 7, 7] -> the fragment image stm_stem_fused_f32 keeps in registers; returns (packed, 1 / wscale)."""
    _dev(weight)
    weight = _f32c(weight)
    O = weight.shape[0]
    nbytes = _lib.lib().stm_stem_packed_weight_bytes(O, fmt)
    if nbytes == 0 or tuple(weight.shape[1:]) != (3, 7, 7):
        raise StmError(f"stem_pack_weights: unsupported stem {tuple(weight.shape)} / format {fmt}")
    import math
    wmax = float(weight.abs().max())
    wscale = 2.0 ** (10 - math.floor(math.log2(wmax))) if wmax > 0 else 1.0
    packed = torch.empty(nbytes, device=weight.device, dtype=torch.uint8)
    call("stm_stem_pack_weights_f32", _p(weight), _p(packed), O, fmt, wscale, _stream())
    return packed, 1.0 / wscale


def stem_fused(x_nhwc, packed, out_scale, bias, fmt, out_fmt=None):
    """conv1 (7x7 / 2 / 3, BN folded) + ReLU + MaxPool2d(3, 2, 1) in one kernel: fp32 frame [B,H,W,3] -> (planes [P, 2, B*Hp*Wp, 32],
    (Hp, Wp)).  stm_stem_fused_f32."""
    _dev(x_nhwc, packed, bias)
    x = _f32c(x_nhwc)
    B, H, W, Cin = x.shape
    if Cin != 3:
        raise StmError(f"stem_fused: 3-channel frames only, got {Cin}")
    out_fmt = fmt if out_fmt is None else out_fmt
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    planes = _empty_planes(out_fmt, 2, B * Hp * Wp, x.device)
    call("stm_stem_fused_f32", _p(x), _p(packed), _p(_f32c(bias)) if bias is not None else c_p(0), _p(planes), B, H, W, 64, fmt, out_fmt, out_scale,
         _stream())
    return planes, (Hp, Wp)


def planes_to_f32(planes):
    """[P, S, N, 32] planes -> fp32 [N, 32*S]."""
    v = planes[0].float()
    if planes.dtype == torch.float16:
        if planes.shape[0] == 2:
            v = v + planes[1].float() / F16_LOW_SCALE
    else:
        for p in range(1, planes.shape[0]):
            v = v + planes[p].float()
    return v.permute(1, 0, 2).reshape(v.shape[1], -1)


def conv2d_planar(xp, packed, weight_shape, hw, bias=None, residual=None, stride=1, padding=0, relu=False, planes=3,
                  out="planes", tile_n=128, fmt=0, out_scale=1.0):
    """The same convolution on the planar activation format: xp [P, C/32, B*H*W, 32] (split_planes / a previous layer's
    output), hw = (B, H, W).  `residual` may be fp32 [B*Ho*Wo, O] or planes [P, O/32, B*Ho*Wo, 32].
    out: "planes" | "f32" | "both"; fp32 result [B*Ho*Wo, O].  fmt 1: fp16 planes, `packed` / `out_scale` from
    conv_pack_weights(..., fmt=1).  fmt 0 with planes = 2 (weights packed with planes = 2): the three-product mode, which reads planes 0
    and 1 of xp -- all three planes or only those two may be given; outputs and a planar residual always have three."""
    _dev(xp, packed, bias, residual)
    P, dt = plane_layout(fmt)
    if fmt >= 1:
        planes = P
    if xp.dtype != dt or xp.dim() != 4 or xp.shape[0] not in (P, planes) or xp.shape[3] != 32 or not xp.is_contiguous():
        raise StmError(f"conv2d_planar: expected contiguous {dt} planes [{P},C/32,N,32], got {xp.dtype} {tuple(xp.shape)}")
    O, C, kh, kw = weight_shape
    B, H, W = hw
    if xp.shape[1] * 32 != C or xp.shape[2] != B * H * W:
        raise StmError(f"conv2d_planar: planes {tuple(xp.shape)} do not match C={C}, B*H*W={B * H * W}")
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    Ho, Wo = conv_out_hw(H, W, kh, kw, sh, sw, ph, pw, 1, 1)
    M = B * Ho * Wo
    y32 = torch.empty(M, O, device=xp.device, dtype=torch.float32) if out in ("f32", "both") else None
    ypl = torch.empty(P, -(-O // 32), M, 32, device=xp.device, dtype=dt) if out in ("planes", "both") else None
    r32 = rpl = None
    if residual is not None:
        if residual.dtype == dt:
            if tuple(residual.shape) != (P, -(-O // 32), M, 32) or not residual.is_contiguous():
                raise StmError(f"conv2d_planar: residual planes {tuple(residual.shape)} != {(P, -(-O // 32), M, 32)}")
            rpl = residual
        else:
            r32 = _f32c(residual)
            if r32.numel() != M * O:
                raise StmError(f"conv2d_planar: residual has {r32.numel()} elements, output {M * O}")
    g = _lib.ConvGeom(B, H, W, C, Ho, Wo, O, kh, kw, sh, sw, ph, pw, 0, 0, 0, planes)
    g.tile_n, g.fmt, g.out_scale = tile_n, fmt, out_scale
    call("stm_conv2d_planar_f32", _p(xp), _p(packed), _p(_f32c(bias) if bias is not None else None), _p(r32), _p(rpl), _p(y32), _p(ypl),
         ctypes.byref(g), 1 if relu else 0, _stream())
    return (y32, ypl) if out == "both" else (y32 if out == "f32" else ypl)


def preprocess_frames(img_u8, size=(640, 360), divisor=32, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375),
                      mode=1):
    """eval.py:703-717 on the device: uint8 [n,H0,W0,3] -> fp32 [n,3,Hp,Wp]; size = (w, h) as mmcv.imresize takes it."""
    _dev(img_u8)
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[-1] != 3:
        raise StmError(f"preprocess_frames: expected uint8 [n,H,W,3], got {img_u8.dtype} {tuple(img_u8.shape)}")
    img = img_u8.contiguous()
    n, H0, W0, _ = img.shape
    w, h = size
    Hp, Wp = -(-h // divisor) * divisor, -(-w // divisor) * divisor
    out = torch.empty(n, 3, Hp, Wp, device=img.device, dtype=torch.float32)
    m3, s3 = (ctypes.c_double * 3)(*mean), (ctypes.c_double * 3)(*std)
    call("stm_preprocess_u8_f32", _p(img), _p(out), n, H0, W0, h, w, Hp, Wp, m3, s3, mode, _stream())
    return out


def preprocess_frames_multi(frames, out=None, size=(640, 360), divisor=32, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375),
                            mode=1):
    """preprocess_frames for n frames that need not share a tensor or a source size: frames = sequence of uint8 [H_i, W_i, 3] device tensors
    (rows may be strided, e.g. a crop view; pixels and channels contiguous).  One launch per 64 frames writes image i into out[i]
    ([n, 3, Hp, Wp] fp32 contiguous, allocated when None), bit-identical to preprocess_frames of that image alone."""
    frames = list(frames)
    if not frames:
        raise StmError("preprocess_frames_multi: no frames")
    _dev(*frames)
    w, h = size
    Hp, Wp = -(-h // divisor) * divisor, -(-w // divisor) * divisor
    n, dev = len(frames), frames[0].device
    desc = (_lib.FrameDesc * n)()
    keep = []                                       # contiguous copies made here live until the launch is enqueued (same stream)
    for i, f in enumerate(frames):
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[-1] != 3 or f.device != dev:
            raise StmError(f"preprocess_frames_multi: frame {i}: expected uint8 [H,W,3] on {dev}, got {f.dtype} {tuple(f.shape)} on {f.device}")
        if f.stride(2) != 1 or f.stride(1) != 3 or f.stride(0) < 3 * f.shape[1]:
            f = f.contiguous()
            keep.append(f)
        desc[i].ptr, desc[i].H0, desc[i].W0, desc[i].row_stride_bytes = f.data_ptr(), f.shape[0], f.shape[1], f.stride(0)
    if out is None:
        out = torch.empty(n, 3, Hp, Wp, device=dev, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, 3, Hp, Wp) or not out.is_contiguous() or out.device != dev:
        raise StmError(f"preprocess_frames_multi: out must be contiguous fp32 {(n, 3, Hp, Wp)} on {dev}, got {out.dtype} {tuple(out.shape)}")
    m3, s3 = (ctypes.c_double * 3)(*mean), (ctypes.c_double * 3)(*std)
    call("stm_preprocess_u8_multi_f32", desc, n, _p(out), h, w, Hp, Wp, m3, s3, mode, _stream())
    return out


def head_assemble(small, trk, B, sizes, n_cls, mask_dim, embed_dim, group_pad):
    """prediction_head_FC.py:168-195 for the planar head: small / trk = per-kernel-shape lists of [pixels, 3*group_pad] /
    [pixels, embed] fp32 matrices over the concatenated levels `sizes` = [(H, W), ...] with B images each.
    -> conf [B,N,n_cls], loc [B,N,4], mask [B,N,mask_dim], track [B,N,embed] (normalised), centerness [B,N,1] (tanh)."""
    _dev(*small, *trk)
    K = len(small)
    L, start = _head_layout(B, K, sizes, n_cls, mask_dim, embed_dim, group_pad, small[0].shape[-1], trk[0].shape[-1])
    N = K * sum(h * w for h, w in sizes)
    for t in list(small) + list(trk):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[0] != start:
            raise StmError("head_assemble: inputs must be contiguous fp32 matrices over all level pixels")
    conf, loc, mask, track, cen = (torch.empty(B, N, n, device=small[0].device) for n in (n_cls, 4, mask_dim, embed_dim, 1))
    call("stm_head_assemble_f32", _ptr4(small), _ptr4(trk), ctypes.byref(L), _p(conf), _p(loc), _p(mask), _p(track), _p(cen), _stream())
    return conf, loc, mask, track, cen


# ---- sparse head (csrc/head_sparse.hip): control block indices as the header lists them
HEAD_CTL_RAW, HEAD_CTL_N, HEAD_CTL_FILL, HEAD_CTL_GATE_A, HEAD_CTL_GATE_B, HEAD_CTL_DENSE, HEAD_CTL_OVERFLOW, HEAD_CTL_INTS = 0, 1, 2, 3, 4, 5, 6, 8
HEAD_CTL_GATE_POS = 7
HEAD_CTL_OWN = 8      # split form: first int of the second block, the same fields over the positions with a kept prior of their own
# shapes form: segment k (the entries of kernel shape k) has its pair of blocks at HEAD_CTL_SEG * (k + 1); at the entry points the capacity counts
# the entries of ONE segment and carries the number of segments from bit 28 on
HEAD_CTL_SEG = 16
HEAD_SEG_SHIFT = 28


def head_seg_capacity(capacity, segs):
    """The capacity argument of the stm_head_* entry points: entries per segment + (segments << 28) in the shapes form, else the capacity."""
    if segs and not 0 < capacity < (1 << HEAD_SEG_SHIFT):
        raise StmError(f"sparse head: a segment of {capacity} entries")
    return capacity + (segs << HEAD_SEG_SHIFT) if segs else capacity


def conv_set_pixel_gate(ctl, index):
    """The next planar convolution launch of this thread runs only the pixel tiles below the device int ctl[index] (stm_conv_set_pixel_gate)."""
    _lib.lib().stm_conv_set_pixel_gate(ctl.data_ptr() + 4 * index)


def level_starts(B, sizes):
    """First pixel of each level on the concatenated pixel axis -- levels `sizes` = [(h, w), ...] with B images each -- and, last, the pixels of
    all levels.  The one place that lays the levels out: PlanarConv's multi-level launches, PlanarGraph.run and the head's entry points use it."""
    starts = [0]
    for h, w in sizes:
        starts.append(starts[-1] + B * h * w)
    return starts


def _level_arrays(B, sizes):
    n, starts = len(sizes), level_starts(B, sizes)
    st, hh, ww = (ctypes.c_int * 9)(*starts), (ctypes.c_int * 8)(*[h for h, _ in sizes]), (ctypes.c_int * 8)(*[w for _, w in sizes])
    return n, st, hh, ww, starts[n]


def _head_layout(B, K, sizes, n_cls, mask_dim, embed_dim, group_pad, small_ld, trk_ld):
    """HeadLayout of K kernel shapes over the concatenated levels `sizes` with B images each, and the pixels of all levels."""
    L = _lib.HeadLayout()
    L.B, L.K, L.n_levels, L.n_cls, L.mask_dim, L.embed_dim, L.group_pad = B, K, len(sizes), n_cls, mask_dim, embed_dim, group_pad
    L.small_ld, L.trk_ld = small_ld, trk_ld
    starts = level_starts(B, sizes)
    for l, (h, w) in enumerate(sizes):
        L.lvl_start[l], L.lvl_hw[l] = starts[l], h * w
    return L, starts[-1]


def _ptr4(ts):
    return (ctypes.c_void_p * 4)(*([t.data_ptr() for t in ts] + [0] * (4 - len(ts))))


def head_candidates(cls_logits, n_cls, conf_thresh, capacity, patch_pixels_a, patch_pixels_b, B, sizes, split=False, shapes=False):
    """stm_head_candidates_f32: cls_logits = per-kernel-shape [pixels, ld] fp32 class logits over the concatenated levels -> (list int32 [capacity] of
    the pixels whose rows the detection stage reads for the priors that pass generate_candidate's test, control block int32 [8]: see
    include/stmask_hip.h).  split: the pixels with a kept prior of their own in front, list[:ctl[HEAD_CTL_OWN + HEAD_CTL_N]], the pixels that are
    only another prior's centerness partner behind them; control block int32 [16], the second block over the own positions.
    shapes (with split): (pixel, kernel shape) entries instead of pixels -- list int32 [K * capacity], segment k = the entries of shape k, each
    ordered as the split list; control block int32 [16 (K + 1)], segment k's pair of blocks at HEAD_CTL_SEG * (k + 1)."""
    if shapes and not split:
        raise StmError("head_candidates: the shapes form is a form of the split form")
    if shapes:      # patch_pixels_a / _b: one pixel count per kernel shape (its window of the two tower layers), packed 8 bits each
        if len(patch_pixels_a) != len(cls_logits) or len(patch_pixels_b) != len(cls_logits) or not all(0 < v < 256 for v in list(patch_pixels_a) + list(patch_pixels_b)):
            raise StmError("head_candidates: the shapes form takes one patch pixel count per kernel shape")
        patch_pixels_a = sum(v << 8 * k for k, v in enumerate(patch_pixels_a))
        patch_pixels_b = sum(v << 8 * k for k, v in enumerate(patch_pixels_b))
    segs = len(cls_logits) if shapes else 0
    _dev(*cls_logits)
    n_px, ld = cls_logits[0].shape
    n, st, hh, ww, total = _level_arrays(B, sizes)
    for t in cls_logits:
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (n_px, ld) or n_px != total:
            raise StmError("head_candidates: inputs must be contiguous fp32 matrices over all level pixels")
    dev = cls_logits[0].device
    lst = torch.empty(capacity * max(segs, 1), dtype=torch.int32, device=dev)
    ctl = torch.empty(HEAD_CTL_SEG * (segs + 1) if segs else HEAD_CTL_INTS * (2 if split else 1), dtype=torch.int32, device=dev)
    flags = torch.empty(n_px + (2 * segs if segs else 2 if split else 0), dtype=torch.int32, device=dev)
    cap_arg = head_seg_capacity(capacity, segs)
    call("stm_head_candidates_f32", _ptr4(cls_logits), len(cls_logits), ld, n_cls, conf_thresh, -cap_arg if split else cap_arg, patch_pixels_a, patch_pixels_b, n, B, st,
         hh, ww, _p(flags), _p(lst), _p(ctl), _stream())
    return lst, ctl


def head_patch_gather(src, dst, side, capacity, B, sizes, lst, ctl, segs=0):
    """stm_head_patch_gather: side x side neighbourhoods of the listed pixels from the level maps (zeros outside a map), planes [P, S, pixels, 32] in and [P, S, capacity * side^2, 32] out.
    segs (shapes form): that many segments of `capacity` patches each, patch i of segment k at slot k * capacity + i."""
    _dev(src, dst)
    if (src.dim() != 4 or dst.dim() != 4 or src.shape[3] != 32 or src.element_size() != 2 or dst.dtype != src.dtype or not src.is_contiguous()
            or not dst.is_contiguous() or tuple(dst.shape) != (src.shape[0], src.shape[1], max(segs, 1) * capacity * side * side, 32)):
        raise StmError(f"head_patch_gather: planes {tuple(src.shape)} -> {tuple(dst.shape)} do not fit capacity {capacity}, side {side}")
    n, st, hh, ww, _ = _level_arrays(B, sizes)
    call("stm_head_patch_gather", _p(src), src.shape[2], _p(dst), side, src.shape[0], src.shape[1], head_seg_capacity(capacity, segs), n, B, st, hh, ww, _p(lst), _p(ctl),
         _stream())
    return dst


def head_patch_mask(planes, side, capacity, B, sizes, lst, ctl, segs=0):
    """stm_head_patch_mask: zero, in place, the pixels of the listed patches that lie outside their level's map (segs: as head_patch_gather)."""
    _dev(planes)
    if planes.dim() != 4 or planes.shape[3] != 32 or planes.element_size() != 2 or not planes.is_contiguous() or planes.shape[2] != max(segs, 1) * capacity * side * side:
        raise StmError(f"head_patch_mask: planes {tuple(planes.shape)} do not fit capacity {capacity}, side {side}")
    n, st, hh, ww, _ = _level_arrays(B, sizes)
    call("stm_head_patch_mask", _p(planes), side, planes.shape[0], planes.shape[1], head_seg_capacity(capacity, segs), n, B, st, hh, ww, _p(lst), _p(ctl), _stream())
    return planes


def head_assemble_sparse(cls_logits, small, trk, small_dense, trk_dense, B, sizes, n_cls, mask_dim, embed_dim, group_pad, row_mul, row_add, lst, ctl,
                         capacity, split=False, shapes=False):
    """stm_head_assemble_sparse_f32 -> (conf, loc, mask, track, centerness) as head_assemble; loc / mask / track / centerness hold values at the
    rows of the listed pixels only (every row after an overflow), the other rows are NOT written.  split (list and ctl from
    head_candidates(split=True)): mask / track at the rows of the own positions only, and their matrices are not read for the others.
    shapes (list and ctl from head_candidates(shapes=True)): small[k] / trk[k] hold one row per entry of segment k, `capacity` of them."""
    segs = len(cls_logits) if shapes else 0
    if ctl.numel() < (HEAD_CTL_SEG * (segs + 1) if segs else HEAD_CTL_INTS * (2 if split else 1)) or (shapes and not split):
        raise StmError("head_assemble_sparse: the split form reads a control block of 16 ints, the shapes form one of 16 (K + 1)")
    _dev(*cls_logits, *small, *trk, *small_dense, *trk_dense)
    K = len(cls_logits)
    L, start = _head_layout(B, K, sizes, n_cls, mask_dim, embed_dim, group_pad, small[0].shape[-1], trk[0].shape[-1])
    N = K * sum(h * w for h, w in sizes)
    for t in list(cls_logits) + list(small_dense) + list(trk_dense):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[0] != start:
            raise StmError("head_assemble_sparse: dense inputs must be contiguous fp32 matrices over all level pixels")
    for t, d in zip(list(small) + list(trk), list(small_dense) + list(trk_dense)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[0] < capacity * row_mul or t.shape[-1] != d.shape[-1]:
            raise StmError("head_assemble_sparse: patch inputs must be contiguous fp32 matrices of capacity * row_mul rows, as wide as the dense ones")
    conf, loc, mask, track, cen = (torch.empty(B, N, n, device=cls_logits[0].device) for n in (n_cls, 4, mask_dim, embed_dim, 1))
    call("stm_head_assemble_sparse_f32", _ptr4(cls_logits), cls_logits[0].shape[-1], _ptr4(small), _ptr4(trk), _ptr4(small_dense), _ptr4(trk_dense),
         ctypes.byref(L), row_mul, row_add, _p(lst), _p(ctl), -head_seg_capacity(capacity, segs) if split else capacity, _p(conf), _p(loc), _p(mask), _p(track), _p(cen), _stream())
    return conf, loc, mask, track, cen


def deform_conv_fused_supported(C, O, kernel_size, has_mask, fmt, deformable_groups=1):
    """True when stm_deform_conv_fused_planar_f32 takes this layer (one deformable group, <= 15 taps, 9 with mask, C % 64 == 0,
    O % 128 == 0, an fp16 plane format)."""
    kh, kw = _pair(kernel_size)
    g = DeformGeom(1, C, 8, 8, kh, kw, 1, 1, kh // 2, kw // 2, 1, 1, deformable_groups, 8, 8)
    return bool(_lib.lib().stm_deform_conv_fused_planar_supported(ctypes.byref(g), O, 1 if has_mask else 0, fmt))


def deform_conv_fused_tiles(B, Ho, Wo, O):
    """Workgroups stm_deform_conv_fused_planar_f32 launches for B images of Ho x Wo output pixels and O channels: tiles of 64 pixels x 256 channels
    where O is a multiple of 256 (STM_DCN_FUSED_WIDE, default on), 128 x 128 otherwise; patches chosen as csrc/dcn_fused.hip pick_patch does (fewest
    wasted tile pixels, then the squarest) -- the callers' small-grid rule."""
    wide = O % 256 == 0 and os.environ.get("STM_DCN_FUSED_WIDE", "1") != "0"
    tp, bn = (64, 256) if wide else (128, 128)
    best, bt, bper = -1.0, 1, 1 << 30
    for tw in range(4, tp + 1):
        th = tp // tw
        if th < 1:
            break
        thc, twc = min(th, Ho), min(tw, Wo)
        tiles = -(-Ho // thc) * -(-Wo // twc)
        eff = Ho * Wo / (tiles * float(tp))
        per = thc + twc
        if eff > best + 1e-9 or (eff > best - 1e-9 and per < bper):
            best, bt, bper = eff, tiles, per
    return B * bt * (O // bn)


def deform_conv_fused_planar(x_pix, B, H, W, C, om, packed, out_scale, bias, O, kernel_size=3, stride=1, padding=1, dilation=1, has_mask=True,
                             relu=False, fmt=1, out_fmt=None, out=None, out_off=0):
    """The whole deformable convolution of the planar graph as one kernel (csrc/dcn_fused.hip: sampler -> plane split -> MFMA product,
    no column buffer): dcn_v2.DCN (backbone.py:20-26,45; has_mask, bias, ReLU) or mmcv DeformConv2d as FeatureAlign uses it
    (Featurealign.py:27-31,72).  x_pix fp32 [B*H*W, ld >= C] pixel-major (unit channel stride), om fp32 [B*Ho*Wo, >= 2K (+K)] raw offsets
    (and mask logits), packed = conv_pack_weights(weight [O, C, kh, kw], tile_n=128, fmt=fmt)[0] with out_scale its second value.
    Returns / fills planes [P, O/32, N, 32] in out_fmt at pixels [out_off, out_off + B*Ho*Wo)."""
    _dev(x_pix, om, packed)
    if x_pix.dtype != torch.float32 or x_pix.dim() != 2 or x_pix.stride(1) != 1 or x_pix.shape[0] != B * H * W or x_pix.shape[1] != C:
        raise StmError(f"deform_conv_fused_planar: x must be fp32 [B*H*W, C] with unit channel stride, got {tuple(x_pix.shape)} {x_pix.stride()}")
    om = _f32c(om)
    kh, kw = _pair(kernel_size)
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    Ho, Wo = conv_out_hw(H, W, kh, kw, sh, sw, ph, pw, dh, dw)
    M, K = B * Ho * Wo, kh * kw
    if om.dim() != 2 or om.shape[0] != M or om.shape[1] < (3 if has_mask else 2) * K:
        raise StmError(f"deform_conv_fused_planar: offsets {tuple(om.shape)} do not match {M} output pixels x {(3 if has_mask else 2) * K}")
    out_fmt = fmt if out_fmt is None else out_fmt
    if out is None:
        out = _empty_planes(out_fmt, O // 32, M, x_pix.device)
        out_off = 0
    elif out.dim() != 4 or out.shape[1] * 32 != O or not out.is_contiguous() or out.shape[0] < plane_layout(out_fmt)[0]:
        raise StmError(f"deform_conv_fused_planar: planes {tuple(out.shape)} do not hold {O} channels in format {out_fmt}")
    if bias is not None:
        _dev(bias)
        bias = _f32c(bias)
    g = DeformGeom(B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, 1, Ho, Wo)
    timing = _fused_dcn_timing
    if timing is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    call("stm_deform_conv_fused_planar_f32", _p(x_pix), x_pix.stride(0), _p(om), om.shape[1], 1 if has_mask else 0, _p(packed), _p(bias), _p(out),
         out.shape[2], out_off, 0, O, 1 if relu else 0, out_scale, ctypes.byref(g), fmt, out_fmt, _stream())
    if timing is not None:
        e1.record()
        # SURVEY.md section 8(d), fused form: input once, offsets (+ mask) per output pixel, output planes, weights (as packed planes); no columns
        npl, npo = plane_layout(fmt)[0], plane_layout(out_fmt)[0]
        nbytes = 4 * B * C * H * W + 4 * (3 if has_mask else 2) * K * M + 2 * npo * O * M + 2 * npl * O * C * K
        timing.append((e0, e1, float(nbytes), 2.0 * M * O * C * K, {1: 3, 2: 1}[fmt]))
    return out


def dcn_sample_planar(x_nhwc, om, stride=1, padding=1, dilation=1, fmt=0):
    """Deformable 3x3 sampling for the planar graph: x fp32 [B,H,W,C], om fp32 [B*Ho*Wo, >=27] (raw conv_offset_mask output,
    pixel-major) -> bf16 planes [3, 9C/32, B*Ho*Wo, 32] with K index = tap*C + channel."""
    _dev(x_nhwc, om)
    x = _f32c(x_nhwc)
    om = _f32c(om)
    B, H, W, C = x.shape
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    Ho, Wo = conv_out_hw(H, W, 3, 3, sh, sw, ph, pw, dh, dw)
    M = B * Ho * Wo
    if om.shape[0] != M or om.shape[1] < 27:
        raise StmError(f"dcn_sample_planar: offset/mask matrix {tuple(om.shape)} does not match {M} output pixels x 27")
    g = DeformGeom(B, C, H, W, 3, 3, sh, sw, ph, pw, dh, dw, 1, Ho, Wo)
    out = _empty_planes(fmt, 9 * C // 32, M, x.device)
    timing = _im2col_timing
    if timing is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    call("stm_dcn_sample_planar_fmt_f32", _p(x), _p(om), om.shape[1], _p(out), M, 0, ctypes.byref(g), fmt, _stream())
    if timing is not None:
        e1.record()
        # algorithmic bytes: input once, 27 offset/mask values per output pixel, columns as planes (6 or 4 B / element)
        timing.append((e0, e1, 4 * B * C * H * W + 4 * 27 * M + 2 * plane_layout(fmt)[0] * 9 * C * M))
    return out
