"""Exact model of the one-plane fp16 arithmetic (planar format 2, BASELINE config 5's backbone) for the kernel tests.

A format-2 kernel rounds each operand to fp16 with round-to-nearest-even and multiplies the rounded values exactly in fp32:
  activations  x~ = RN16(x)                  (split_planes(fmt=2), or the previous layer's epilogue),
  weights      w~ = RN16(w * s) / s          (s = 2 ** (10 - floor(log2 max|w|)), the power of two of ops.conv_pack_weights;
                                              one s is shared where several tensors are packed as one product),
  DCN columns  RN16(fp32 bilinear sample * mask),
then sums the exact products in fp32, takes s out again and adds bias / residual in fp32.  Against an fp64 evaluation of
the ROUNDED operands (conv_q, dcn_cols_q) the result must therefore sit at fp32 accumulation distance,
|y - model| <= 2e-6 * mag with mag = conv(|x~|, |w~|) + |b| + |r|, whereas the unrounded fp64 oracle is up to ~2^-10 of mag
away.  fp16 subnormals (|v| < 2^-14) are KEPT by the model: RN16 is torch's / numpy's conversion, which rounds to the
subnormal grid of 2^-24 and flushes only below 2^-25.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14
F16_MIN_SUBNORMAL = 2.0 ** -24


def q16(x):
    """RN16 and back, subnormals kept.  fp32 (and narrower) tensors round once through torch's half(); fp64 tensors round
    directly from fp64 through numpy (torch converts fp64 -> fp32 -> fp16, a double rounding)."""
    if x.dtype == torch.float64:
        return torch.from_numpy(x.detach().cpu().numpy().astype(np.float16).astype(np.float64)).to(x.device)
    return x.half().to(x.dtype)


def pow2_wscale(weight):
    """The power-of-two weight scale of ops.conv_pack_weights / ops._pow2_wscale, 2 ** (10 - floor(log2 max|w|)), computed
    with frexp (exact at the powers of two where floor(log2) steps): max|w * s| lies in [1024, 2048)."""
    wmax = float(weight.detach().abs().max())
    if wmax == 0.0:
        return 1.0
    _, e = math.frexp(wmax)          # wmax = m * 2^e, 0.5 <= m < 1: floor(log2 wmax) = e - 1
    return 2.0 ** (11 - e)


def wq(w, scale=None):
    """The weights a format-2 kernel multiplies by: RN16(w * s) / s in fp32 (s = pow2_wscale(w) unless given: pass the
    scale of the concatenation where several tensors are packed under one scale)."""
    s = pow2_wscale(w) if scale is None else float(scale)
    w = w.detach().float()
    return q16(w * s) / s


def _patches(x, kh, kw, stride, pad):
    """x [B, H, W, C] -> patches [B, Ho, Wo, kh * kw * C] (tap-major, channel minor) with zero padding."""
    (sh, sw), (ph, pw) = _pair(stride), _pair(pad)
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, pw, pw, ph, ph))
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    cols = [xp[:, ky:ky + sh * (Ho - 1) + 1:sh, kx:kx + sw * (Wo - 1) + 1:sw, :] for ky in range(kh) for kx in range(kw)]
    return torch.cat(cols, -1), Ho, Wo


def _row_patches(x, kh, kw, stride, pad, rows):
    """The patches of the flat output pixels `rows` only: [len(rows), kh * kw * C], same order as _patches."""
    (sh, sw), (ph, pw) = _pair(stride), _pair(pad)
    B, H, W, C = x.shape
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    xp = F.pad(x, (0, 0, pw, pw, ph, ph))
    b, rem = rows // (Ho * Wo), rows % (Ho * Wo)
    oy, ox = rem // Wo, rem % Wo
    ky = torch.arange(kh, device=x.device).repeat_interleave(kw)
    kx = torch.arange(kw, device=x.device).repeat(kh)
    iy = oy[:, None] * sh + ky[None, :]
    ix = ox[:, None] * sw + kx[None, :]
    return xp[b[:, None], iy, ix].reshape(len(rows), kh * kw * C)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def conv_q(xq, wqt, b=None, r=None, stride=1, pad=0, relu=False, rows=None):
    """fp64 convolution of ROUNDED operands: xq [B, H, W, C] (fp16-exact values), wqt [O, C, kh, kw] (= wq(w)), bias [O],
    residual [B, Ho, Wo, O] -> (y, mag) as fp64 [B, Ho, Wo, O], mag = conv(|xq|, |wqt|) + |b| + |r| (before the ReLU).
    rows: optional LongTensor of flat output pixels (b * Ho * Wo + oy * Wo + ox): then y, mag are [len(rows), O].
    Runs on the device of xq (fp64 matmuls over gathered patches)."""
    O, C, kh, kw = wqt.shape
    dev = xq.device
    x = xq.double()
    wm = wqt.double().to(dev).permute(0, 2, 3, 1).reshape(O, kh * kw * C).t()
    if rows is None:
        P, Ho, Wo = _patches(x, kh, kw, stride, pad)
        P = P.reshape(-1, kh * kw * C)
    else:
        P = _row_patches(x, kh, kw, stride, pad, rows.to(dev))
    y, mag = P @ wm, P.abs() @ wm.abs()
    if b is not None:
        bd = b.double().to(dev)
        y, mag = y + bd, mag + bd.abs()
    if r is not None:
        rd = r.double().to(dev).reshape(-1, O)
        if rows is not None:
            rd = rd[rows.to(dev)]
        y, mag = y + rd, mag + rd.abs()
    if relu:
        y = y.clamp_min(0)
    if rows is None:
        y, mag = y.view(x.shape[0], Ho, Wo, O), mag.view(x.shape[0], Ho, Wo, O)
    return y, mag


def midpoint_distance16(v):
    """fp64 tensor -> distance of every value to the nearest rounding midpoint of the fp16 grid (the points where RN16
    changes its result), as fp64."""
    a = v.detach().cpu().numpy().astype(np.float64)
    h = a.astype(np.float16)
    up = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    hd = h.astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.minimum(np.abs(a - (hd + up) / 2), np.abs(a - (hd + dn) / 2))
    return torch.from_numpy(np.nan_to_num(d, nan=np.inf)).to(v.device)


def dcn_cols_q(x, off, mask_logit, kh, kw, stride=1, pad=1, dilation=1, rel_amb=2.0 ** -20, rows=None):
    """Modulated deformable sampling in fp64 on the conventions of the kernels (and oracle.deform_conv / mmcv): x [B, H, W, C],
    off [B, Ho, Wo, 2K] as (dy, dx) per tap (positions formed in fp32), mask_logit [B, Ho, Wo, K] or None (no mask) -> (cols, amb, smag):
      cols [B * Ho * Wo, K * C] fp64: RN16 of the fp64 value  sum_corners w_corner * x_corner * sigmoid(logit)  (tap-major,
           the column order of the sampler's planes and of the fused kernel's K loop);
      amb  bool, same shape: the fp64 value lies within rel_amb * smag of an fp16 rounding midpoint, where smag =
           sum |w_corner * x_corner * mask| -- the kernel samples in fp32 (fp32 sigmoid, fp32 corner weights, fmas), so there
           it may legitimately round to the other neighbour (one fp16 ulp away);
      smag the fp64 magnitudes (unrounded).
    A sample whose position is outside (-1, H) x (-1, W) is 0; corners outside the image count 0.
    rows: optional LongTensor of flat output pixels: then the three are [len(rows), K * C]."""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(pad), _pair(dilation)
    B, H, W, C = x.shape
    Ho, Wo = off.shape[1], off.shape[2]
    K = kh * kw
    if rows is None:
        rows = torch.arange(B * Ho * Wo)
    rows = rows.cpu()
    b, rem = rows // (Ho * Wo), rows % (Ho * Wo)
    oy, ox = (rem // Wo)[:, None], (rem % Wo)[:, None]
    xd = x.double().cpu()
    offf = off.float().cpu().reshape(B * Ho * Wo, K, 2)[rows]
    if mask_logit is not None:
        mk = torch.sigmoid(mask_logit.double().cpu().reshape(B * Ho * Wo, K)[rows])
    else:
        mk = torch.ones(len(rows), K, dtype=torch.float64)
    ky = (torch.arange(K) // kw)[None, :]
    kx = (torch.arange(K) % kw)[None, :]
    # the sampling position is formed in fp32 (integer base + fp32 offset), as the kernels and the oracle form it
    fy = ((oy * sh - ph + ky * dh).float() + offf[..., 0]).double()
    fx = ((ox * sw - pw + kx * dw).float() + offf[..., 1]).double()
    inside = (fy > -1) & (fx > -1) & (fy < H) & (fx < W)
    y0, x0 = torch.floor(fy), torch.floor(fx)
    ly, lx = fy - y0, fx - x0
    y0, x0 = y0.long(), x0.long()
    val = torch.zeros(len(rows), K, C, dtype=torch.float64)
    smag = torch.zeros_like(val)
    bi = b[:, None]
    for cy, cx, wgt in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx), (y0 + 1, x0, ly * (1 - lx)), (y0 + 1, x0 + 1, ly * lx)):
        ok = inside & (cy >= 0) & (cy < H) & (cx >= 0) & (cx < W)
        g = xd[bi, cy.clamp(0, H - 1), cx.clamp(0, W - 1)]                          # [R, K, C]
        t = g * (wgt * mk * ok).unsqueeze(-1)
        val += t
        smag += t.abs()
    val, smag = val.reshape(len(rows), K * C), smag.reshape(len(rows), K * C)
    amb = midpoint_distance16(val) <= rel_amb * smag
    return q16(val), amb, smag
