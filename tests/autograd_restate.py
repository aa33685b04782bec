"""fp64 PyTorch restatements of the drop-ins' forward, differentiable by autograd: the yardsticks of the backward kernels.

They share no code with the kernels or with oracle/stm_oracle.c (the pattern of test_oracle_independent.py):
  * deformable convolution (dcn_v2 / mmcv DeformConv2d) = F.grid_sample(padding_mode="zeros", align_corners=True) on pixel coordinates, times
    the mask, then a matrix product;
  * RoIAlign (mmcv 1.x, avg) = grid_sample(padding_mode="border") on the sample coordinates, samples outside [-1, H] x [-1, W] zeroed, then the
    mean over ceil(roi / out) (or sampling_ratio) squared samples per bin;
  * correlation (kernel_size 1) = F.pad and slices.
Sample POSITIONS are formed in fp32 with the kernels' operation order (the position is an input to the arithmetic being checked, not part of
it); everything after that is fp64.
"""
import torch
import torch.nn.functional as F


def _sample_zeros(img, ys, xs):
    """img [N, C, H, W] fp64, ys / xs [N, h, w] pixel coordinates -> [N, C, h, w] bilinear samples of the zero-extended image."""
    H, W = img.shape[-2:]
    grid = torch.stack([2.0 * xs / (W - 1) - 1.0, 2.0 * ys / (H - 1) - 1.0], -1)
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def _positions(B, Ho, Wo, kh, kw, stride, padding, dilation, offset, g, K, k):
    """fp32 sample position of tap k of deformable group g, as the kernels form it: (float)(ho*sh - ph + i*dh) + dy."""
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
    i, j = divmod(k, kw)
    by = (torch.arange(Ho, dtype=torch.float32) * sh - ph + i * dh).view(1, Ho, 1)
    bx = (torch.arange(Wo, dtype=torch.float32) * sw - pw + j * dw).view(1, 1, Wo)
    dy = offset[:, g * 2 * K + 2 * k].detach().float().cpu()
    dx = offset[:, g * 2 * K + 2 * k + 1].detach().float().cpu()
    return (by + dy).double(), (bx + dx).double()


def deform_conv(x, offset, mask, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), deform_groups=1, fp32_positions=True):
    """fp64; x [B,C,H,W], offset [B, dg*2K, Ho, Wo] (dy, dx per tap), mask [B, dg*K, Ho, Wo] or None -> [B, O, Ho, Wo].
    fp32_positions: the position takes the kernels' fp32 value and the offset's gradient through position + (offset - offset.detach());
    False: positions in fp64 (for gradcheck, whose finite differences an fp32 rounding would swamp)."""
    B, C, H, W = x.shape
    O, _, kh, kw = weight.shape
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    K, Cg = kh * kw, C // deform_groups
    cols = []
    for g in range(deform_groups):
        xg = x[:, g * Cg:(g + 1) * Cg]
        taps = []
        for k in range(K):
            oy, ox = offset[:, g * 2 * K + 2 * k], offset[:, g * 2 * K + 2 * k + 1]
            if fp32_positions:
                ys, xs = _positions(B, Ho, Wo, kh, kw, stride, padding, dilation, offset, g, K, k)
                ys, xs = ys + (oy - oy.detach()), xs + (ox - ox.detach())
            else:
                i, j = divmod(k, kw)
                ys = (torch.arange(Ho, dtype=torch.float64) * sh - ph + i * dh).view(1, Ho, 1) + oy
                xs = (torch.arange(Wo, dtype=torch.float64) * sw - pw + j * dw).view(1, 1, Wo) + ox
            v = _sample_zeros(xg, ys, xs)                                   # [B, Cg, Ho, Wo]
            if mask is not None:
                v = v * mask[:, g * K + k].unsqueeze(1)
            taps.append(v)
        cols.append(torch.stack(taps, 2))                                   # [B, Cg, K, Ho, Wo]
    col = torch.cat(cols, 1).reshape(B, C * K, Ho * Wo)
    y = torch.matmul(weight.reshape(O, C * K), col).view(B, O, Ho, Wo)
    if bias is not None:
        y = y + bias.view(1, O, 1, 1)
    return y


def deform_conv_offset_magnitude(x, offset, mask, grad_out, weight, stride, padding, dilation, deform_groups=1):
    """Sum of |terms| of the offset gradient, per offset element: |m| * sum_c |g_c| * (hw (|v1| + |v3|) + lw (|v2| + |v4|)) for dy (and the
    transposed form for dx) -- each = a zero-extended bilinear sample of |x| on the rows (columns) floor(h) and floor(h) + 1.  Returns
    [B, dg*2K, Ho, Wo] fp64.  grad_cols = W^T grad_out is formed on absolute values too."""
    B, C, H, W = x.shape
    O, _, kh, kw = weight.shape
    K, Cg = kh * kw, C // deform_groups
    Ho, Wo = grad_out.shape[-2:]
    ax = x.detach().double().abs()
    gcols = torch.matmul(weight.detach().double().abs().reshape(O, C * K).t(), grad_out.detach().double().abs().reshape(B, O, Ho * Wo))
    gcols = gcols.view(B, C, K, Ho, Wo)
    out = torch.zeros(B, deform_groups * 2 * K, Ho, Wo, dtype=torch.float64)
    for g in range(deform_groups):
        for k in range(K):
            ys, xs = _positions(B, Ho, Wo, kh, kw, stride, padding, dilation, offset, g, K, k)
            inside = (ys > -1) & (ys < H) & (xs > -1) & (xs < W)
            fy, fx = torch.floor(ys), torch.floor(xs)
            xg = ax[:, g * Cg:(g + 1) * Cg]
            gy = _sample_zeros(xg, fy, xs) + _sample_zeros(xg, fy + 1, xs)
            gx = _sample_zeros(xg, ys, fx) + _sample_zeros(xg, ys, fx + 1)
            gc = gcols[:, g * Cg:(g + 1) * Cg, k]
            m = mask[:, g * K + k].detach().double().abs() if mask is not None else 1.0
            out[:, g * 2 * K + 2 * k] = (gc * gy).sum(1) * m * inside
            out[:, g * 2 * K + 2 * k + 1] = (gc * gx).sum(1) * m * inside
    return out


def _roi_positions(rois, PH, PW, spatial_scale, sampling_ratio):
    """Per RoI: (b, ys [PH*gh] fp32, xs [PW*gw] fp32, count) with the kernel's fp32 expressions (aligned=True)."""
    out = []
    f = torch.float32
    for r in rois.detach().float().cpu():
        b = int(r[0])
        sw_, sh_ = r[1] * spatial_scale - 0.5, r[2] * spatial_scale - 0.5
        ew_, eh_ = r[3] * spatial_scale - 0.5, r[4] * spatial_scale - 0.5
        rw, rh = ew_ - sw_, eh_ - sh_
        bh, bw = rh / torch.tensor(PH, dtype=f), rw / torch.tensor(PW, dtype=f)
        gh = sampling_ratio if sampling_ratio > 0 else int(torch.ceil(rh / torch.tensor(PH, dtype=f)))
        gw = sampling_ratio if sampling_ratio > 0 else int(torch.ceil(rw / torch.tensor(PW, dtype=f)))
        count = max(gh * gw, 1)
        if gh <= 0 or gw <= 0:
            out.append((b, None, None, count, gh, gw))
            continue
        py = torch.arange(PH, dtype=f).view(PH, 1)
        iy = torch.arange(gh, dtype=f).view(1, gh)
        ys = (sh_ + py * bh) + ((iy + 0.5) * bh) / torch.tensor(gh, dtype=f)
        px = torch.arange(PW, dtype=f).view(PW, 1)
        ix = torch.arange(gw, dtype=f).view(1, gw)
        xs = (sw_ + px * bw) + ((ix + 0.5) * bw) / torch.tensor(gw, dtype=f)
        out.append((b, ys.reshape(-1), xs.reshape(-1), count, gh, gw))
    return out


def roi_align(feat, rois, output_size, spatial_scale=1.0, sampling_ratio=0):
    """fp64 mmcv roi_align (avg, aligned=True): feat [B,C,H,W], rois [n,5] -> [n, C, PH, PW]."""
    PH, PW = output_size
    B, C, H, W = feat.shape
    outs = []
    for b, ys, xs, count, gh, gw in _roi_positions(rois, PH, PW, spatial_scale, sampling_ratio):
        if ys is None:
            outs.append(feat.new_zeros(C, PH, PW))
            continue
        Y = ys.double().view(-1, 1).expand(-1, xs.numel())
        X = xs.double().view(1, -1).expand(ys.numel(), -1)
        inside = ((Y >= -1) & (Y <= H) & (X >= -1) & (X <= W)).to(torch.float64)
        grid = torch.stack([2.0 * X.clamp(0, W - 1) / max(W - 1, 1) - 1.0, 2.0 * Y.clamp(0, H - 1) / max(H - 1, 1) - 1.0], -1)
        v = F.grid_sample(feat[b:b + 1], grid[None], mode="bilinear", padding_mode="border", align_corners=True)[0] * inside
        v = v.view(C, PH, gh, PW, gw).sum((2, 4)) / count
        outs.append(v)
    return torch.stack(outs) if outs else feat.new_zeros(0, C, PH, PW)


def correlation(in1, in2, patch_size, dilation_patch=1):
    """fp64 spatial_correlation_sample(kernel_size=1): [B,C,H,W] x 2 -> [B, P, P, H, W]."""
    B, C, H, W = in1.shape
    R = (patch_size // 2) * dilation_patch
    p2 = F.pad(in2, (R, R, R, R))
    rows = []
    for i in range(patch_size):
        cols = []
        for j in range(patch_size):
            dy, dx = i * dilation_patch, j * dilation_patch
            cols.append((in1 * p2[:, :, dy:dy + H, dx:dx + W]).sum(1))
        rows.append(torch.stack(cols, 1))
    return torch.stack(rows, 1)
