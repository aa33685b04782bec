"""fp64 PyTorch restatements of the drop-ins' forward, differentiable by autograd: the yardsticks of the backward kernels.

They share no code with the kernels or with oracle/stm_oracle.c (the pattern of test_oracle_independent.py):
  * deformable convolution (dcn_v2 / mmcv DeformConv2d) = F.grid_sample(padding_mode="zeros", align_corners=True) on pixel coordinates, times
    the mask, then a matrix product;
  * the same deformable convolution a second time (deform_conv_corners), as the explicit four-corner rule of DCNv2 / mmcv 1.x: floor, gather
    and an `inside` mask.  grid_sample cannot be the yardstick AT integer and border positions (its normalised grid returns x = 1 as
    0.99999..., so the one-sided derivative is taken on the other side, and at -1 it returns the neighbour's value where DCNv2 returns 0);
    autograd through the four-corner expression IS the convention there.  At fractional positions the two agree to 1e-14
    (test_autograd_cpu.py);
  * RoIAlign (mmcv 1.x, avg) = grid_sample(padding_mode="border") on the sample coordinates, samples outside [-1, H] x [-1, W] zeroed, then the
    mean over ceil(roi / out) (or sampling_ratio) squared samples per bin; aligned=False: no half-pixel shift, RoI size at least 1;
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

def _corner_values(img, ys, xs):
    """img [B, C, H, W], ys / xs [B, h, w] -> (v1, v2, v3, v4, ly, lx, inside): the values at (floor y, floor x), (floor y, floor x + 1),
    (floor y + 1, floor x), (floor y + 1, floor x + 1), a corner outside the image giving 0; l = p - floor(p) with the floor detached;
    inside = (-1 < y < H) & (-1 < x < W)."""
    B, C, H, W = img.shape
    y0, x0 = torch.floor(ys).detach(), torch.floor(xs).detach()
    flat = img.reshape(B, C, H * W)

    def corner(yi, xi):
        ok = (yi >= 0) & (yi <= H - 1) & (xi >= 0) & (xi <= W - 1)
        idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long().view(B, 1, -1).expand(-1, C, -1)
        return flat.gather(2, idx).view(B, C, *ys.shape[1:]) * ok.unsqueeze(1)

    inside = (ys > -1) & (ys < H) & (xs > -1) & (xs < W)
    return corner(y0, x0), corner(y0, x0 + 1), corner(y0 + 1, x0), corner(y0 + 1, x0 + 1), (ys - y0).unsqueeze(1), (xs - x0).unsqueeze(1), \
        inside.unsqueeze(1)


def _tap_positions(B, Ho, Wo, kh, kw, stride, padding, dilation, offset, g, K, k, fp32_positions):
    """Sample position of tap k of group g, differentiable w.r.t. the offset.  fp32_positions: the kernels' fp32 value, the gradient through
    offset - offset.detach(); otherwise fp64 throughout."""
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
    oy, ox = offset[:, g * 2 * K + 2 * k], offset[:, g * 2 * K + 2 * k + 1]
    if fp32_positions:
        ys, xs = _positions(B, Ho, Wo, kh, kw, stride, padding, dilation, offset, g, K, k)
        return ys + (oy - oy.detach()), xs + (ox - ox.detach())
    i, j = divmod(k, kw)
    return ((torch.arange(Ho, dtype=torch.float64) * sh - ph + i * dh).view(1, Ho, 1) + oy,
            (torch.arange(Wo, dtype=torch.float64) * sw - pw + j * dw).view(1, 1, Wo) + ox)


def deform_conv_corners(x, offset, mask, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), deform_groups=1,
                        fp32_positions=True):
    """deform_conv's arguments and result, by the four-corner rule: position p, floor(p) detached, l = p - floor(p), the four corner values
    gathered (0 outside the image), the sample times (-1 < y < H) & (-1 < x < W), then mask, matrix product, bias.  Autograd through this
    is DCNv2's convention at integer and border positions: the derivative is the right-sided one (h_low = floor(h) also at integer h), and
    value and derivative are 0 at and beyond -1 and H / W."""
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
            ys, xs = _tap_positions(B, Ho, Wo, kh, kw, stride, padding, dilation, offset, g, K, k, fp32_positions)
            v1, v2, v3, v4, ly, lx, inside = _corner_values(xg, ys, xs)
            v = ((1 - ly) * (1 - lx) * v1 + (1 - ly) * lx * v2 + ly * (1 - lx) * v3 + ly * lx * v4) * inside
            if mask is not None:
                v = v * mask[:, g * K + k].unsqueeze(1)
            taps.append(v)
        cols.append(torch.stack(taps, 2))                                   # [B, Cg, K, Ho, Wo]
    col = torch.cat(cols, 1).reshape(B, C * K, Ho * Wo)
    y = torch.matmul(weight.reshape(O, C * K), col).view(B, O, Ho, Wo)
    if bias is not None:
        y = y + bias.view(1, O, 1, 1)
    return y


def deform_conv_corners_offset_magnitude(x, offset, mask, grad_out, weight, stride, padding, dilation, deform_groups=1):
    """deform_conv_offset_magnitude from the four-corner gathers (no grid_sample on an integer row): per offset element
    |m| * sum_c |g_c| * ((1 - lx) (|v1| + |v3|) + lx (|v2| + |v4|)) for dy, |m| * sum_c |g_c| * ((1 - ly) (|v1| + |v2|) + ly (|v3| + |v4|)) for dx,
    0 where the sample is not inside.  Returns [B, dg*2K, Ho, Wo] fp64."""
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
            v1, v2, v3, v4, ly, lx, inside = _corner_values(ax[:, g * Cg:(g + 1) * Cg], ys, xs)
            gc = gcols[:, g * Cg:(g + 1) * Cg, k]
            m = mask[:, g * K + k].detach().double().abs() if mask is not None else 1.0
            out[:, g * 2 * K + 2 * k] = (gc * ((1 - lx) * (v1 + v3) + lx * (v2 + v4)) * inside).sum(1) * m
            out[:, g * 2 * K + 2 * k + 1] = (gc * ((1 - ly) * (v1 + v2) + ly * (v3 + v4)) * inside).sum(1) * m
    return out


def _roi_positions(rois, PH, PW, spatial_scale, sampling_ratio, aligned=True):
    """Per RoI: (b, ys [PH*gh] fp32, xs [PW*gw] fp32, count) with the kernel's fp32 expressions.  aligned=False (mmcv 1.x): no half-pixel
    shift, and the RoI's width and height are at least 1."""
    out = []
    f = torch.float32
    shift = 0.5 if aligned else 0.0
    for r in rois.detach().float().cpu():
        b = int(r[0])
        sw_, sh_ = r[1] * spatial_scale - shift, r[2] * spatial_scale - shift
        ew_, eh_ = r[3] * spatial_scale - shift, r[4] * spatial_scale - shift
        rw, rh = ew_ - sw_, eh_ - sh_
        if not aligned:
            rw, rh = torch.clamp(rw, min=1.0), torch.clamp(rh, min=1.0)
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


def roi_align(feat, rois, output_size, spatial_scale=1.0, sampling_ratio=0, aligned=True):
    """fp64 mmcv roi_align (avg): feat [B,C,H,W], rois [n,5] -> [n, C, PH, PW]."""
    PH, PW = output_size
    B, C, H, W = feat.shape
    outs = []
    for b, ys, xs, count, gh, gw in _roi_positions(rois, PH, PW, spatial_scale, sampling_ratio, aligned):
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


# ---- inputs on the lattice of integer, border and half-integer positions ------------------------------------------------------------------
LATTICE_CLASSES = ("integer inside", "0", "H-1", "-1", "H", "just inside -1", "just inside H", "half-integer", "far outside")


def _bases(kh, kw, Ho, Wo, stride, padding, dilation):
    """Integer base positions (before the offset) as fp32 [K, Ho, 1] and [K, 1, Wo]."""
    K = kh * kw
    by = (torch.arange(Ho) * stride[0] - padding[0]).view(1, Ho, 1) + (torch.arange(K) // kw * dilation[0]).view(K, 1, 1)
    bx = (torch.arange(Wo) * stride[1] - padding[1]).view(1, 1, Wo) + (torch.arange(K) % kw * dilation[1]).view(K, 1, 1)
    return by.float(), bx.float()


def lattice_offsets(B, dg, kh, kw, H, W, stride, padding, dilation, gen):
    """fp32 offsets [B, dg*2K, Ho, Wo] that put each axis of each sample on a position drawn from LATTICE_CLASSES.  The neighbour just inside -1
    (-1 + 2^-24) is only reachable exactly from a base of -1 or 0 (a larger base needs an offset fp32 cannot hold), so the samples with such a
    base take it with probability 0.4 and all others draw from the remaining classes uniformly."""
    K = kh * kw
    Ho = (H + 2 * padding[0] - (dilation[0] * (kh - 1) + 1)) // stride[0] + 1
    Wo = (W + 2 * padding[1] - (dilation[1] * (kw - 1) + 1)) // stride[1] + 1
    by, bx = _bases(kh, kw, Ho, Wo, stride, padding, dilation)
    off = torch.zeros(B, dg, K, 2, Ho, Wo)
    shape = (B, dg, K, Ho, Wo)
    for axis, base, size in ((0, by.expand(K, Ho, Wo), H), (1, bx.expand(K, Ho, Wo), W)):
        cls = torch.randint(0, 8, shape, generator=gen)
        n = torch.randint(0, 4, shape, generator=gen).float()
        inner = torch.randint(1, max(size - 1, 2), shape, generator=gen).float()
        half = torch.randint(-1, size, shape, generator=gen).float() + 0.5
        far = torch.where(torch.rand(shape, generator=gen) < 0.5, -3.5 - n, size + 2.25 + n)
        below_size = torch.nextafter(torch.tensor(float(size)), torch.tensor(0.0))
        above_m1 = torch.nextafter(torch.tensor(-1.0), torch.tensor(0.0))
        target = torch.stack([inner, torch.zeros(shape), torch.full(shape, size - 1.0), torch.full(shape, -1.0), torch.full(shape, float(size)),
                              below_size.expand(shape), half, far]).gather(0, cls[None])[0]
        near_m1 = ((base == -1) | (base == 0)).expand(shape) & (torch.rand(shape, generator=gen) < 0.4)
        target = torch.where(near_m1, above_m1.expand(shape), target)
        off[:, :, :, axis] = target - base
    return off.reshape(B, dg * 2 * K, Ho, Wo)


def position_classes(off, dg, kh, kw, H, W, stride, padding, dilation):
    """The fp32 sample positions of `off` as the kernels form them, and per axis the share of samples in each of LATTICE_CLASSES.  Asserts that
    base + offset is exact in fp32, so that an fp64 yardstick samples at the very same point."""
    B, _, Ho, Wo = off.shape
    K = kh * kw
    by, bx = _bases(kh, kw, Ho, Wo, stride, padding, dilation)
    o = off.view(B, dg, K, 2, Ho, Wo)
    shares = []
    for axis, base, size in ((0, by, H), (1, bx, W)):
        d = o[:, :, :, axis]
        p = base + d
        assert torch.equal(p.double(), base.double() + d.double()), "base + offset is not exact in fp32"
        below_size = torch.nextafter(torch.tensor(float(size)), torch.tensor(0.0))
        above_m1 = torch.nextafter(torch.tensor(-1.0), torch.tensor(0.0))
        is_int = p == torch.round(p)
        member = {"integer inside": is_int & (p > 0) & (p < size - 1), "0": p == 0, "H-1": p == size - 1, "-1": p == -1, "H": p == size,
                  "just inside -1": p == above_m1, "just inside H": p == below_size,
                  "half-integer": (p * 2 == torch.round(p * 2)) & ~is_int & (p > -1) & (p < size), "far outside": (p < -2) | (p > size + 1)}
        shares.append({k: v.float().mean().item() for k, v in member.items()})
    return shares
