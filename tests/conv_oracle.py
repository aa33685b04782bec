"""Helpers shared by tests/test_gpu_conv.py and tests/test_gpu_conv_rows.py: seeded inputs, the fp64 oracle of a (multi-level, grouped) planar
convolution per (level, group), and the CPU restatement of format 0's three-product mode."""
import torch

import oracle
from fp16_model import _patches
from stmask_amd import ops

DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def level_group_oracle(xs, sizes, B, wts, bias, pad, relu, C, groups, cg, real, res=None):
    """[(rows, columns, ref, mag)] of oracle.conv2d_nhwc per (level, group): xs[l] = [B, h, w, groups * C] fp32, group g reads its own C channels and
    writes columns [g * cg, g * cg + real[g]); res: fp32 residual [pixels of all levels, groups * cg] or None.  mag = sum |x w| + |bias| + |res|."""
    starts = [0]
    for h, w in sizes:
        starts.append(starts[-1] + B * h * w)
    out = []
    for l, (h, w) in enumerate(sizes):
        for g in range(groups):
            rows, cols = slice(starts[l], starts[l + 1]), slice(g * cg, g * cg + real[g])
            xg = xs[l][..., g * C:(g + 1) * C].contiguous()
            wg, bg = wts[cols], (bias[cols] if bias is not None else None)
            rg = res[rows, cols].reshape(B, h, w, real[g]).contiguous() if res is not None else None
            ref = oracle.conv2d_nhwc(xg, wg, bg, rg, padding=pad, relu=relu)
            mag = oracle.conv2d_nhwc(xg.abs(), wg.abs(), bg.abs() if bg is not None else None, rg.abs() if rg is not None else None, padding=pad)
            out.append((rows, cols, ref, mag))
    return out


def worst_ratio(y32, refs):
    """max |y - ref| / max(mag, 1e-6) of an fp32 output [pixels, channels] (CPU) over the (level, group) references of level_group_oracle."""
    worst = 0.0
    for rows, cols, ref, mag in refs:
        worst = max(worst, ((y32[rows, cols].reshape(ref.shape) - ref).abs() / mag.clamp_min(1e-6)).max().item())
    return worst


def planar_conv_vs_oracle(conv, xs, sizes, B, wts, bias, pad, relu, C, groups, cg, real, fmt, tol, refs=None):
    """Run `conv` over the concatenated levels and compare every (level, group) with the fp64 oracle (refs: level_group_oracle of the same
    arguments, where the caller has it already)."""
    flat = torch.cat([x.reshape(-1, x.shape[-1]) for x in xs], 0)
    xp = ops.split_planes(flat.to(DEV), fmt)
    shape = ("levels", B, sizes) if len(sizes) > 1 else ("img", B, *sizes[0])
    y32, ypl = conv(xp, shape, out="both")
    y32, ypl = y32.cpu(), ypl.cpu()
    if refs is None:
        refs = level_group_oracle(xs, sizes, B, wts, bias, pad, relu, C, groups, cg, real)
    worst = worst_ratio(y32, refs)
    assert worst < tol, worst
    return y32, ypl, worst


# ---- format 0 with planes = 2: the three-product mode -------------------------------------------------------------------------------------
BF16_U = 2.0 ** -9          # unit roundoff of bf16: 8 significand bits, round to nearest


def bf16_split2(v):
    """p0 = RN_bf16(v), p1 = RN_bf16(v - p0) as fp32 tensors (v - p0 is exact in fp32: it has at most 16 significant bits)."""
    v = v.float()
    p0 = v.bfloat16().float()
    p1 = (v - p0).bfloat16().float()
    return p0, p1


def three_product_model(x, w, stride, pad):
    """sum (p0 q0 + p0 q1 + p1 q0) in fp64 over the taps and channels of the convolution: x [B, H, W, C], w [O, C, kh, kw] -> [B, Ho, Wo, O].
    No bias, no residual, no ReLU: the caller adds them in fp64."""
    O, C, kh, kw = w.shape
    (p0, p1), (q0, q1) = bf16_split2(x), bf16_split2(w)
    mat = lambda q: q.double().permute(0, 2, 3, 1).reshape(O, kh * kw * C).t()
    P0, Ho, Wo = _patches(p0.double(), kh, kw, stride, pad)
    P1, _, _ = _patches(p1.double(), kh, kw, stride, pad)
    y = P0.reshape(-1, kh * kw * C) @ (mat(q0) + mat(q1)) + P1.reshape(-1, kh * kw * C) @ mat(q0)
    return y.view(x.shape[0], Ho, Wo, O)


# |x w - (p0 q0 + p0 q1 + p1 q0)| <= THREE_PRODUCT_REL |x w|: derived in the docstring of test_case_vs_oracle (tests/test_gpu_conv_rows.py)
THREE_PRODUCT_REL = 3 * BF16_U ** 2 * (1 + BF16_U)
