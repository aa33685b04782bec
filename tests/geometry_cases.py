"""Geometries with UNEQUAL stride / padding / dilation pairs for the drop-in ops, shared by test_geometry_cpu.py and test_gpu_geometry.py.

Every deformable kernel form works out `ho*sh - ph + i*dh` and `wo*sw - pw + j*dw` for itself, and the tiled launchers size their LDS rows and halo
from sh / dh / ph.  A form that took sh where sw belongs passes any test whose pairs are equal; the cases here have sh != sw, dh != dw and
ph != pw (also with square kernels), padding 0 and padding above "same", kernels from 1x1 to 7x7, H != W, one-row and one-column outputs.

  * DEFORM_TABLE: the fixed table.  `route` says what the automatic dispatch of stm_deform_im2col_f32 does with the case (asserted on the CPU against
    a restatement of the rule, so that the table cannot drift away from what it claims to cover).
  * DEFORM_DRAWS: 40 more geometries drawn with a fixed seed from the argument space stm_validate_deform_geom accepts.
  * deform_inputs(case): x, offsets, mask, weight, bias, grad_out.  Offsets are Gaussian (scale 2) with a share of the samples steered, per axis,
    into the (-1, 0) band, the (H-1, H) band and outside the map; every third case mixes in autograd_restate.lattice_offsets (integer, border and
    half-integer positions).  position_shares() counts the four classes the way the kernels form a position (fp32 base + offset).
  * PLANAR_CASES / FUSED_CASES: the shapes the planar samplers and the fused kernel are built for (C in {128, 256, 512}; C % 64, O % 128).
  * roi_cases() / ROI_*: RoIs over three images, rows not sorted by image; CORR_CASES: correlation patches 1 .. 21, dilations 1 .. 3.
"""
import torch

import autograd_restate as R


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def out_hw(c):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = c["k"], c["st"], c["pad"], c["dl"]
    return (c["H"] + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (c["W"] + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def case_id(c):
    return "{name}".format(**c)


def _case(B, C, O, H, W, k, st, pad, dl, dg, route, note):
    name = "k{}x{} s{}{} p{}{} d{}{} dg{} {}x{}x{}x{} {}".format(*k, *st, *pad, *dl, dg, B, C, H, W, note).strip().replace(" ", "_")
    return dict(B=B, C=C, O=O, H=H, W=W, k=k, st=st, pad=pad, dl=dl, dg=dg, route=route, name=name)


# route: what variant 0 (automatic) picks -- "direct" (C/dg % 4 != 0), "v3" (deform_im2col.hip: Cg % 32 == 0 and HWo*K >= 3840*9), "v3s2" (the
# stride-2 rule: Cg % 32 == 0, sh == 2, HWo >= 960) or "v2"
DEFORM_TABLE = [
    #     B   C   O   H    W    k       stride  padding dilation dg
    _case(2, 8, 12, 11, 14, (3, 3), (1, 2), (0, 3), (2, 1), 1, "v2", "sh_lt_sw dh_gt_dw pad0 overpad"), # Ho*Wo = 7*9 = 63
    _case(2, 8, 8, 13, 16, (3, 5), (2, 1), (2, 0), (1, 3), 2, "v2", "sh_gt_sw dh_lt_dw"),               # 8*4 = 32 (% 4 == 0)
    _case(2, 8, 8, 6, 10, (1, 1), (2, 1), (0, 1), (1, 1), 1, "v2", "one tap"),                          # 3*12
    _case(2, 8, 12, 12, 15, (5, 3), (2, 3), (1, 4), (2, 2), 1, "v2", ""),                               # 3*7 = 21
    _case(2, 16, 8, 7, 12, (1, 3), (1, 1), (1, 0), (1, 2), 4, "v2", "dg4"),                             # 9*8
    _case(1, 8, 8, 9, 12, (7, 7), (1, 1), (3, 2), (1, 1), 1, "v2", "ph_ne_pw"),                         # 9*10
    _case(2, 8, 8, 14, 9, (3, 1), (2, 1), (3, 0), (3, 1), 1, "v2", "one column"),                       # 7*9
    _case(2, 8, 8, 10, 12, (3, 3), (1, 1), (2, 0), (1, 1), 1, "v2", "square ph_ne_pw"),                 # 12*10 (% 4 == 0)
    _case(2, 6, 8, 10, 12, (3, 3), (2, 1), (1, 1), (1, 2), 1, "direct", "C_mod4_ne_0"),                 # 5*10
    _case(2, 8, 8, 5, 12, (5, 3), (1, 2), (0, 1), (1, 1), 1, "v2", "Ho1"),                              # 1*6
    _case(2, 8, 8, 12, 5, (3, 3), (2, 1), (1, 0), (1, 2), 1, "v2", "Wo1"),                              # 6*1
    _case(1, 32, 32, 48, 160, (3, 3), (1, 2), (1, 2), (1, 2), 1, "v3", "variant3"),                     # 48*80 = 3840
    _case(1, 32, 32, 64, 40, (3, 3), (2, 1), (1, 1), (1, 1), 1, "v3s2", "stride-2 rule"),               # 32*40 = 1280
    _case(2, 8, 8, 8, 11, (5, 3), (1, 1), (4, 3), (1, 2), 2, "v2", "overpad dg2"),                      # 12*13
    _case(2, 16, 12, 9, 20, (3, 5), (1, 3), (1, 2), (2, 1), 2, "v2", ""),                               # 7*7 = 49
    _case(3, 12, 8, 15, 7, (3, 3), (3, 1), (0, 0), (1, 3), 1, "v2", "pad0 both"),                       # 5*1
]
for _i, _c in enumerate(DEFORM_TABLE):
    _c.update(seed=1000 + _i, lattice=_i % 3 == 0)


def _draws(n, seed):
    """n geometries from the accepted argument space (kernel, stride, dilation > 0, padding >= 0, C % dg == 0, Ho, Wo >= 1), small maps, H != W."""
    g = _gen(seed)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=g))

    kernels = [(1, 1), (1, 3), (3, 1), (3, 3), (3, 5), (5, 3), (7, 7), (2, 3), (5, 5)]
    out = []
    while len(out) < n:
        k = kernels[ri(0, len(kernels) - 1)]
        st, dl, pad = (ri(1, 3), ri(1, 3)), (ri(1, 3), ri(1, 3)), (ri(0, 4), ri(0, 4))
        dg = (1, 2, 4)[ri(0, 2)]
        C = dg * (2, 4, 6, 8)[ri(0, 3)]
        if k == (1, 1):
            dl = (1, 1)                                 # one tap: the dilation forms no position, a swapped pair could not be told
        c = _case(ri(1, 3), C, (4, 8, 12)[ri(0, 2)], ri(4, 18), ri(4, 18), k, st, pad, dl, dg, None, "draw%d" % len(out))
        Ho, Wo = out_hw(c)
        if c["H"] == c["W"] or Ho < 1 or Wo < 1 or Ho * Wo < 2 or Ho * Wo > 400:
            continue
        c.update(seed=2000 + len(out), lattice=len(out) % 3 == 0)
        out.append(c)
    return out


DEFORM_DRAWS = _draws(40, seed=20260)
DEFORM_CASES = DEFORM_TABLE + DEFORM_DRAWS


def auto_route(c):
    """The dispatch rule of stm_deform_im2col_f32 for variant 0, restated (deform_im2col.hip, `if (variant == 0)`)."""
    Ho, Wo = out_hw(c)
    K, Cg, HWo = c["k"][0] * c["k"][1], c["C"] // c["dg"], Ho * Wo
    if Cg % 4:
        return "direct"
    if Cg % 32 == 0 and HWo * K >= 3840 * 9:
        return "v3"
    if Cg % 32 == 0 and c["st"][0] == 2 and HWo >= 960:
        return "v3s2"
    return "v2"


def _bases(c):
    """fp32 integer base positions [K, Ho, 1] and [K, 1, Wo]: ho*sh - ph + i*dh and wo*sw - pw + j*dw."""
    Ho, Wo = out_hw(c)
    return R._bases(c["k"][0], c["k"][1], Ho, Wo, c["st"], c["pad"], c["dl"])


def steered_offsets(c, gen, scale=2.0, share=0.36):
    """Gaussian offsets [B, dg*2K, Ho, Wo]; per axis, `share` of the samples is moved in equal parts into (-1, 0), into (size-1, size) and outside
    the map (half of those below -1, half above size)."""
    B, dg, (kh, kw) = c["B"], c["dg"], c["k"]
    K = kh * kw
    Ho, Wo = out_hw(c)
    off = torch.randn(B, dg, K, 2, Ho, Wo, generator=gen) * scale
    by, bx = _bases(c)
    shape = (B, dg, K, Ho, Wo)
    for axis, base, size in ((0, by.expand(K, Ho, Wo), c["H"]), (1, bx.expand(K, Ho, Wo), c["W"])):
        u = torch.rand(shape, generator=gen)
        f = 0.02 + 0.96 * torch.rand(shape, generator=gen)
        far = 0.3 + 3.0 * torch.rand(shape, generator=gen)
        which = torch.randint(0, 6, shape, generator=gen)                 # 0, 1: low band; 2, 3: high band; 4: below -1; 5: above size
        target = torch.stack([-1.0 + f, -1.0 + f, size - 1.0 + f, size - 1.0 + f, -1.0 - far, size + far]).gather(0, which[None])[0]
        off[:, :, :, axis] = torch.where(u < share, target - base, off[:, :, :, axis])
    return off.reshape(B, dg * 2 * K, Ho, Wo)


def offsets(c, gen):
    off = steered_offsets(c, gen)
    if c["lattice"]:
        lat = R.lattice_offsets(c["B"], c["dg"], c["k"][0], c["k"][1], c["H"], c["W"], c["st"], c["pad"], c["dl"], gen)
        off = torch.where(torch.rand(off.shape, generator=gen) < 0.5, lat, off)
    return off


def position_shares(c, off):
    """Per axis, the share of (pixel, tap) samples whose fp32 position base + offset is inside [0, size-1], in (-1, 0), in (size-1, size), outside."""
    B, dg, K = c["B"], c["dg"], c["k"][0] * c["k"][1]
    Ho, Wo = out_hw(c)
    o = off.view(B, dg, K, 2, Ho, Wo)
    by, bx = _bases(c)
    shares = []
    for axis, base, size in ((0, by, c["H"]), (1, bx, c["W"])):
        p = base + o[:, :, :, axis]                                       # fp32, the kernels' own operation
        cls = {"inside": (p >= 0) & (p <= size - 1), "low band": (p > -1) & (p < 0), "high band": (p > size - 1) & (p < size),
               "outside": (p <= -1) | (p >= size)}
        assert sum(v.sum().item() for v in cls.values()) == p.numel()
        shares.append({k: v.float().mean().item() for k, v in cls.items()})
    return shares


def deform_inputs(c, with_mask=True, with_bias=True):
    """-> x, offset, mask (values in (0, 1)) or None, weight, bias or None, grad_out; all fp32 on the CPU."""
    g = _gen(c["seed"])
    B, C, O, (kh, kw), dg = c["B"], c["C"], c["O"], c["k"], c["dg"]
    Ho, Wo = out_hw(c)
    off = offsets(c, g)
    x = torch.randn(B, C, c["H"], c["W"], generator=g)
    mask = torch.rand(B, dg * kh * kw, Ho, Wo, generator=g)
    w = torch.randn(O, C, kh, kw, generator=g) / (C * kh * kw) ** 0.5
    b = torch.randn(O, generator=g)
    go = torch.randn(B, O, Ho, Wo, generator=g)
    return x, off, mask if with_mask else None, w, b if with_bias else None, go


def transposed(c, which):
    """The case with one pair swapped (which in "st", "pad", "dl"): what a kernel that took the other axis' value would compute."""
    d = dict(c)
    d[which] = (c[which][1], c[which][0])
    return d


def unequal_pairs(c):
    return [w for w in ("st", "pad", "dl") if c[w][0] != c[w][1]]


def columns_fp64(c, x, off, mask, positions=None):
    """fp64 deformable columns [B, C*K, Ho*Wo] on c's output grid by the four-corner rule (autograd_restate's own pieces).  positions: the case whose
    stride / padding / dilation form the sample positions (default c itself) -- with transposed(c, ...) the model of a kernel that read the other
    axis' value while everything else (output grid, tensor sizes) stayed as the caller gave it."""
    p = positions or c
    B, C, dg, (kh, kw) = c["B"], c["C"], c["dg"], c["k"]
    K, Cg = kh * kw, C // dg
    Ho, Wo = out_hw(c)
    x = x.double()
    groups = []
    for g in range(dg):
        taps = []
        for k in range(K):
            ys, xs = R._tap_positions(B, Ho, Wo, kh, kw, p["st"], p["pad"], p["dl"], off, g, K, k, True)
            v1, v2, v3, v4, ly, lx, inside = R._corner_values(x[:, g * Cg:(g + 1) * Cg], ys, xs)
            v = ((1 - ly) * (1 - lx) * v1 + (1 - ly) * lx * v2 + ly * (1 - lx) * v3 + ly * lx * v4) * inside
            if mask is not None:
                v = v * mask[:, g * K + k].double().unsqueeze(1)
            taps.append(v)
        groups.append(torch.stack(taps, 2))
    return torch.cat(groups, 1).reshape(B, C * K, Ho * Wo)


# ---- planar samplers: 3x3 with mask (dcn_sample_planar), C in {128, 256, 512}.  lds: the STM_DCN_LDS=1 launcher takes the case (dh == dw == 1 and
# sh == sw in {1, 2}) or must decline it
PLANAR_CASES = [
    dict(B=2, C=128, H=9, W=13, st=(1, 2), pad=(0, 2), dl=(2, 1), lds=False),
    dict(B=1, C=256, H=11, W=8, st=(2, 1), pad=(2, 0), dl=(1, 3), lds=False),
    dict(B=2, C=512, H=7, W=10, st=(2, 2), pad=(0, 1), dl=(1, 1), lds=True),
    dict(B=2, C=128, H=10, W=21, st=(1, 1), pad=(2, 0), dl=(1, 1), lds=True),
    dict(B=1, C=256, H=12, W=9, st=(2, 3), pad=(1, 1), dl=(1, 1), lds=False),
    dict(B=2, C=128, H=8, W=12, st=(3, 3), pad=(1, 2), dl=(1, 1), lds=False),
    dict(B=1, C=256, H=20, W=14, st=(2, 2), pad=(3, 1), dl=(2, 2), lds=False),
    dict(B=2, C=512, H=9, W=7, st=(2, 1), pad=(1, 0), dl=(1, 2), lds=False),
    dict(B=1, C=256, H=9, W=37, st=(2, 2), pad=(2, 3), dl=(1, 1), lds=True),
]
for _c in PLANAR_CASES:
    _c.update(k=(3, 3), name="C{C} {B}x{H}x{W} s{st[0]}{st[1]} p{pad[0]}{pad[1]} d{dl[0]}{dl[1]}".format(**_c).replace(" ", "_"))
    assert _c["lds"] == (_c["dl"] == (1, 1) and _c["st"][0] == _c["st"][1] and _c["st"][0] in (1, 2))

# ---- the mask-free planar sampler (deform_sample_planar: stride 1, dilation 1, C = 256, H x W outputs) with padding ABOVE "same": it then computes
# the first H x W outputs of the (H + 2 ph - kh + 1) x (W + 2 pw - kw + 1) the deformable convolution has
SAMPLE_PLANAR_CASES = [dict(k=(3, 3), pad=(2, 1)), dict(k=(3, 3), pad=(1, 3)), dict(k=(3, 5), pad=(1, 3)), dict(k=(5, 3), pad=(4, 1)),
                       dict(k=(3, 5), pad=(2, 2))]

# ---- fused deformable convolution: one group, C % 64 == 0, O % 128 == 0, <= 15 taps (9 with mask)
FUSED_CASES = [
    dict(B=2, C=64, H=9, W=13, O=128, k=(3, 3), st=(1, 2), pad=(0, 2), dl=(2, 1), mask=True),
    dict(B=1, C=128, H=11, W=8, O=256, k=(3, 3), st=(2, 1), pad=(2, 0), dl=(1, 3), mask=True),
    dict(B=2, C=64, H=7, W=10, O=256, k=(3, 5), st=(1, 1), pad=(2, 1), dl=(1, 2), mask=False),
    dict(B=1, C=64, H=12, W=9, O=128, k=(5, 3), st=(2, 3), pad=(1, 2), dl=(1, 1), mask=False),
    dict(B=2, C=64, H=8, W=12, O=128, k=(1, 3), st=(1, 2), pad=(1, 0), dl=(1, 2), mask=False),
    dict(B=2, C=128, H=10, W=6, O=256, k=(3, 1), st=(2, 1), pad=(0, 0), dl=(3, 1), mask=False),
    dict(B=1, C=64, H=14, W=23, O=128, k=(3, 3), st=(3, 2), pad=(3, 0), dl=(1, 1), mask=True),
]
for _i, _c in enumerate(FUSED_CASES):
    _c.update(dg=1, seed=3000 + _i, lattice=False,
              name="k{k[0]}x{k[1]} C{C} O{O} {B}x{H}x{W} s{st[0]}{st[1]} p{pad[0]}{pad[1]} d{dl[0]}{dl[1]}".format(**_c).replace(" ", "_"))


# ---- RoIAlign: three images, every batch index used, rows not sorted by image; boxes at most 1.8 maps wide or high (the adaptive grid loops over
# ceil(extent / bins) samples), overhanging each border; one empty RoI, one below a pixel
ROI_B, ROI_H, ROI_W = 3, 20, 28
ROI_SCALES, ROI_OUTS, ROI_CHANNELS = (0.25, 0.5, 1.0, 2.0), ((7, 7), (3, 5), (1, 1), (14, 2)), (1, 3, 40, 256)


def rois(scale, seed=77):
    """[n, 5] = (image, x1, y1, x2, y2) in input coordinates: map coordinates / spatial_scale."""
    g = _gen(seed)
    H, W = float(ROI_H), float(ROI_W)
    r = []
    for i in range(10):
        x1, y1 = (torch.rand(2, generator=g) * torch.tensor([W, H]) * 0.8).tolist()
        w, h = (torch.rand(2, generator=g) * torch.tensor([W, H]) * 0.6 + 0.5).tolist()
        r.append([(2 * i + 1) % 3, x1, y1, x1 + w, y1 + h])
    r += [[2, -0.35 * W, 0.2 * H, 0.3 * W, 0.6 * H],            # over the left border
          [0, 0.3 * W, -0.4 * H, 0.7 * W, 0.5 * H],             # top
          [1, 0.6 * W, 0.1 * H, 1.4 * W, 0.9 * H],              # right
          [2, 0.2 * W, 0.7 * H, 0.5 * W, 1.45 * H],             # bottom
          [0, -0.4 * W, -0.4 * H, 1.4 * W, 1.4 * H],            # all four, 1.8 maps each way
          [1, 5.0, 6.0, 5.0, 6.0],                              # empty
          [2, 3.0, 2.0, 3.25, 2.5],                             # below a pixel
          [1, W - 0.5, H - 0.5, W + 3.0, H + 2.0]]              # almost all of it outside
    t = torch.tensor(r, dtype=torch.float32)
    t[:, 1:] /= scale
    return t


def roi_cases():
    """One case per (spatial_scale, output size); sampling_ratio 0 .. 4 and aligned cycle with periods 5 and 2 (all ten pairs appear), the channel
    counts with a shift per row of the table."""
    out = []
    for i in range(16):
        c = dict(scale=ROI_SCALES[i % 4], out=ROI_OUTS[i // 4], sr=i % 5, aligned=i % 2 == 0, C=ROI_CHANNELS[(i + i // 4) % 4])
        c["name"] = "scale{scale} {out[0]}x{out[1]} sr{sr} aligned={aligned} C{C}".format(**c).replace(" ", "_")
        out.append(c)
    return out


# ---- correlation: patch sizes 1 .. 21, patch dilations 1 .. 3, B >= 2, W % 4 and C % 4 zero and non-zero
CORR_CASES = [dict(B=2, C=8, H=9, W=12, P=1, dil=1), dict(B=2, C=9, H=7, W=14, P=1, dil=2), dict(B=2, C=6, H=7, W=13, P=3, dil=2),
              dict(B=2, C=8, H=8, W=8, P=3, dil=3), dict(B=2, C=3, H=5, W=9, P=9, dil=1), dict(B=2, C=5, H=10, W=16, P=9, dil=3),
              dict(B=3, C=12, H=8, W=11, P=13, dil=1), dict(B=2, C=16, H=9, W=12, P=13, dil=3), dict(B=2, C=4, H=12, W=20, P=21, dil=2),
              dict(B=2, C=7, H=6, W=10, P=21, dil=3), dict(B=2, C=8, H=6, W=12, P=21, dil=1), dict(B=2, C=5, H=7, W=9, P=13, dil=2)]
for _c in CORR_CASES:
    _c["name"] = "B{B} C{C} {H}x{W} P{P} dil{dil}".format(**_c).replace(" ", "_")
