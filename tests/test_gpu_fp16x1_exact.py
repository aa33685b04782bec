"""The fp16x1 (planar format 2, BASELINE config 5's backbone) kernels held to their exact arithmetic (tests/fp16_model.py).

A format-2 kernel multiplies RN16-rounded activations by RN16(w * s) / s weights exactly and sums in fp32, so against an fp64
evaluation of those ROUNDED operands it must sit at fp32 accumulation distance:
    |y - model| <= 2e-6 * mag + 2^-24 |y|,   mag = conv(|x~|, |w~|) + |b| + |r|
(the 2^-24 |y|: the epilogue's fp32 addition of bias / residual).  Every test also keeps a LOWER bound against the unrounded
fp64 oracle, so it really measures the one-plane arithmetic.  The weight images are read back exactly (one-hot inputs), which
pins the rounding mode and the scale independently of any accumulation bound.  Subnormals: split_planes(fmt=2), the epilogues
and the weight packs keep fp16 subnormals (RN16 onto the 2^-24 grid), and the MFMAs multiply them exactly -- the model states it
and the tests check it at 1e-6-scale activations and with weights under 2^-24 / s.

The worst ratio |y - model| / mag of each kernel family is printed (pytest -s): "WORST <family> <value>".
"""
import numpy as np
import pytest
import torch

import oracle
from fp16_model import conv_q, dcn_cols_q, pow2_wscale, q16, wq
from stmask_amd import ops
from stmask_amd.planar import PlanarConv
from test_gpu_conv import CONV_CASES, KXR_CASES
from test_gpu_dcn_fused import FUSED_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-6


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def dec(planes):
    return ops.planes_to_f32(planes.cpu() if planes.is_cuda else planes)


def report(family, worst):
    print(f"WORST {family} {worst:.3e}")


def check_model(y, model, mag, what, lower=None):
    """|y - model| <= 2e-6 mag + 2^-24 |y| (fp64 model); returns the worst |y - model| / mag.  lower = (oracle, oracle_mag): the
    unrounded fp64 result must be FURTHER away somewhere than fp32 arithmetic could explain (it is the one-plane arithmetic)."""
    y = y.double().to(model.device).reshape(model.shape)
    mag = mag.reshape(model.shape)
    err = (y - model).abs()
    bad = ~(err <= TOL * mag + 2.0 ** -24 * y.abs())           # (a non-finite output is outside too)
    worst = (err / mag.clamp_min(1e-30)).max().item()
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} outside the model bound; worst |y - model| / mag = {worst:.3e}"
    if lower is not None:
        ref, rmag = lower
        far = ((y.cpu() - ref.double().cpu().reshape(y.shape)).abs() / rmag.double().cpu().reshape(y.shape).clamp_min(1e-30)).max().item()
        assert far > 1e-5, f"{what}: only {far:.2e} from the unrounded oracle -- not the one-plane arithmetic"
    return worst


def conv_model(x, w, b, r, s, pad, relu, scale=None, res_rounded=False):
    """conv_q of the rounded operands, on the device."""
    return conv_q(q16(x).to(DEV), wq(w, scale).to(DEV), b, (q16(r) if res_rounded else r) if r is not None else None, s, pad, relu)


# ------------------------------------------------------------------------------------------------ the general planar kernel
@pytest.mark.parametrize("tile_n", [64, 128])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_fmt2_against_the_exact_model(case, tile_n):
    """conv2d_planar fmt 2 on every CONV_CASE: fp32 output and residual, residual as one-plane planes (modelled RN16-rounded),
    vector (Cout % 8 == 0) and scalar epilogues, planes out = RN16 of the fp32 output, out_fmt 1 = both planes of it."""
    B, H, W, C, O, kh, kw, s, pad, has_bias, has_res, relu = case
    x = rnd(B, H, W, C, seed=0)
    w = rnd(O, C, kh, kw, seed=1, scale=(C * kh * kw) ** -0.5)
    b = rnd(O, seed=2) if has_bias else None
    Ho, Wo = ops.conv_out_hw(H, W, kh, kw, s, s, pad[0], pad[1], 1, 1)
    r = rnd(B, Ho, Wo, O, seed=3) if has_res else None
    ref = oracle.conv2d_nhwc(x, w, b, r, stride=s, padding=pad, relu=relu)
    rmag = oracle.conv2d_nhwc(x.abs(), w.abs(), b.abs() if has_bias else None, r.abs() if has_res else None, stride=s, padding=pad)
    bd = b.to(DEV) if has_bias else None
    xp = ops.split_planes(x.to(DEV), fmt=2)
    assert torch.equal(dec(xp), q16(x.view(-1, C)))
    conv = PlanarConv(w.to(DEV), bd, s, pad, relu=relu, tile_n=tile_n, fmt=2)
    conv.kxr = False
    y32, ypl = conv(xp, ("img", B, H, W), out="both", residual=r.view(-1, O).to(DEV) if has_res else None)
    assert conv.out_scale == 1.0 / pow2_wscale(w)
    model, mag = conv_model(x, w, b, r, s, pad, relu)
    worst = check_model(y32, model, mag, f"fmt2 {case} tile {tile_n}", lower=(ref, rmag))
    assert torch.equal(dec(ypl)[:, :O], q16(y32.cpu()))
    conv2 = PlanarConv(w.to(DEV), bd, s, pad, relu=relu, tile_n=tile_n, fmt=2, out_fmt=1)
    conv2.kxr = False
    z32, zpl = conv2(xp, ("img", B, H, W), out="both", residual=r.view(-1, O).to(DEV) if has_res else None)
    assert torch.equal(z32, y32)
    zb = dec(zpl)[:, :O]
    assert ((zb - z32.cpu()).abs() <= 2.0 ** -21 * z32.cpu().abs() + 1.5e-11).all()
    if has_res:
        y3 = conv(xp, ("img", B, H, W), out="f32", residual=ops.split_planes(r.to(DEV), fmt=2))
        model3, mag3 = conv_model(x, w, b, r, s, pad, relu, res_rounded=True)
        worst = max(worst, check_model(y3, model3, mag3, f"fmt2 {case} planar residual"))
    report("conv2d_planar", worst)


@pytest.mark.parametrize("tile_n", [64, 128])
def test_conv_fmt2_loop_variants_and_split_k_against_the_model(tile_n, tunables):
    """Every K-loop variant (three-buffer ring, two-buffer loop, the 64-wide ring forced) and split-K (fp32 partial sums + finishing
    kernel, vector and scalar finish) meet the exact model, not only each other."""
    worst = 0.0
    for (B, H, W, C, O, k) in [(2, 24, 40, 64, 128, 3), (8, 48, 80, 128, 256, 3), (1, 12, 20, 512, 64, 1), (2, 6, 10, 1024, 128, 3),
                               (1, 5, 7, 512, 41, 1)]:
        x = rnd(B, H, W, C, seed=C + k)
        w = rnd(O, C, k, k, seed=O, scale=(C * k * k) ** -0.5)
        b = rnd(O, seed=7)
        r = rnd(B * H * W, O, seed=8)
        conv = PlanarConv(w.to(DEV), b.to(DEV), 1, k // 2, relu=True, tile_n=tile_n, fmt=2)
        conv.kxr = False
        xp = ops.split_planes(x.to(DEV), fmt=2)
        model, mag = conv_model(x, w, b, r.view(B, H, W, O), 1, k // 2, True)
        for name, env in [("ring", {}), ("two-buffer", {"STM_CONV_RING": "2", "STM_CONV_RING64": "2"}), ("ring64", {"STM_CONV_RING64": "4"}),
                          ("splitk3", {"STM_CONV_SPLITK": "3"}), ("splitk5", {"STM_CONV_SPLITK": "5"})]:
            tunables.set(**env)
            y32, ypl = conv(xp, ("img", B, H, W), out="both", residual=r.to(DEV))
            tunables.clear(*env)
            worst = max(worst, check_model(y32, model, mag, f"{name} {(B, H, W, C, O, k)} tile {tile_n}"))
            assert torch.equal(dec(ypl)[:, :O], q16(y32.cpu())), name
    report("conv2d_planar loop variants / split-K", worst)


# ------------------------------------------------------------------------------------------------ weight images read back exactly
def spread_weights(O, C, kh, kw, seed, top=0.125):
    """Weights whose largest magnitude is an exact power of two (`top`: the floor(log2) boundary of the scale formula), with a
    sprinkling of tiny values that land on fp16's subnormal grid (or under it) after the scale, and values at odd ties."""
    w = rnd(O, C, kh, kw, seed=seed, scale=top / 6).clamp(-0.9 * top, 0.9 * top)
    flat = w.view(-1)
    n = flat.numel()
    g = torch.Generator().manual_seed(seed + 1)
    idx = torch.randperm(n, generator=g)
    k = max(8, n // 20)
    flat[idx[:k]] *= 2.0 ** -torch.randint(14, 34, (k,), generator=g).float()      # w s from ~2^-4 down to under 2^-25: subnormals and zeros
    flat[idx[k]] = top
    flat[idx[k + 1]] = -top * 0.75
    return w


def onehot_input(C, kh, kw, ph, pw, B=1):
    """One 1.0 per input channel c, at pixels spaced kh x kw apart: output (py + ph - ky, px + pw - kx) of that pixel holds
    w~[:, c, ky, kx] alone.  Returns (x [B, H, W, C], positions [(b, py, px)] per channel)."""
    per = -(-C // B)
    nx = -(-per // 8)
    H, W = 8 * kh, nx * kw
    x = torch.zeros(B, H, W, C)
    pos = []
    for c in range(C):
        b, i = c // per, c % per
        py, px = (kh - 1 - ph) + (i // nx) * kh, (kw - 1 - pw) + (i % nx) * kw
        x[b, py, px, c] = 1.0
        pos.append((b, py, px))
    return x, pos


def read_back(y, pos, O, kh, kw, ph, pw):
    """y [B, H, W, >= O] of a one-hot launch -> w~ [O, C, kh, kw]."""
    back = torch.empty(O, len(pos), kh, kw)
    for c, (b, py, px) in enumerate(pos):
        blk = y[b, py + ph - kh + 1:py + ph + 1, px + pw - kw + 1:px + pw + 1, :O]      # [kh, kw, O], rows oy = py + ph - ky
        back[:, c] = blk.flip(0, 1).permute(2, 0, 1)
    return back


@pytest.mark.parametrize("tile_n", [64, 128])
@pytest.mark.parametrize("shape", [(64, 32, 3, 3, 1, 1), (41, 64, 5, 3, 2, 1), (130, 32, 1, 1, 0, 0), (256, 96, 3, 5, 1, 2)])
def test_weight_pack_fmt2_reads_back_exactly(shape, tile_n):
    """The general fmt-2 pack (ops.conv_pack_weights) holds exactly RN16(w s) / s: subnormal products kept, RNE ties, the scale of
    the power-of-two boundary."""
    O, C, kh, kw, ph, pw = shape
    w = spread_weights(O, C, kh, kw, seed=O + C)
    x, pos = onehot_input(C, kh, kw, ph, pw)
    conv = PlanarConv(w.to(DEV), None, 1, (ph, pw), relu=False, tile_n=tile_n, fmt=2)
    conv.kxr = False
    B, H, W, _ = x.shape
    y = conv(ops.split_planes(x.to(DEV), fmt=2), ("img", B, H, W), out="f32").cpu().view(B, H, W, O)
    want = wq(w)
    assert (want != 0).any() and ((want.abs() < 2.0 ** -14 / pow2_wscale(w)) & (want != 0)).any()    # subnormal products are present
    got = read_back(y, pos, O, kh, kw, ph, pw)
    assert torch.equal(got, want), f"{int((got != want).sum())} weights differ"


def test_weight_pack_kxr_fmt2_reads_back_exactly():
    """The kx-reuse kernel's own pack (ops.conv_pack_weights_kxr): one scale over all groups."""
    for (O, C, kh, kw, G, real) in [(48, 32, 3, 3, 1, [41]), (192, 64, 3, 5, 3, [41, 5, 32])]:
        cg = O // G
        w = spread_weights(O, C, kh, kw, seed=O + kh)
        for g_ in range(G):
            w[g_ * cg + real[g_]:(g_ + 1) * cg] = 0.0
        ph, pw = (kh - 1) // 2, (kw - 1) // 2
        x1, pos = onehot_input(C, kh, kw, ph, pw)
        x = x1.repeat(1, 1, 1, G)                                  # every group reads the same one-hot pattern in its own channels
        B, H, W, _ = x.shape
        conv = PlanarConv(w.to(DEV), None, 1, (ph, pw), relu=False, groups=G, group_cout=real, tile_n=64, fmt=2)
        conv.kxr = ops.conv_kxr_supported(O, C, kh, kw, 1, (ph, pw), G, real, 2)
        conv.kxr_min_pixels = 0
        assert conv.kxr
        y = conv(ops.split_planes(x.to(DEV), fmt=2), ("img", B, H, W), out="f32").cpu().view(B, H, W, O)
        assert "kxr" in conv._packed
        want = wq(w)
        for g_ in range(G):
            got = read_back(y[..., g_ * cg:g_ * cg + real[g_]], pos, real[g_], kh, kw, ph, pw)
            assert torch.equal(got, want[g_ * cg:g_ * cg + real[g_]]), (O, g_, int((got != want[g_ * cg:g_ * cg + real[g_]]).sum()))


def test_weight_pack_dual_fmt2_reads_back_under_the_shared_scale():
    """conv3 + projection shortcut as one product, W = [W3 | Wds]: ONE scale, that of the concatenation -- here Wds holds the
    largest weight, so W3's tiny weights round on the subnormal grid of the shared scale, not of their own."""
    P, Cin, O, s = 64, 128, 256, 2
    w3 = spread_weights(O, P, 1, 1, seed=5, top=2.0 ** -6)
    wd = spread_weights(O, Cin, 1, 1, seed=6, top=0.5)
    wcat = torch.cat([w3, wd], 1)
    assert pow2_wscale(wcat) != pow2_wscale(w3) and not torch.equal(wq(w3, pow2_wscale(wcat)), wq(w3))
    Ho, Wo = 12, 16                                  # 192 output pixels: one-hots of mid at pixels 0..63, of x at 64..191
    mid = torch.zeros(1, Ho, Wo, P)
    x = torch.zeros(1, 2 * Ho, 2 * Wo, Cin)
    for c in range(P):
        mid[0, c // Wo, c % Wo, c] = 1.0
    for c in range(Cin):
        p = P + c
        x[0, s * (p // Wo), s * (p % Wo), c] = 1.0
    conv = PlanarConv(wcat.to(DEV), None, 1, 0, relu=False, fmt=2, tile_n=128)
    y = conv(ops.split_planes(mid.to(DEV), fmt=2), ("img", 1, Ho, Wo), out="f32", x2=(ops.split_planes(x.to(DEV), fmt=2), 2 * Ho, 2 * Wo, s)).cpu()
    got = y[:P + Cin].t().reshape(O, P + Cin, 1, 1)
    want = wq(wcat)
    assert torch.equal(got, want), f"{int((got != want).sum())} weights differ"
    assert torch.count_nonzero(y[P + Cin:]) == 0


# ------------------------------------------------------------------------------------------------ dual source, kx-reuse, stem
@pytest.mark.parametrize("case", [(2, 24, 40, 64, 64, 256, 1, 64), (2, 25, 39, 128, 256, 512, 2, 64), (1, 12, 20, 256, 512, 1024, 2, 128),
                                  (3, 6, 10, 512, 1024, 2048, 2, 128)])
def test_conv_dual_fmt2_against_the_model(case):
    """relu([W3 | Wds] [mid ; x[::s, ::s]] + b3 + bds) against the model of the concatenated product under the concatenation's scale."""
    B, H2, W2, P, Cin, O, s, tile_n = case
    Ho, Wo = (H2 - 1) // s + 1, (W2 - 1) // s + 1
    mid, x = rnd(B, Ho, Wo, P, seed=90), rnd(B, H2, W2, Cin, seed=91)
    w3, wd = rnd(O, P, 1, 1, seed=92, scale=P ** -0.5), rnd(O, Cin, 1, 1, seed=93, scale=Cin ** -0.5)
    b = rnd(O, seed=94) + rnd(O, seed=95)
    xs = x[:, ::s, ::s].contiguous()
    wcat = torch.cat([w3, wd], 1)
    conv = PlanarConv(wcat.to(DEV), b.to(DEV), 1, 0, relu=True, fmt=2, tile_n=tile_n)
    y32, ypl = conv(ops.split_planes(mid.to(DEV), fmt=2), ("img", B, Ho, Wo), out="both", x2=(ops.split_planes(x.to(DEV), fmt=2), H2, W2, s))
    cat = torch.cat([mid, xs], -1)
    model, mag = conv_model(cat, wcat, b, None, 1, 0, True)
    ref = oracle.conv2d_nhwc(cat, wcat, b, None, relu=True)
    rmag = oracle.conv2d_nhwc(cat.abs(), wcat.abs(), b.abs(), None)
    worst = check_model(y32, model, mag, f"dual {case}", lower=(ref, rmag))
    assert torch.equal(dec(ypl)[:, :O], q16(y32.cpu()))
    report("conv2d_planar_dual", worst)


@pytest.mark.parametrize("case", KXR_CASES)
def test_conv_kxr_fmt2_against_the_model(case):
    """The kx-reuse kernel (multi-level pixel axes, grouped layers) against the model, per level and group."""
    kh, kw, G, cg, real, sizes, B, relu = case
    C = 64
    xs = [rnd(B, h, w, G * C, seed=40 + i) for i, (h, w) in enumerate(sizes)]
    wts = rnd(G * cg, C, kh, kw, seed=50, scale=(C * kh * kw) ** -0.5)
    for g in range(G):
        wts[g * cg + real[g]:(g + 1) * cg] = 0.0
    bias = rnd(G * cg, seed=51)
    pad = ((kh - 1) // 2, (kw - 1) // 2)
    conv = PlanarConv(wts.to(DEV), bias.to(DEV), 1, pad, relu=relu, groups=G, group_cout=list(real), tile_n=64, fmt=2)
    conv.kxr = ops.conv_kxr_supported(G * cg, C, kh, kw, 1, pad, G, list(real), 2)
    conv.kxr_min_pixels = 0
    assert conv.kxr
    flat = torch.cat([x.reshape(-1, x.shape[-1]) for x in xs], 0)
    shape = ("levels", B, sizes) if len(sizes) > 1 else ("img", B, *sizes[0])
    y32, ypl = conv(ops.split_planes(flat.to(DEV), 2), shape, out="both")
    y32 = y32.cpu()
    s_all = pow2_wscale(wts)
    worst, start = 0.0, 0
    for l, (h, w) in enumerate(sizes):
        n = B * h * w
        for g in range(G):
            xg = xs[l][..., g * C:(g + 1) * C].contiguous()
            wg, bg = wts[g * cg:g * cg + real[g]], bias[g * cg:g * cg + real[g]]
            model, mag = conv_model(xg, wg, bg, None, 1, pad, relu, scale=s_all)
            out = y32[start:start + n, g * cg:g * cg + real[g]]
            worst = max(worst, check_model(out, model, mag, f"kxr {case} level {l} group {g}"))
            assert torch.equal(dec(ypl)[start:start + n, g * cg:g * cg + real[g]], q16(out))
        start += n
    report("conv2d_planar_kxr", worst)


@pytest.mark.parametrize("hw", [(64, 96), (37, 53), (384, 640)])
def test_stem_fused_fmt2_against_the_model(hw):
    """stm_stem_fused_f32 fmt 2.  What it rounds (csrc/stem_fused.hip): the frame's RGB values to RN16 as they enter LDS (plane h
    only), the weights to RN16(w s) (stem_pack_kernel); products in the MFMA, fp32 sums, * 1 / s, 3x3 / 2 max-pool of those fp32
    values (padding -inf), then + bias and ReLU in fp32 and RN16 at the store.  Model: max-pool of conv_q(RN16(x), w~), + b, ReLU.
    out_fmt 1 gives the fp32 value to 22 bits (checked against the model); the one-plane output is plane 0 of it = RN16(value)."""
    H, W = hw
    B = 2 if H < 300 else 1
    x = rnd(B, H, W, 3, seed=70)
    w = rnd(64, 3, 7, 7, seed=71, scale=147 ** -0.5)
    b = rnd(64, seed=72)
    packed, osc = ops.stem_pack_weights(w.to(DEV), 2)
    assert osc == 1.0 / pow2_wscale(w)
    p1, (Hp, Wp) = ops.stem_fused(x.to(DEV), packed, osc, b.to(DEV), 2)
    p2, _ = ops.stem_fused(x.to(DEV), packed, osc, b.to(DEV), 2, out_fmt=1)
    assert p1.shape[0] == 1 and p2.shape[0] == 2
    y = dec(p2).view(B, Hp, Wp, 64)
    pre, pmag = conv_q(q16(x).to(DEV), wq(w).to(DEV), None, None, 2, 3, False)
    pool = torch.nn.functional.max_pool2d(pre.permute(0, 3, 1, 2), 3, 2, 1)
    magp = torch.nn.functional.max_pool2d(pmag.permute(0, 3, 1, 2), 3, 2, 1)
    model = (pool + b.double().to(DEV).view(1, 64, 1, 1)).clamp_min(0).permute(0, 2, 3, 1)
    mag = (magp + b.abs().double().to(DEV).view(1, 64, 1, 1)).permute(0, 2, 3, 1)
    # (22 bits of the fp32 value: + 2^-21 |y|)
    err = (y.double().to(DEV) - model).abs()
    assert (err <= TOL * mag + 2.0 ** -21 * y.double().to(DEV).abs()).all(), (err / mag).max().item()
    worst = (err / mag).max().item()
    assert torch.equal(dec(p1), dec(p2[0:1]))
    assert ((dec(p1) - dec(p2)).abs() <= 0.5 * ulp16(dec(p1)).float()).all()          # h = RN16 of the value
    xd, wd = x.permute(0, 3, 1, 2).double(), w.double()
    ref = torch.nn.functional.max_pool2d(torch.relu(torch.nn.functional.conv2d(xd, wd, b.double(), stride=2, padding=3)), 3, 2, 1).permute(0, 2, 3, 1)
    assert (y.double() - ref).abs().max().item() > 1e-4 * ref.abs().max().item()      # the rounded frame, not the fp32 one
    report("stem_fused", worst)


# ------------------------------------------------------------------------------------------------ deformable convolution
def _om(B, Ho, Wo, K, off_scale, has_mask, seed):
    off = rnd(B, Ho, Wo, 2 * K, seed=seed, scale=off_scale)
    logit = rnd(B, Ho, Wo, K, seed=seed + 1) if has_mask else None
    om = torch.cat([off, logit], -1) if has_mask else off
    return off, logit, om.reshape(B * Ho * Wo, -1).contiguous()


def ulp16(v):
    a = np.abs(v.detach().cpu().numpy()).astype(np.float16)
    return torch.from_numpy(np.spacing(a).astype(np.float64))


@pytest.mark.parametrize("case", [c for c in FUSED_CASES if c[10] and c[5:7] == (3, 3)] + [(2, 64, 10, 14, 128, 3, 3, 1, (1, 1), 40.0, True, True)])
def test_dcn_sample_fmt2_columns_are_rn16_of_the_fp64_samples(case):
    """dcn_sample_planar(fmt=2): every column value equals RN16 of the fp64 sample * mask, except samples within 2^-20 of their
    magnitude from an fp16 rounding midpoint (fp32 sampling may round those the other way): at most one fp16 ulp off, and few."""
    B, C, H, W, O, kh, kw, s, pad, off_scale, has_mask, relu = case
    C = max(C, 128)                                              # (the planar sampler takes 128, 256 or 512 channels)
    Ho, Wo = ops.conv_out_hw(H, W, 3, 3, s, s, pad[0], pad[1], 1, 1)
    x = rnd(B, H, W, C, seed=11)
    off, logit, om = _om(B, Ho, Wo, 9, off_scale, True, seed=12)
    cols = dec(ops.dcn_sample_planar(x.to(DEV), om.to(DEV), s, pad, 1, fmt=2)).double()
    want, amb, _ = dcn_cols_q(x, off, logit, 3, 3, s, pad, 1)
    diff = cols != want
    assert not (diff & ~amb).any(), f"{int((diff & ~amb).sum())} samples differ from RN16 of the fp64 sample"
    assert ((cols - want).abs() <= ulp16(want) * amb).all()
    assert amb.float().mean().item() < 2e-2 and diff.float().mean().item() < 1e-2
    if off_scale > 10:
        assert (want == 0).float().mean().item() > 0.2                  # many samples fall outside the image


@pytest.mark.parametrize("wide", ["1", "0"])
@pytest.mark.parametrize("case", FUSED_CASES + [(2, 64, 10, 14, 256, 3, 3, 1, (1, 1), 40.0, True, True)])
def test_dcn_fused_fmt2_against_the_model(case, wide, tunables):
    """deform_conv_fused_planar fmt 2 against the fp64 GEMM of dcn_cols_q x w~: 2e-6 mag plus, for every ambiguous sample, one fp16
    ulp times |w~|.  Both tile widths (STM_DCN_FUSED_WIDE), offsets far outside the image, no-mask FCB shapes."""
    B, C, H, W, O, kh, kw, s, pad, off_scale, has_mask, relu = case
    K = kh * kw
    Ho, Wo = ops.conv_out_hw(H, W, kh, kw, s, s, pad[0], pad[1], 1, 1)
    x = rnd(B, H, W, C, seed=21)
    off, logit, om = _om(B, Ho, Wo, K, off_scale, has_mask, seed=22)
    w = rnd(O, C, kh, kw, seed=23, scale=(C * K) ** -0.5)
    bias = rnd(O, seed=24) if has_mask else None
    tunables.set(STM_DCN_FUSED_WIDE=wide)
    packed, osc = ops.conv_pack_weights(w.to(DEV), tile_n=128, fmt=2)
    args = (x.reshape(-1, C).contiguous().to(DEV), B, H, W, C, om.to(DEV), packed, osc, None if bias is None else bias.to(DEV), O, (kh, kw), s, pad, 1)
    p2 = ops.deform_conv_fused_planar(*args, has_mask=has_mask, relu=relu, fmt=2, out_fmt=1)
    p1 = ops.deform_conv_fused_planar(*args, has_mask=has_mask, relu=relu, fmt=2)
    tunables.clear("STM_DCN_FUSED_WIDE")
    y = dec(p2).double()
    cols, amb, _ = dcn_cols_q(x, off, logit, kh, kw, s, pad, 1)
    wk = wq(w).permute(0, 2, 3, 1).reshape(O, K * C).double().t().to(DEV)
    cols, amb = cols.to(DEV), amb.to(DEV)
    model = cols @ wk
    mag = cols.abs() @ wk.abs()
    slack = (ulp16(cols).to(DEV) * amb) @ wk.abs()
    if bias is not None:
        model, mag = model + bias.double().to(DEV), mag + bias.abs().double().to(DEV)
    if relu:
        model = model.clamp_min(0)
    err = (y.to(DEV) - model).abs()
    assert (err <= TOL * mag + slack + 2.0 ** -21 * y.to(DEV).abs()).all(), f"{case}: {(err / mag).max().item():.3e}"
    clean = slack == 0
    worst = (err / mag)[clean].max().item() if clean.any() else 0.0
    assert torch.equal(dec(p1), dec(p2[0:1])) and ((dec(p1) - dec(p2)).abs() <= 0.5 * ulp16(dec(p1)).float()).all()
    report("deform_conv_fused_planar (samples off midpoints)", worst)


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("scale", [1e-6, 3e-5, 3e4])
def test_conv_fmt2_subnormal_and_large_activations(scale, tunables):
    """Activations at 1e-6 (fp16 subnormals: split_planes(fmt=2) keeps them on the 2^-24 grid and the MFMAs multiply them exactly), at
    the normal / subnormal border and near 3e4 (fp32 output only: those outputs leave fp16's range).  Split and unsplit K, both tile
    widths; the planes written at the small scales are RN16 of the fp32 output, subnormals included (split and epilogue agree)."""
    B, H, W, C, O = 2, 9, 12, 64, 96
    x = rnd(B, H, W, C, seed=20).clamp(-2, 2) * scale                 # (3e4: up to 6e4, inside fp16's range)
    w = rnd(O, C, 3, 3, seed=21, scale=(C * 9) ** -0.5 * (1e-2 if scale > 1 else 1.0))
    flag = ops.planar_range_flag()
    flag.zero_()
    xp = ops.split_planes(x.to(DEV), fmt=2)
    assert torch.equal(dec(xp), q16(x.view(-1, C))) and _raised(flag) == 0
    if scale < 1e-4:
        assert ((dec(xp).abs() < 2.0 ** -14) & (dec(xp) != 0)).float().mean().item() > 0.5
    model, mag = conv_model(x, w, None, None, 1, 1, False)
    worst = 0.0
    for tile_n in (64, 128):
        for env in ({}, {"STM_CONV_SPLITK": "3"}):
            tunables.set(**env)
            conv = PlanarConv(w.to(DEV), None, 1, 1, relu=False, tile_n=tile_n, fmt=2)
            conv.kxr = False
            if scale > 1:
                y32 = conv(xp, ("img", B, H, W), out="f32")
            else:
                y32, ypl = conv(xp, ("img", B, H, W), out="both")
                assert torch.equal(dec(ypl)[:, :O], q16(y32.cpu()))
            tunables.clear(*env)
            worst = max(worst, check_model(y32, model, mag, f"scale {scale} tile {tile_n} {env}"))
    ops.planar_range_flag().zero_()
    report(f"conv2d_planar activations x{scale:g}", worst)


def test_conv_fmt2_weights_with_subnormal_products():
    """A layer where a few weights round to fp16 subnormals or to zero under the scale (their max an exact power of two): the model's
    w~ holds them, and the kernel's products with them are exact -- one-hot inputs read each of them back, random inputs meet the model."""
    O, C = 64, 64
    w = spread_weights(O, C, 3, 3, seed=3, top=0.25)
    s = pow2_wscale(w)
    assert s == 2.0 ** 12
    wt = wq(w)
    sub = (wt.abs() * s < 2.0 ** -14) & (wt != 0)
    gone = (wt == 0) & (w != 0)
    assert sub.sum() > 10 and gone.sum() > 10
    x = rnd(2, 10, 12, C, seed=4) * 100.0
    conv = PlanarConv(w.to(DEV), None, 1, 1, relu=False, tile_n=64, fmt=2)
    conv.kxr = False
    y = conv(ops.split_planes(x.to(DEV), fmt=2), ("img", 2, 10, 12), out="f32")
    model, mag = conv_model(x, w, None, None, 1, 1, False)
    report("conv2d_planar subnormal weights", check_model(y, model, mag, "subnormal weights"))


# ------------------------------------------------------------------------------------------------ the fp16 range guard in format 2
def _raised(flag):
    torch.cuda.synchronize()
    v = int(flag.item())
    flag.zero_()
    return v


def test_fp16_range_flag_is_raised_by_every_format2_producer():
    """|x| > 65504, inf and nan raise the sticky flag in every producer of one-plane planes; in-range values leave it alone.  The rule
    the code states (planar_common.h f16_range_check8, stem_fused.hip): the fp32 magnitude bits above those of 65504 -- so values in
    (65504, 65520), which RN16 would still round to 65504, raise it too; 65504 itself does not."""
    flag = ops.planar_range_flag()
    flag.zero_()
    x = rnd(1, 4, 4, 32, seed=1)
    for v, want in [(65504.0, 0), (-65504.0, 0), (65504.004, 1), (65519.0, 1), (-7e4, 1), (float("inf"), 1), (float("-inf"), 1), (float("nan"), 1)]:
        xb = x.clone()
        xb[0, 1, 2, 3] = v
        p = ops.split_planes(xb.to(DEV), fmt=2)
        assert _raised(flag) == want, v
        if want == 0:
            assert dec(p)[6, 3] == v
    # conv epilogue, vector (64) and scalar (41) forms, one-plane and two-plane outputs: y = 32 * xin
    for O in (64, 41):
        w = torch.full((O, 32, 1, 1), 1.0)
        for xin, want in [(2047.0, 0), (2048.0, 1)]:                       # 65504 / 65536
            xp = ops.split_planes(torch.full((1, 4, 4, 32), xin).to(DEV), fmt=2)
            for out_fmt in (2, 1):
                conv = PlanarConv(w.to(DEV), None, 1, 0, relu=False, fmt=2, out_fmt=out_fmt)
                conv.kxr = False
                y = conv(xp, ("img", 1, 4, 4), out="f32")
                assert _raised(flag) == 0 and torch.equal(y.cpu(), torch.full((16, O), 32 * xin))
                conv(xp, ("img", 1, 4, 4), out="both")
                assert _raised(flag) == want, (O, xin, out_fmt)
    # stem_fused: the frame itself (input guard) and the pooled output
    wst = rnd(64, 3, 7, 7, seed=2, scale=0.05)
    packed, osc = ops.stem_pack_weights(wst.to(DEV), 2)
    frame = rnd(1, 20, 24, 3, seed=3)
    ops.stem_fused(frame.to(DEV), packed, osc, None, 2)
    assert _raised(flag) == 0
    fb = frame.clone()
    fb[0, 5, 5, 1] = float("nan")
    ops.stem_fused(fb.to(DEV), packed, osc, None, 2)
    assert _raised(flag) == 1
    ops.stem_fused(frame.to(DEV), packed, osc, torch.full((64,), 7e4).to(DEV), 2)          # in-range frame, outputs ~7e4: the output guard
    assert _raised(flag) == 1
    # dual: the projection source overflows the output
    mid, xs = torch.ones(1, 4, 4, 32), torch.full((1, 8, 8, 32), 2048.0)
    dual = PlanarConv(torch.ones(32, 64, 1, 1).to(DEV), None, 1, 0, relu=False, fmt=2)
    dual(ops.split_planes(mid.to(DEV), fmt=2), ("img", 1, 4, 4), out="both", x2=(ops.split_planes(xs.to(DEV), fmt=2), 8, 8, 2))
    assert _raised(flag) == 1
    dual(ops.split_planes(mid.to(DEV), fmt=2), ("img", 1, 4, 4), out="both", x2=(ops.split_planes((xs / 4).to(DEV), fmt=2), 8, 8, 2))
    assert _raised(flag) == 0
    # kx-reuse
    for xin, want in [(227.0, 0), (228.0, 1)]:                              # 9 * 32 * 227 = 65376, 9 * 32 * 228 = 65664
        kx = PlanarConv(torch.ones(16, 32, 3, 3).to(DEV), None, 1, 1, relu=False, tile_n=64, fmt=2)
        kx.kxr_min_pixels = 0
        assert kx.kxr
        kx(ops.split_planes(torch.full((1, 6, 6, 32), xin).to(DEV), fmt=2), ("img", 1, 6, 6), out="both")
        assert _raised(flag) == want, xin
    # fused DCN: the PRE-activation guard (a ReLU would hide -inf / nan)
    C, O = 64, 128
    xd = rnd(1, 8, 8, C, seed=4)
    om = torch.cat([torch.zeros(64, 18), torch.full((64, 9), 10.0)], 1)
    wdc = -rnd(O, C, 3, 3, seed=5, scale=0.05).abs()
    packed, osc = ops.conv_pack_weights(wdc.to(DEV), tile_n=128, fmt=2)
    for v, want in [(1.0, 0), (6e4, 0), (1e5, 1), (float("nan"), 1)]:
        xb = xd.clone()
        xb[0, 4, 4, 7] = v
        out = ops.deform_conv_fused_planar(xb.reshape(-1, C).to(DEV), 1, 8, 8, C, om.to(DEV), packed, osc, None, O, (3, 3), 1, (1, 1), 1,
                                           has_mask=True, relu=True, fmt=2)
        assert _raised(flag) == want, v
        if want == 0:
            assert torch.isfinite(dec(out)).all()


def test_fp16x1_graph_out_of_range_falls_back_to_bf16x3():
    """The fp16x1 graph (config 5's net, R101-DCN FCB(ali), at 128 x 192) fed a frame scaled out of fp16's range must fall back to bf16x3
    instead of returning detections built from inf / nan: same ids and classes as a pipeline that ran bf16x3 from the start, finite
    rows; range_fallback = False raises, naming the graph's format."""
    from stmask_amd import planar, synthetic
    from stmask_amd.fuse import optimize_for_inference
    from stmask_amd.pipeline import BatchedClipPipeline
    from test_gpu_model import build

    def make(planes, scale_layer=False):
        net = build("STMask_plus_base_ali_config")
        if scale_layer:
            with torch.no_grad():
                net.backbone.layers[2][3].conv1.weight.mul_(1e5)      # a layer3 1x1 conv: its epilogue leaves fp16's range mid-backbone
        optimize_for_inference(net, planar=True, planes=planes)
        net = net.to(memory_format=torch.channels_last)
        net.TemporalNet = net.TemporalNet.to(memory_format=torch.contiguous_format)
        return net, BatchedClipPipeline(net, 2)

    try:
        clip = torch.stack([synthetic.synthetic_clip(3, 128, 192, seed=s) for s in (2, 7)]).cuda()
        clip[:, 0] *= 1e5                                                 # the stem's input guard fires on the first step: every step after
        frames = [clip[:, t].contiguous(memory_format=torch.channels_last) for t in range(3)]      # runs bf16x3 in both pipelines
        (net_a, a), (_, b) = make("fp16x1"), make("bf16x3")
        assert net_a._planar_planes == "fp16x1"
        seen = 0
        for t in range(3):
            pa, pb = a.step(frames[t], is_first=(t == 0)), b.step(frames[t], is_first=(t == 0))
            assert a.fell_back and not b.fell_back
            assert torch.isfinite(pa).all()
            da, db = a.detections(), b.detections()
            for c in range(2):
                assert torch.equal(da[c]["box_ids"], db[c]["box_ids"]) and torch.equal(da[c]["class"], db[c]["class"]), (t, c)
                seen += da[c]["box"].shape[0]
        assert seen > 0 and net_a._planar.fmt == 0 and net_a._planar_planes == "bf16x3"
        # an overflow inside the backbone (a conv epilogue, not the stem's input guard): same fallback, same results as the bf16x3 graph
        # of the same weights
        (_, a2), (_, b2) = make("fp16x1", True), make("bf16x3", True)
        good = clip[:, 2].contiguous(memory_format=torch.channels_last)
        pa, pb = a2.step(good, is_first=True), b2.step(good, is_first=True)
        assert a2.fell_back and torch.equal(pa, pb)
        _, a3 = make("fp16x1")
        a3.range_fallback = False
        with pytest.raises(ops.StmError, match="range of the fp16x1 planar format"):
            a3.step(frames[0], is_first=True)
    finally:
        planar.set_format(1)
        ops.set_range_format("fp16x2")


# ------------------------------------------------------------------------------------------------ config 5's backbone, layer by layer
def ddec(pl, planes=1):
    """Planes [P, S, N, 32] fp16 on the device -> fp32 [N, S * 32]: plane 0 (what a format-2 layer reads), or h + l / 2048."""
    v = pl[0].float()
    if planes == 2:
        v = v + pl[1].float() / ops.F16_LOW_SCALE
    return v.permute(1, 0, 2).reshape(pl.shape[2], pl.shape[1] * 32)


def sample_rows(B, Ho, Wo, n=512, seed=0):
    """~n flat output pixels: the first and last, image-row and image borders, pixels at multiples of 64 / 128 / 256 +- 1 (the
    kernels' pixel tiles), the last partial tile of each width, and random ones."""
    M = B * Ho * Wo
    s = {0, M - 1}
    for b in {0, B - 1}:
        for oy in (0, 1, Ho // 2, Ho - 2, Ho - 1):
            for ox in (0, 1, Wo // 2, Wo - 2, Wo - 1):
                if 0 <= oy < Ho and 0 <= ox < Wo:
                    s.add((b * Ho + oy) * Wo + ox)
    g = torch.Generator().manual_seed(seed)
    for t in (64, 128, 256):
        ks = torch.linspace(1, max(1, M // t), steps=min(20, max(1, M // t))).long().unique().tolist()
        for k in ks:
            for d in (-1, 0, 1):
                if 0 <= k * t + d < M:
                    s.add(k * t + d)
        last = (M // t) * t
        s.update(range(last, min(M, last + 6)))
        s.update(range(max(last, M - 6), M))
    for r in torch.randint(0, Ho, (24,), generator=g).tolist():         # row borders
        s.update({r * Wo, r * Wo + Wo - 1})
    for c in torch.randint(0, Wo, (24,), generator=g).tolist():         # image borders
        s.update({c, (Ho - 1) * Wo + c})
    rest = max(0, n - len(s))
    s.update(torch.randint(0, M, (rest,), generator=g).tolist())
    return torch.tensor(sorted(x for x in s if 0 <= x < M), device=DEV)


def test_config5_backbone_layer_by_layer_at_736x1280(monkeypatch):
    """BASELINE config 5 (R101-DCN FCB(ali), planes="fp16x1") at its real shape, one 736 x 1280 frame, the planar backbone only.  Every
    launch is recorded (PlanarConv.__call__, PlanarConv.deform = the fused DCN, ops.stem_fused).  For each recorded layer the ACTUAL input
    planes are decoded (plane 0: fp16-exact, so errors do not accumulate from layer to layer) and its fp32 output is checked against the
    exact model at ~512 sampled pixels over all output channels; the planes handed on must be RN16 of that fp32 output (one plane inside
    a stage, both planes of format 1 where a stage hands its output to the FPN).  Layers whose launch writes planes only are launched once
    more with an fp32 (or two-plane) output for this.  The recorded set must cover the stem and every layer of every block."""
    from stmask_amd import planar
    from stmask_amd.fuse import optimize_for_inference
    from test_gpu_model import build

    orig_call, orig_deform, orig_stem = PlanarConv.__call__, PlanarConv.deform, ops.stem_fused
    log, on = [], [False]

    def rec_call(self, xp, shape, *args, **kw):
        res = orig_call(self, xp, shape, *args, **kw)
        if on[0]:
            out = kw.get("out", args[0] if args else "planes")
            log.append(dict(kind="conv", conv=self, xp=xp, shape=shape, out=out, res=res, residual=kw.get("residual"), x2=kw.get("x2"),
                            kxr="kxr" in self._packed))
        return res

    def rec_deform(self, x32, B, H, W, om, stride, padding, dilation, has_mask, out=None, out_off=0):
        res = orig_deform(self, x32, B, H, W, om, stride, padding, dilation, has_mask, out=out, out_off=out_off)
        if on[0]:
            log.append(dict(kind="dcn", conv=self, x32=x32, geom=(B, H, W), om=om, sp=(stride, padding, dilation), has_mask=has_mask, res=res))
        return res

    def rec_stem(x_nhwc, packed, out_scale, bias, fmt, out_fmt=None):
        res = orig_stem(x_nhwc, packed, out_scale, bias, fmt, out_fmt)
        if on[0]:
            log.append(dict(kind="stem", args=(x_nhwc, packed, out_scale, bias, fmt), out_fmt=fmt if out_fmt is None else out_fmt, res=res))
        return res

    try:
        net = build("STMask_plus_base_ali_config")
        optimize_for_inference(net, planar=True, planes="fp16x1")
        bb = net._planar_backbone
        assert bb.fmt == 2
        monkeypatch.setattr(PlanarConv, "__call__", rec_call)
        monkeypatch.setattr(PlanarConv, "deform", rec_deform)
        monkeypatch.setattr(ops, "stem_fused", rec_stem)
        x = rnd(1, 3, 736, 1280, seed=5).to(DEV).contiguous(memory_format=torch.channels_last)
        on[0] = True
        with torch.no_grad():
            bb(x)
        on[0] = False
        torch.cuda.synchronize()
        assert int(ops.planar_range_flag().item()) == 0

        names = {}
        for si, blks in enumerate(bb.blocks):
            for bi, e in enumerate(blks):
                assert "chain" not in e                     # (the chain kernel is fp16x2-only: it would run outside the hooks)
                for role, v in e.items():
                    if isinstance(v, PlanarConv):
                        names[id(v)] = f"layer{si + 1}.{bi}.{role}"
        table, worst = [], {}

        def note(fam, v):
            worst[fam] = max(worst.get(fam, 0.0), v)

        def run_checks():
            for r in log:
                if r["kind"] == "stem":
                    xs, packed, osc, bias, fmt = r["args"]
                    planes, (Hp, Wp) = r["res"]
                    B = xs.shape[0]
                    p2, _ = orig_stem(xs, packed, osc, bias, fmt, 1)
                    table.append(("stem", "stem_fused", f"{xs.shape[1]}x{xs.shape[2]} -> {Hp}x{Wp}, out fmt {r['out_fmt']}"))
                    y = ddec(p2, 2)
                    assert torch.equal(ddec(planes), ddec(p2)), "stem: planes handed on differ from the re-run"
                    rows = sample_rows(B, Hp, Wp, seed=1)
                    b, rem = rows // (Hp * Wp), rows % (Hp * Wp)
                    py, px = rem // Wp, rem % Wp
                    Hc, Wc = (xs.shape[1] - 1) // 2 + 1, (xs.shape[2] - 1) // 2 + 1
                    dy = torch.tensor([-1, -1, -1, 0, 0, 0, 1, 1, 1], device=DEV)
                    dx = torch.tensor([-1, 0, 1, -1, 0, 1, -1, 0, 1], device=DEV)
                    cy, cx = 2 * py[:, None] + dy, 2 * px[:, None] + dx
                    ok = (cy >= 0) & (cy < Hc) & (cx >= 0) & (cx < Wc)
                    crow = ((b[:, None] * Hc + cy.clamp(0, Hc - 1)) * Wc + cx.clamp(0, Wc - 1)).reshape(-1)
                    wst = bb.bb.conv1.weight.detach()
                    pre, pmag = conv_q(q16(xs.float()), wq(wst).to(DEV), None, None, 2, 3, False, rows=crow)
                    pre = pre.view(len(rows), 9, -1).masked_fill(~ok[..., None], float("-inf"))
                    pmag = pmag.view(len(rows), 9, -1).masked_fill(~ok[..., None], 0.0)
                    bd = bias.double()
                    model = (pre.max(1).values + bd).clamp_min(0)
                    mag = pmag.max(1).values + bd.abs()
                    yy = y[rows].double()
                    err = (yy - model).abs()
                    assert (err <= TOL * mag + 2.0 ** -21 * yy.abs()).all(), f"stem: {(err / mag).max().item():.3e}"
                    note("stem_fused", (err / mag).max().item())
                    if r["out_fmt"] == 2:
                        assert ((ddec(planes) - y).abs() <= 0.5 * ulp16(ddec(planes)).to(DEV).float()).all()
                    continue
                conv = r["conv"]
                name = names.get(id(conv), "?")
                O, C, kh, kw_ = conv.O, conv.C, conv.kh, conv.kw
                if r["kind"] == "dcn":
                    B, H, W = r["geom"]
                    (st, pd, dl) = r["sp"]
                    Ho, Wo = ops.conv_out_hw(H, W, kh, kw_, *_p2(st), *_p2(pd), *_p2(dl))
                    wide = O % 256 == 0
                    table.append((name, "fused DCN", f"{'64 px x 256 ch' if wide else '128 px x 128 ch'} tiles, {H}x{W} -> {Ho}x{Wo}, C {C} -> {O}, out fmt {conv.out_fmt}"))
                    p2 = ops.deform_conv_fused_planar(r["x32"], B, H, W, C, r["om"], conv.packed(128), conv.out_scale, conv.bias, O, (kh, kw_), st, pd, dl,
                                                      has_mask=r["has_mask"], relu=conv.relu, fmt=2, out_fmt=1)
                    y = ddec(p2, 2)[:, :O]
                    h = ddec(r["res"])[:, :O]
                    assert torch.equal(h, ddec(p2)[:, :O]), f"{name}: planes differ from the re-run"
                    assert ((h - y).abs() <= 0.5 * ulp16(h).to(DEV).float()).all(), f"{name}: planes are not RN16 of the output"
                    rows = sample_rows(B, Ho, Wo, seed=len(table))
                    K = kh * kw_
                    om = r["om"]
                    xin = r["x32"][:, :C].reshape(B, H, W, C)
                    cols, amb, _ = dcn_cols_q(xin, om[:, :2 * K].reshape(B, Ho, Wo, 2 * K), om[:, 2 * K:3 * K].reshape(B, Ho, Wo, K) if r["has_mask"] else None,
                                              kh, kw_, st, pd, dl, rows=rows)
                    wk = wq(conv.weight).permute(0, 2, 3, 1).reshape(O, K * C).double().t().to(DEV)
                    cols, amb = cols.to(DEV), amb.to(DEV)
                    model, mag = cols @ wk, cols.abs() @ wk.abs()
                    slack = (ulp16(cols).to(DEV) * amb) @ wk.abs()
                    if conv.bias is not None:
                        model, mag = model + conv.bias.double(), mag + conv.bias.double().abs()
                    if conv.relu:
                        model = model.clamp_min(0)
                    yy = y[rows].double()
                    err = (yy - model).abs()
                    assert (err <= TOL * mag + slack + 2.0 ** -21 * yy.abs()).all(), f"{name}: {(err / mag).max().item():.3e}"
                    clean = slack == 0
                    note("fused DCN", (err / mag)[clean].max().item())
                    continue
                _, B, H, W = r["shape"]
                Ho, Wo = ops.conv_out_hw(H, W, kh, kw_, conv.sh, conv.sw, conv.ph, conv.pw, 1, 1)
                M = B * Ho * Wo
                x2 = r["x2"]
                if x2 is not None:
                    kind, fam = "dual (c3ds)", "dual"
                elif r["kxr"]:
                    kind, fam = "kxr", "kxr"
                else:
                    kind, fam = f"planar, {conv.pick_tile(M)}-channel tiles", "planar"
                res_ = r["residual"]
                table.append((name, kind, f"{H}x{W} -> {Ho}x{Wo}, C {C} -> {O}, k {kh}x{kw_} s {conv.sh}, out {r['out']} fmt {conv.out_fmt}"
                              + (", residual planes" if res_ is not None else "")))
                res = r["res"]
                if r["out"] in ("f32", "both"):
                    y32 = res[0] if r["out"] == "both" else res
                else:
                    y32 = orig_call(conv, r["xp"], r["shape"], out="f32", residual=res_, x2=x2)
                if r["out"] in ("planes", "both"):
                    pl = res[1] if r["out"] == "both" else res
                    h = ddec(pl)[:, :O]
                    assert torch.equal(h, y32.half().float()), f"{name}: plane 0 handed on is not RN16 of the fp32 output"
                    if conv.out_fmt == 1:
                        full = ddec(pl, 2)[:, :O]
                        assert ((full - y32).abs() <= 2.0 ** -21 * y32.abs() + 1.5e-11).all(), f"{name}: two-plane output"
                rows = sample_rows(B, Ho, Wo, seed=len(table))
                wqt = wq(conv.weight).to(DEV)
                X = ddec(r["xp"])
                if x2 is not None:
                    p2_, H2, W2, s2 = x2
                    X2 = ddec(p2_).view(B, H2, W2, -1)
                    b, rem = rows // (Ho * Wo), rows % (Ho * Wo)
                    P = torch.cat([X[rows], X2[b, (rem // Wo) * s2, (rem % Wo) * s2]], 1).double()
                    wm = wqt.reshape(O, C).double().t()
                    model, mag = P @ wm + conv.bias.double(), P.abs() @ wm.abs() + conv.bias.double().abs()
                    if conv.relu:
                        model = model.clamp_min(0)
                else:
                    rm = None
                    if res_ is not None:
                        rm = ddec(res_)[:, :O] if res_.dtype == torch.float16 else res_
                        rm = rm.reshape(B, Ho, Wo, O)
                    model, mag = conv_q(X.view(B, H, W, -1)[..., :C], wqt, conv.bias, rm, (conv.sh, conv.sw), (conv.ph, conv.pw), conv.relu, rows=rows)
                note(fam, check_model(y32[rows], model, mag, name))

        try:
            run_checks()
        except AssertionError as exc:
            raise AssertionError(f"{exc}\n" + format_table(table)) from None
        print(format_table(table))
        for k, v in worst.items():
            report(f"config5 {k}", v)
        # coverage: the stem and every layer of every block went through a hook
        seen = {id(r["conv"]) for r in log if r["kind"] != "stem"}
        assert sum(r["kind"] == "stem" for r in log) == 1
        missing = []
        for si, blks in enumerate(bb.blocks):
            for bi, e in enumerate(blks):
                need = [e["c1"]]
                if "dcn" in e:
                    need.append(e["om"])
                    need.append(e["dcn_fused"] if id(e.get("dcn_fused")) in seen else e.get("dcn_conv"))
                else:
                    need.append(e["c2"])
                if "c3ds" in e:
                    need.append(e["c3ds"])
                else:
                    need.append(e["c3"])
                    if "ds" in e:
                        need.append(e["ds"])
                missing += [names.get(id(c), f"layer{si + 1}.{bi}.?") for c in need if c is None or id(c) not in seen]
        assert not missing, f"layers that escaped the hooks: {missing}\n" + format_table(table)
        assert len(table) == len(log)
    finally:
        planar.set_format(1)
        ops.set_range_format("fp16x2")


def _p2(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def format_table(table):
    w = max(len(t[0]) for t in table) if table else 10
    k = max(len(t[1]) for t in table) if table else 10
    lines = ["layer".ljust(w) + "  " + "kernel".ljust(k) + "  geometry  (split-K and the 128 / 256 pixel tile height are chosen inside the library)"]
    lines += [a.ljust(w) + "  " + b.ljust(k) + "  " + c for a, b, c in table]
    return "\n".join(lines)
