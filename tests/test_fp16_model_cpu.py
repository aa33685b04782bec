"""CPU checks of the exact format-2 model (tests/fp16_model.py) that the fp16x1 kernel tests measure against: RN16 ties and
subnormals, the power-of-two weight scale of ops.conv_pack_weights, the fp64 convolution of rounded operands and the deformable
sampler model against the fp64 oracle."""
import math

import torch

import oracle
from fp16_model import conv_q, dcn_cols_q, midpoint_distance16, pow2_wscale, q16, wq
from stmask_amd import ops


def test_q16_rounds_to_nearest_even_and_keeps_subnormals():
    e = 2.0 ** -10                                    # fp16 ulp at 1
    x = torch.tensor([1 + e / 2, 1 + 3 * e / 2, 1 + e / 2 + 2.0 ** -20, -(1 + e / 2), 65519.0, 65520.0, 2.0 ** -24, 2.0 ** -25,
                      3 * 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -26, -0.0])
    want = torch.tensor([1.0, 1 + 2 * e, 1 + e, -1.0, 65504.0, float("inf"), 2.0 ** -24, 0.0, 2.0 ** -23, 2.0 ** -24, 2.0 ** -14,
                         0.0, -0.0])
    got = q16(x)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(torch.signbit(got), torch.signbit(want))
    # fp64 values round ONCE (fp64 -> fp32 -> fp16 would make the first value a tie and round it down to 1)
    xd = torch.tensor([1 + e / 2 + 2.0 ** -40, 1 + e / 2 - 2.0 ** -40, 2.0 ** -25 + 2.0 ** -60], dtype=torch.float64)
    assert torch.equal(q16(xd), torch.tensor([1 + e, 1.0, 2.0 ** -24], dtype=torch.float64))


def test_midpoint_distance():
    e = 2.0 ** -10
    v = torch.tensor([1 + e / 2, 1 + e / 2 + 2.0 ** -30, 1.0, 2.0 ** -25, 1 - 2.0 ** -12], dtype=torch.float64)
    d = midpoint_distance16(v)
    # (below 1 the grid is 2^-11: the midpoints next to 1 are 1 - 2^-12 and 1 + 2^-11)
    assert torch.equal(d, torch.tensor([0.0, 2.0 ** -30, 2.0 ** -12, 0.0, 0.0], dtype=torch.float64))


def test_pow2_wscale_is_the_packing_formula():
    vals = [1.0, 0.5, 2.0 ** -7, 3.0, 1 - 2.0 ** -24, 1 + 2.0 ** -23, 2.0 ** 20, 0.0123, 2.0 ** -30, 1.9999999]
    for v in vals:
        w = torch.tensor([[v, -v / 3]], dtype=torch.float32)
        s = pow2_wscale(w)
        assert s == ops._pow2_wscale(w), v
        m = float(w.abs().max()) * s
        assert 1024 <= m < 2048 and math.frexp(s)[0] == 0.5, v
    assert pow2_wscale(torch.zeros(3)) == 1.0 == ops._pow2_wscale(torch.zeros(3))
    # the boundary: an exact power of two is scaled to 1024, the fp32 value just below it to just under 2048
    assert pow2_wscale(torch.tensor([0.25])) == 2.0 ** 12 and pow2_wscale(torch.tensor([0.25 * (1 - 2.0 ** -24)])) == 2.0 ** 13


def test_wq_rounds_under_the_scale_and_shares_it():
    w = torch.tensor([1.0, 1 + 2.0 ** -12, 1 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -26, 3 * 2.0 ** -26, -(2.0 ** -35)])
    s = pow2_wscale(w)                                # 2^10: max |w s| = 1024
    assert s == 1024.0
    want = torch.tensor([1.0, 1.0, 1 + 2.0 ** -9, 2.0 ** -24, 2.0 ** -26, 3 * 2.0 ** -26, -0.0])   # (2^-26 s: subnormal, on the grid)
    got = wq(w)
    assert torch.equal(got, want)
    # below 2^-34 (2^-24 / s) a weight is gone, from 2^-34 to 2^-24 it lands on the subnormal grid of 2^-34
    tiny = torch.tensor([1.0, 2.0 ** -35, 1.5 * 2.0 ** -34, 2.5 * 2.0 ** -34, 2.0 ** -30 + 2.0 ** -36])
    assert torch.equal(wq(tiny), torch.tensor([1.0, 0.0, 2.0 ** -33, 2 * 2.0 ** -34, 2.0 ** -30]))
    # a shared scale: the same rounding in the normal range, a different one where the other tensor's subnormals begin
    a, b = torch.tensor([2.0 ** -20 * (1 + 2.0 ** -10), 1.0 / 3]), torch.tensor([64.0])
    s_cat = pow2_wscale(torch.cat([a, b]))
    assert s_cat == 16.0 and pow2_wscale(a) == 2.0 ** 12
    assert torch.equal(wq(a, s_cat)[1:], wq(a)[1:])
    assert wq(a)[0] == a[0] and wq(a, s_cat)[0] == 2.0 ** -20


def test_conv_q_equals_the_oracle_on_fp16_exact_operands():
    g = torch.Generator().manual_seed(3)
    for (B, H, W, C, O, k, s, p, relu) in [(2, 7, 9, 32, 24, 3, 1, 1, True), (1, 9, 8, 64, 16, 1, 2, 0, False), (1, 6, 10, 32, 8, 5, 1, 2, False)]:
        x = q16(torch.randn(B, H, W, C, generator=g))
        w = wq(torch.randn(O, C, k, k, generator=g) * 0.1)
        b = torch.randn(O, generator=g)
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        r = torch.randn(B, Ho, Wo, O, generator=g)
        y, mag = conv_q(x, w, b, r, stride=s, pad=p, relu=relu)
        ref = oracle.conv2d_nhwc(x, w, b, r, stride=s, padding=p, relu=relu).double()
        assert y.dtype == torch.float64 and y.shape == ref.shape
        assert ((y - ref).abs() <= 2.0 ** -24 * ref.abs() + 1e-12 * mag).all()
        _, mag0 = conv_q(x.abs(), w.abs(), b.abs(), r.abs(), stride=s, pad=p)
        assert torch.allclose(mag, mag0, rtol=1e-15, atol=0)
        rows = torch.tensor([0, 5, B * Ho * Wo - 1])
        yr, mr = conv_q(x, w, b, r, stride=s, pad=p, relu=relu, rows=rows)
        assert torch.equal(yr, y.reshape(-1, O)[rows]) and torch.equal(mr, mag.reshape(-1, O)[rows])


def test_dcn_cols_q_against_the_oracle():
    """The rounded columns times the weights sit within RN16's half ulp of the fp64 oracle; with quarter-pixel offsets, no mask
    and small-integer inputs every sample is fp16-exact and the product equals the oracle to fp32 rounding."""
    g = torch.Generator().manual_seed(5)
    B, C, H, W, O, K = 2, 8, 7, 9, 6, 9
    x = torch.randn(B, H, W, C, generator=g)
    off = torch.randn(B, H, W, 2 * K, generator=g) * 2.5
    off[0, 0, 0, :2] = torch.tensor([-30.0, 40.0])                # a sample far outside: zero
    logit = torch.randn(B, H, W, K, generator=g)
    w = torch.randn(O, C, 3, 3, generator=g) * 0.2
    cols, amb, smag = dcn_cols_q(x, off, logit, 3, 3, 1, 1, 1)
    assert cols.shape == (B * H * W, K * C) and cols[0, :C].abs().max() == 0
    wk = w.permute(0, 2, 3, 1).reshape(O, K * C).double()
    ref = oracle.deform_conv(x.permute(0, 3, 1, 2), off.permute(0, 3, 1, 2).contiguous(), torch.sigmoid(logit).permute(0, 3, 1, 2).contiguous(),
                             w, None, 1, 1, 1, 1).permute(0, 2, 3, 1).reshape(-1, O).double()
    got = cols @ wk.t()
    bound = (2.0 ** -11 * smag + 2.0 ** -25) @ wk.abs().t() + 2.0 ** -22 * ref.abs() + 1e-6
    assert ((got - ref).abs() <= bound).all()
    assert (got - ref).abs().max() > 1e-5                           # the columns really are rounded
    assert 0 < amb.float().mean() < 2e-2                           # (~2^-8 smag / |v| of the samples)
    rows = torch.tensor([0, 7, 62, B * H * W - 1])
    cr, ar, sr = dcn_cols_q(x, off, logit, 3, 3, 1, 1, 1, rows=rows)
    assert torch.equal(cr, cols[rows]) and torch.equal(ar, amb[rows]) and torch.equal(sr, smag[rows])
    # exact samples
    xi = torch.randint(-8, 9, (B, H, W, C), generator=g).float()
    offi = torch.randint(-12, 13, (B, H, W, 2 * K), generator=g).float() / 4
    cols, amb, _ = dcn_cols_q(xi, offi, None, 3, 3, 1, 1, 1)
    ref = oracle.deform_conv(xi.permute(0, 3, 1, 2), offi.permute(0, 3, 1, 2).contiguous(), None, w, None, 1, 1, 1, 1)
    got = (cols @ wk.t()).float().view(B, H, W, O).permute(0, 3, 1, 2)
    assert ((got - ref).abs() <= 2.0 ** -22 * ref.abs() + 1e-6).all()
