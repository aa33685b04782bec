"""The yardsticks of the drop-ins' backward kernels, pinned on the CPU (no GPU):

  * each fp64 restatement of tests/autograd_restate.py computes the forward the oracle already pins (oracle.deform_conv / roi_align /
    corr_patch, which accumulate in double and return fp32: inputs are fp32-representable), within 1e-6 of the largest value;
  * each restatement passes torch.autograd.gradcheck in fp64 on small shapes, so the gradients it hands the GPU tests are right;
  * the four-corner restatement of the deformable convolution (the yardstick at integer and border positions, where grid_sample is not one)
    equals the oracle's forward also on the lattice of -1 / 0 / H-1 / H / half-integer positions, agrees with the grid_sample restatement on
    every gradient at fractional positions, gives F.conv2d's gradients at zero offsets, and reproduces a hand-worked vector of values and
    one-sided derivatives that is this repository's written record of the DCNv2 convention;
  * the new C entry points refuse bad arguments before any launch, and the shims' autograd switch follows grad mode / requires_grad.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import oracle
import autograd_restate as R
from autograd_restate import correlation, deform_conv, deform_conv_corners, roi_align
from stmask_amd import _lib


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _offsets(shape, g, scale=2.0):
    """fp32 offsets whose sums with integer base positions are exact in fp32 (multiples of 2^-10), kept off integer positions."""
    o = torch.round(torch.randn(shape, generator=g) * scale * 1024) / 1024
    return o + (o == torch.round(o)).float() * (1.0 / 512)


def _close(a, b, tol=1e-6):
    return (a.double() - b.double()).abs().max().item() <= tol * max(b.double().abs().max().item(), 1e-30)


@pytest.mark.parametrize("case", [
    dict(C=8, O=6, H=9, W=11, k=(3, 3), s=(1, 1), p=(1, 1), d=(1, 1), dg=1, mask=True, bias=True),
    dict(C=8, O=5, H=12, W=10, k=(3, 3), s=(2, 2), p=(1, 1), d=(1, 1), dg=2, mask=True, bias=True),
    dict(C=6, O=4, H=10, W=12, k=(3, 3), s=(1, 1), p=(2, 2), d=(2, 2), dg=1, mask=True, bias=False),
    dict(C=8, O=8, H=8, W=13, k=(3, 5), s=(1, 1), p=(1, 2), d=(1, 1), dg=2, mask=False, bias=False),
    dict(C=4, O=4, H=11, W=9, k=(5, 3), s=(1, 1), p=(2, 1), d=(1, 1), dg=1, mask=False, bias=False),
])
def test_deform_conv_restatement_matches_the_oracle(case):
    g = _gen(1)
    kh, kw = case["k"]
    K = kh * kw
    B, C, H, W = 2, case["C"], case["H"], case["W"]
    (sh, sw), (ph, pw), (dh, dw) = case["s"], case["p"], case["d"]
    Ho, Wo = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    x = torch.randn(B, C, H, W, generator=g)
    off = _offsets((B, case["dg"] * 2 * K, Ho, Wo), g, 3.0)
    mask = torch.rand(B, case["dg"] * K, Ho, Wo, generator=g) if case["mask"] else None
    w = torch.randn(case["O"], C, kh, kw, generator=g) * 0.2
    b = torch.randn(case["O"], generator=g) if case["bias"] else None
    ref = oracle.deform_conv(x, off, mask, w, b, case["s"], case["p"], case["d"], case["dg"])
    for restatement in (deform_conv, deform_conv_corners):
        got = restatement(x.double(), off.double(), None if mask is None else mask.double(), w.double(), None if b is None else b.double(),
                          case["s"], case["p"], case["d"], case["dg"])
        assert _close(got, ref), restatement.__name__


@pytest.mark.parametrize("sampling_ratio", [0, 2])
def test_roi_align_restatement_matches_the_oracle(sampling_ratio):
    g = _gen(2)
    feat = torch.randn(2, 5, 12, 16, generator=g)
    rois = torch.tensor([[0, 1.0, 2.0, 20.0, 18.0],        # inside
                         [1, -6.0, -4.0, 9.0, 7.5],         # partly outside (top-left)
                         [0, 24.0, 14.0, 40.0, 30.0],       # partly outside (bottom-right), samples beyond H and W
                         [1, 5.0, 5.0, 5.0, 5.0],           # degenerate: zero size
                         [0, 3.25, 7.5, 3.5, 20.0],         # degenerate width
                         [1, 0.0, 0.0, 31.0, 23.0]])        # the whole map
    for scale in (0.5, 1.0):
        ref = oracle.roi_align(feat, rois, (7, 7), scale, sampling_ratio)
        got = roi_align(feat.double(), rois, (7, 7), scale, sampling_ratio)
        assert _close(got, ref)


@pytest.mark.parametrize("P,dil", [(5, 1), (5, 2), (11, 1), (11, 2)])
def test_correlation_restatement_matches_the_oracle(P, dil):
    g = _gen(3)
    f1, f2 = torch.randn(2, 6, 9, 13, generator=g), torch.randn(2, 6, 9, 13, generator=g)
    ref = oracle.corr_patch(f1, f2, P, dil)
    got = correlation(f1.double(), f2.double(), P, dil)
    assert _close(got, ref)


def test_deform_conv_restatement_gradcheck():
    g = _gen(4)
    for (kh, kw), dg, with_mask, stride, dil in (((3, 3), 1, True, (1, 1), (1, 1)), ((3, 3), 2, True, (2, 2), (1, 1)),
                                                  ((3, 5), 1, False, (1, 1), (1, 1)), ((3, 3), 1, True, (1, 1), (2, 2))):
        K = kh * kw
        B, C, H, W, O = 1, 4, 6, 7, 3
        pad = ((kh // 2) * dil[0], (kw // 2) * dil[1])
        Ho, Wo = (H + 2 * pad[0] - (dil[0] * (kh - 1) + 1)) // stride[0] + 1, (W + 2 * pad[1] - (dil[1] * (kw - 1) + 1)) // stride[1] + 1
        x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        # fractional offsets at least 0.05 away from integer positions (the derivative jumps there)
        o = torch.randn(B, dg * 2 * K, Ho, Wo, generator=g, dtype=torch.float64) * 2
        o = torch.floor(o) + 0.05 + 0.9 * torch.rand(o.shape, generator=g, dtype=torch.float64)
        off = o.requires_grad_(True)
        mask = torch.rand(B, dg * K, Ho, Wo, generator=g, dtype=torch.float64).requires_grad_(True) if with_mask else None
        w = (torch.randn(O, C, kh, kw, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
        b = torch.randn(O, generator=g, dtype=torch.float64, requires_grad=True)

        def f(x, off, w, b, *m):
            return deform_conv(x, off, m[0] if m else None, w, b, stride, pad, dil, dg, fp32_positions=False)

        args = (x, off, w, b) + ((mask,) if mask is not None else ())
        assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_roi_align_restatement_gradcheck():
    g = _gen(5)
    feat = torch.randn(2, 3, 7, 9, generator=g, dtype=torch.float64, requires_grad=True)
    rois = torch.tensor([[0, 0.7, 1.3, 9.1, 6.2], [1, -2.3, -1.6, 4.1, 3.3], [0, 10.3, 5.2, 14.9, 9.7], [1, 2.0, 2.0, 2.0, 2.0]])
    for sr in (0, 2):
        assert torch.autograd.gradcheck(lambda f: roi_align(f, rois, (3, 3), 1.0, sr), (feat,), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_correlation_restatement_gradcheck():
    g = _gen(6)
    a = torch.randn(1, 3, 6, 7, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(1, 3, 6, 7, generator=g, dtype=torch.float64, requires_grad=True)
    for P, dil in ((5, 1), (3, 2)):
        assert torch.autograd.gradcheck(lambda u, v: correlation(u, v, P, dil), (a, b), eps=1e-6, atol=1e-6, rtol=1e-5)


# ---- the four-corner restatement: the yardstick at integer and border positions ------------------------------------------------------
@pytest.mark.parametrize("k,s,dg,with_mask", [((3, 3), (1, 1), 1, True), ((3, 5), (2, 2), 2, False), ((5, 3), (1, 1), 1, True)])
def test_four_corner_restatement_matches_the_oracle_on_the_lattice(k, s, dg, with_mask):
    """Positions exactly on -1, 0, H-1, H, their fp32 neighbours inside, integers, half-integers and far outside (each class present)."""
    g = _gen(7)
    kh, kw = k
    pad, H, W, C, O = (kh // 2, kw // 2), 8, 10, 4, 3
    off = R.lattice_offsets(2, dg, kh, kw, H, W, s, pad, (1, 1), g)
    for shares in R.position_classes(off, dg, kh, kw, H, W, s, pad, (1, 1)):
        assert min(shares.values()) >= 0.01, shares
    x = torch.randn(2, C, H, W, generator=g)
    mask = torch.rand(2, dg * kh * kw, *off.shape[-2:], generator=g) if with_mask else None
    w = torch.randn(O, C, kh, kw, generator=g) * 0.2
    b = torch.randn(O, generator=g)
    ref = oracle.deform_conv(x, off, mask, w, b, s, pad, (1, 1), dg)
    got = deform_conv_corners(x.double(), off.double(), None if mask is None else mask.double(), w.double(), b.double(), s, pad, (1, 1), dg)
    assert _close(got, ref)


@pytest.mark.parametrize("fp32_positions", [True, False])
def test_four_corner_and_grid_sample_restatements_agree_at_fractional_positions(fp32_positions):
    """Two independent restatements; every gradient within 1e-10 of its largest element (they agree to ~1e-14)."""
    g = _gen(8)
    for (kh, kw), dg, with_mask, stride, dil in (((3, 3), 1, True, (1, 1), (1, 1)), ((3, 3), 2, True, (2, 2), (1, 1)),
                                                  ((3, 5), 1, False, (1, 1), (1, 1)), ((5, 3), 2, False, (1, 1), (1, 1)),
                                                  ((3, 3), 1, True, (1, 1), (2, 2))):
        K, B, C, H, W, O = kh * kw, 2, 4, 9, 11, 3
        pad = ((kh // 2) * dil[0], (kw // 2) * dil[1])
        Ho, Wo = (H + 2 * pad[0] - (dil[0] * (kh - 1) + 1)) // stride[0] + 1, (W + 2 * pad[1] - (dil[1] * (kw - 1) + 1)) // stride[1] + 1
        leaves = [torch.randn(B, C, H, W, generator=g), _offsets((B, dg * 2 * K, Ho, Wo), g, 3.0),
                  torch.rand(B, dg * K, Ho, Wo, generator=g) if with_mask else None, torch.randn(O, C, kh, kw, generator=g) * 0.3,
                  torch.randn(O, generator=g)]
        go = torch.randn(B, O, Ho, Wo, generator=g).double()
        grads = []
        for restatement in (deform_conv, deform_conv_corners):
            a = [None if t is None else t.double().requires_grad_() for t in leaves]
            y = restatement(*a, stride, pad, dil, dg, fp32_positions=fp32_positions)
            y.backward(go)
            grads.append([y.detach()] + [t.grad for t in a if t is not None])
        for u, v in zip(*grads):
            assert (u - v).abs().max().item() <= 1e-10 * v.abs().max().item()


def test_four_corner_restatement_gradcheck():
    g = _gen(9)
    for (kh, kw), dg, with_mask, stride, dil in (((3, 3), 1, True, (1, 1), (1, 1)), ((3, 3), 2, True, (2, 2), (1, 1)),
                                                  ((3, 5), 1, False, (1, 1), (1, 1)), ((3, 3), 1, True, (1, 1), (2, 2))):
        K = kh * kw
        B, C, H, W, O = 1, 4, 6, 7, 3
        pad = ((kh // 2) * dil[0], (kw // 2) * dil[1])
        Ho, Wo = (H + 2 * pad[0] - (dil[0] * (kh - 1) + 1)) // stride[0] + 1, (W + 2 * pad[1] - (dil[1] * (kw - 1) + 1)) // stride[1] + 1
        x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        o = torch.randn(B, dg * 2 * K, Ho, Wo, generator=g, dtype=torch.float64) * 2
        o = torch.floor(o) + 0.05 + 0.9 * torch.rand(o.shape, generator=g, dtype=torch.float64)     # finite differences need a smooth point
        off = o.requires_grad_(True)
        mask = torch.rand(B, dg * K, Ho, Wo, generator=g, dtype=torch.float64).requires_grad_(True) if with_mask else None
        w = (torch.randn(O, C, kh, kw, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
        b = torch.randn(O, generator=g, dtype=torch.float64, requires_grad=True)

        def f(x, off, w, b, *m):
            return deform_conv_corners(x, off, m[0] if m else None, w, b, stride, pad, dil, dg, fp32_positions=False)

        args = (x, off, w, b) + ((mask,) if mask is not None else ())
        assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("k", [(3, 3), (3, 5), (5, 3)])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dil", [1, 2])
def test_four_corner_restatement_at_zero_offsets_is_a_convolution(k, stride, dil):
    """Zero offsets and a constant mask m: y = m * conv2d(x, w) + bias (the bias is not scaled), so the x / weight / bias gradients are
    F.conv2d's.  The outer taps of the border outputs sit exactly on -1 and on H / W.  The offset gradient is checked too, against the rule
    written with F.unfold: d sample / d dy at an integer row r is x[r + 1] - x[r] (x[H] = 0) for 0 <= r <= H - 1 and 0 elsewhere -- at
    r = -1 it is 0, not x[0] -- and F.unfold's zero padding supplies exactly those zeros."""
    g = _gen(10)
    kh, kw = k
    K, B, C, O, H, W, m = kh * kw, 2, 3, 4, 9, 10, 0.375
    st, dl, pad = (stride, stride), (dil, dil), ((kh // 2) * dil, (kw // 2) * dil)
    x, w, b = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((B, C, H, W), (O, C, kh, kw), (O,)))
    ref = [t.clone().requires_grad_() for t in (x, w, b)]
    y_ref = m * F.conv2d(ref[0], ref[1], None, st, pad, dl) + ref[2].view(1, O, 1, 1)
    go = torch.randn(y_ref.shape, generator=g, dtype=torch.float64)
    y_ref.backward(go)
    Ho, Wo = y_ref.shape[-2:]
    for fp32_positions in (True, False):
        got = [t.clone().requires_grad_() for t in (x, w, b)]
        off = torch.zeros(B, 2 * K, Ho, Wo, dtype=torch.float64, requires_grad=True)
        mask = torch.full((B, K, Ho, Wo), m, dtype=torch.float64)
        y = deform_conv_corners(got[0], off, mask, got[1], got[2], st, pad, dl, 1, fp32_positions=fp32_positions)
        y.backward(go)
        assert (y - y_ref).abs().max().item() <= 1e-10 * y_ref.abs().max().item()
        for u, v in zip(got, ref):
            assert (u.grad - v.grad).abs().max().item() <= 1e-10 * v.grad.abs().max().item()
        gcols = torch.matmul(w.reshape(O, C * K).t(), go.reshape(B, O, Ho * Wo)).view(B, C, K, Ho * Wo)
        d_dy = F.pad(x, (0, 0, 0, 1))[:, :, 1:] - x            # x[r + 1] - x[r], rows 0 .. H-1
        d_dx = F.pad(x, (0, 1))[:, :, :, 1:] - x
        want = torch.stack([(gcols * F.unfold(d, k, dl, pad, st).view(B, C, K, Ho * Wo)).sum(1) * m for d in (d_dy, d_dx)], 2)
        want = want.view(B, 2 * K, Ho, Wo)
        assert (off.grad - want).abs().max().item() <= 1e-10 * want.abs().max().item()


def test_four_corner_restatement_hand_worked_vector():
    """The written record of the convention (the reference tree carries no source for DCNv2's CUDA extension).  The rule, from DCNv2's
    dmcn_im2col_bilinear and dmcn_get_coordinate_weight: a sample and its coordinate weights are 0 if `h <= -1 || h >= H || w <= -1 || w >= W`;
    otherwise `h_low = floor(h)` (also at integer h), `lh = h - h_low`, the four corners weighted (1 - lh)(1 - lw), (1 - lh) lw, lh (1 - lw),
    lh lw with a corner outside the image contributing 0; the weight of the h coordinate is the derivative of that expression with h_low held
    fixed: -(1 - lw) v1 - lw v2 + (1 - lw) v3 + lw v4.

    One channel, the 3x3 image below, one tap (a 1x1 kernel of weight 1).  A position p on one axis, an integer c on the other.  Along the
    axis the image column (a0, a1, a2) gives, row by row of the tables: the value as weights on (a0, a1, a2), and the derivative likewise:
        p = -1    value 0         derivative 0           (not inside)
        p = -0.5  value 0.5 a0    derivative +a0         (h_low = -1 is outside: only row 0 counts, with weight lh)
        p = 0     value a0        derivative a1 - a0     (right-sided)
        p = 1     value a1        derivative a2 - a1
        p = 2     value a2        derivative -a2         (= H-1: h_high = 3 is outside)
        p = 2.5   value 0.5 a2    derivative -a2
        p = 3     value 0         derivative 0           (= H: not inside)
    and the derivative along the other axis, at its integer c, is the same value weights applied to the right-sided difference
    x[., c + 1] - x[., c] (x[., 3] = 0)."""
    img = torch.tensor([[1.0, 2.0, 4.0], [7.0, 11.0, 16.0], [22.0, 29.0, 37.0]], dtype=torch.float64)
    VALUE = {-1.0: (0, 0, 0), -0.5: (0.5, 0, 0), 0.0: (1, 0, 0), 1.0: (0, 1, 0), 2.0: (0, 0, 1), 2.5: (0, 0, 0.5), 3.0: (0, 0, 0)}
    DERIV = {-1.0: (0, 0, 0), -0.5: (1, 0, 0), 0.0: (-1, 1, 0), 1.0: (0, -1, 1), 2.0: (0, 0, -1), 2.5: (0, 0, -1), 3.0: (0, 0, 0)}
    one = torch.ones(1, 1, 1, 1, dtype=torch.float64)
    idx = torch.arange(3, dtype=torch.float64)
    for axis in (0, 1):
        a = img if axis == 0 else img.t()                      # a[r, c]: r along the axis under test
        right = torch.cat([a[:, 1:], torch.zeros(3, 1, dtype=torch.float64)], 1) - a
        for p in VALUE:
            inside = -1 < p < 3
            wv, wd = torch.tensor(VALUE[p], dtype=torch.float64), torch.tensor(DERIV[p], dtype=torch.float64)
            value, d_along, d_across = wv @ a, wd @ a, (wv @ right) * inside            # one entry per c
            for fp32_positions in (True, False):
                off = torch.zeros(1, 2, 3, 3, dtype=torch.float64)
                off[0, axis] = (p - idx).view(3, 1) if axis == 0 else (p - idx).view(1, 3)      # every output samples (p, c) / (c, p)
                off.requires_grad_()
                y = deform_conv_corners(img.view(1, 1, 3, 3), off, None, one, None, fp32_positions=fp32_positions)
                y.sum().backward()
                for r in range(3):                              # the output index along the axis does not matter: all sample at p
                    sel = (lambda t: t[r, :]) if axis == 0 else (lambda t: t[:, r])
                    assert torch.equal(sel(y[0, 0].detach()), value), (axis, p, "value")
                    assert torch.equal(sel(off.grad[0, axis]), d_along), (axis, p, "derivative along the axis")
                    assert torch.equal(sel(off.grad[0, 1 - axis]), d_across), (axis, p, "derivative across the axis")


@pytest.mark.parametrize("sampling_ratio", [0, 1, 2])
def test_roi_align_restatement_not_aligned_matches_the_oracle_and_gradcheck(sampling_ratio):
    g = _gen(11)
    feat = torch.randn(2, 5, 12, 16, generator=g)
    rois = torch.tensor([[0, 1.0, 2.0, 20.0, 18.0], [1, -6.0, -4.0, 9.0, 7.5], [0, 24.0, 14.0, 40.0, 30.0],
                         [1, 5.0, 5.0, 5.0, 5.0],            # zero size: clamped to 1 x 1
                         [0, 3.25, 7.5, 3.5, 20.0],          # width below 1
                         [1, 0.0, 0.0, 31.0, 23.0],
                         [0, -2.0, -2.0, 12.0, 12.0]])       # integer corners: with sampling_ratio 1 samples land on -1 and on integers
    for scale in (0.5, 1.0):
        for out in ((7, 7), (7, 3), (1, 1)):
            ref = oracle.roi_align(feat, rois, out, scale, sampling_ratio, "avg", False)
            got = roi_align(feat.double(), rois, out, scale, sampling_ratio, aligned=False)
            assert _close(got, ref), (scale, out)
    f64 = torch.randn(2, 3, 7, 9, generator=g, dtype=torch.float64, requires_grad=True)
    small = torch.tensor([[0, 0.7, 1.3, 9.1, 6.2], [1, -2.3, -1.6, 4.1, 3.3], [0, 10.3, 5.2, 14.9, 9.7], [1, 2.0, 2.0, 2.0, 2.0]])
    assert torch.autograd.gradcheck(lambda f: roi_align(f, small, (3, 3), 1.0, sampling_ratio, aligned=False), (f64,), eps=1e-6, atol=1e-6,
                                    rtol=1e-5)


# ---- C entry points and the shims' switch, without a GPU ---------------------------------------------------------------------------
def test_backward_entries_are_bound_and_exported():
    L = _lib.lib()
    for name in ("stm_deform_col2im_f32", "stm_deform_col2im_coord_f32", "stm_roi_align_backward_f32", "stm_corr_backward_f32"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name)


def test_backward_entries_refuse_bad_arguments_before_launching():
    L = _lib.lib()
    fake = ctypes.c_void_p(1 << 40)             # never dereferenced: every call below fails its argument checks first
    c_i, c_l, c_f = ctypes.c_int, ctypes.c_int64, ctypes.c_float
    good = _lib.DeformGeom(1, 8, 6, 6, 3, 3, 1, 1, 1, 1, 1, 1, 1, 6, 6)
    bad_out = _lib.DeformGeom(1, 8, 6, 6, 3, 3, 1, 1, 1, 1, 1, 1, 1, 5, 6)
    bad_dg = _lib.DeformGeom(1, 8, 6, 6, 3, 3, 1, 1, 1, 1, 1, 1, 3, 6, 6)
    full = c_l(2 * 9 * 36)
    assert L.stm_deform_col2im_f32(fake, fake, full, None, c_l(0), c_i(0), fake, ctypes.byref(bad_out), None) == -1
    assert L.stm_deform_col2im_f32(fake, fake, full, None, c_l(0), c_i(0), fake, ctypes.byref(bad_dg), None) == -1
    assert L.stm_deform_col2im_f32(fake, fake, c_l(2 * 9 * 36 - 1), None, c_l(0), c_i(0), fake, ctypes.byref(good), None) == -1
    assert L.stm_deform_col2im_f32(None, fake, full, None, c_l(0), c_i(0), fake, ctypes.byref(good), None) == -2
    assert L.stm_deform_col2im_f32(fake, fake, full, None, c_l(0), c_i(0), fake, None, None) == -2
    assert b"stm_deform_col2im_f32" in L.stm_last_error_string()
    co = L.stm_deform_col2im_coord_f32
    assert co(fake, fake, fake, full, None, c_l(0), c_i(0), None, full, None, c_l(0), ctypes.byref(good), None) == -2   # nothing to compute
    assert co(fake, fake, fake, full, None, c_l(0), c_i(0), fake, full, fake, c_l(81), ctypes.byref(good), None) == -1  # grad_mask, no mask
    assert co(fake, fake, fake, full, fake, c_l(8), c_i(0), fake, full, fake, c_l(324), ctypes.byref(good), None) == -1  # mask stride
    assert co(fake, None, fake, full, None, c_l(0), c_i(0), fake, full, None, c_l(0), ctypes.byref(good), None) == -2
    ra = L.stm_roi_align_backward_f32
    assert ra(fake, fake, fake, c_i(1), c_i(4), c_i(8), c_i(8), c_i(-1), c_i(7), c_i(7), c_f(1.0), c_i(0), c_i(1), None) == -1
    assert ra(fake, fake, fake, c_i(1), c_i(4), c_i(8), c_i(8), c_i(3), c_i(0), c_i(7), c_f(1.0), c_i(0), c_i(1), None) == -1
    assert ra(None, fake, fake, c_i(1), c_i(4), c_i(8), c_i(8), c_i(3), c_i(7), c_i(7), c_f(1.0), c_i(0), c_i(1), None) == -2
    assert ra(None, None, None, c_i(1), c_i(4), c_i(8), c_i(8), c_i(0), c_i(7), c_i(7), c_f(1.0), c_i(0), c_i(1), None) == 0  # no RoIs
    cb = L.stm_corr_backward_f32
    assert cb(fake, fake, fake, fake, fake, c_i(1), c_i(4), c_i(8), c_i(8), c_i(4), c_i(1), None) == -1     # even patch
    assert cb(fake, fake, fake, fake, fake, c_i(1), c_i(4), c_i(8), c_i(8), c_i(5), c_i(0), None) == -1     # dilation 0
    assert cb(fake, fake, fake, None, None, c_i(1), c_i(4), c_i(8), c_i(8), c_i(5), c_i(1), None) == -2
    assert cb(fake, fake, fake, fake, fake, c_i(0), c_i(4), c_i(8), c_i(8), c_i(5), c_i(1), None) == -1


def test_autograd_switch_follows_grad_mode_and_requires_grad():
    from stmask_amd.autograd import wants_grad
    a, p = torch.zeros(2), torch.nn.Parameter(torch.zeros(2))
    assert wants_grad(a, p) and not wants_grad(a, None)
    with torch.no_grad():
        assert not wants_grad(a, p)
    p.requires_grad_(False)
    assert not wants_grad(a, p)


def test_fused_relu_dcn_refuses_autograd():
    """fuse.optimize_for_inference sets DCN.fuse_relu; under autograd that module must refuse rather than silently fuse (raised before
    any kernel is launched, so a CPU tensor is enough to see it)."""
    from stmask_amd.dcn_v2 import DCN
    m = DCN(4, 4, 3, 1, 1)
    m.fuse_relu = True
    with pytest.raises(RuntimeError, match="inference-only"):
        m(torch.randn(1, 4, 5, 5))
