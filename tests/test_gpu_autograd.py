"""Gradients of the drop-ins on the MI355X (stmask_amd/autograd.py over csrc/deform_backward.hip and csrc/temporal_backward.hip), held to the
fp64 restatements of tests/autograd_restate.py (pinned on the CPU by test_autograd_cpu.py).

Tolerance (the style of test_gpu_conv.py): |g - g64| <= 1e-5 * sum|terms| + 1e-7, where sum|terms| is the same gradient computed on absolute
values (for the offsets, where the bilinear derivative is a difference, autograd_restate.deform_conv_offset_magnitude sums its terms' sizes).
Where a sample position comes out of a GPU layer (DCN's conv_offset_mask, an offset convolution), the fp64 side takes that layer's fp32
VALUE and its own fp64 graph, so both sides sample at the same point (a floor() on either side of an integer would be a different gradient).
The tests call only the shims and the restatements: on a tree without backward kernels they fail on the missing gradients.

What this file deliberately avoids: sample positions ON integers and ON -1 / H / W (_offsets moves every integer offset by 0.125), because
grid_sample, the yardstick here, is not right there.  test_gpu_autograd_edges.py covers exactly those positions (a freshly constructed DCN, a
lattice of border / integer / half-integer positions) with the four-corner restatement, and with them correlation maps of several tiles and the
global-memory form, RoIAlign with aligned=False, and the ways autograd calls the Functions.
"""
import copy

import pytest
import torch
import torch.nn as nn

import autograd_restate as R
from stmask_amd._lib import StmError
from stmask_amd.dcn_v2 import DCN, DCNv2
from stmask_amd.mmcv_ops import DeformConv2d, RoIAlign, roi_align
from stmask_amd.spatial_correlation_sampler import SpatialCorrelationSampler, spatial_correlation_sample

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _check(name, g, g64, mag, rel=1e-5):
    assert g is not None, f"{name}: no gradient"
    d = (g.detach().cpu().double() - g64.detach().double()).abs()
    bound = rel * mag.detach().double() + 1e-7
    worst = (d / bound).max().item()
    assert worst <= 1.0, f"{name}: worst |g - g64| / bound = {worst:.3f}"


def _offsets(B, dg, kh, kw, Ho, Wo, H, W, stride, padding, dilation, g, scale=2.0, band_share=0.3):
    """fractional offsets; a share of the samples is sent to the (-1, 0) and (H-1, H) bands and outside the image, on both axes."""
    K = kh * kw
    off = torch.randn(B, dg, K, 2, Ho, Wo, generator=g) * scale
    by = (torch.arange(Ho) * stride[0] - padding[0]).view(1, 1, 1, Ho, 1).float()
    bx = (torch.arange(Wo) * stride[1] - padding[1]).view(1, 1, 1, 1, Wo).float()
    ti = (torch.arange(K) // kw * dilation[0]).view(1, 1, K, 1, 1).float()
    tj = (torch.arange(K) % kw * dilation[1]).view(1, 1, K, 1, 1).float()
    for axis, base, size in ((0, by + ti, H), (1, bx + tj, W)):
        shape = (B, dg, K, Ho, Wo)
        u = torch.rand(shape, generator=g)
        target = torch.where(u < 0.5, -1.0 + 0.02 + 0.96 * torch.rand(shape, generator=g),          # (-1, 0)
                             size - 1.0 + 0.02 + 0.96 * torch.rand(shape, generator=g))             # (H-1, H)
        far = torch.rand(shape, generator=g) < 0.25
        outside = torch.where(u < 0.5, -3.3 + torch.rand(shape, generator=g), size + 0.3 + torch.rand(shape, generator=g))
        target = torch.where(far, outside, target)
        pick = torch.rand(shape, generator=g) < band_share
        off[:, :, :, axis] = torch.where(pick, target - base, off[:, :, :, axis])
    off = off + (off == torch.round(off)).float() * 0.125
    return off.reshape(B, dg * 2 * K, Ho, Wo)


def _dcn_case(B, C, O, H, W, k, stride, pad, dil, dg, seed, with_mask=True, with_bias=True):
    g = _gen(seed)
    kh, kw = k
    Ho, Wo = (H + 2 * pad[0] - (dil[0] * (kh - 1) + 1)) // stride[0] + 1, (W + 2 * pad[1] - (dil[1] * (kw - 1) + 1)) // stride[1] + 1
    x = torch.randn(B, C, H, W, generator=g)
    off = _offsets(B, dg, kh, kw, Ho, Wo, H, W, stride, pad, dil, g)
    mask = torch.rand(B, dg * kh * kw, Ho, Wo, generator=g) if with_mask else None
    w = torch.randn(O, C, kh, kw, generator=g) / (C * kh * kw) ** 0.5
    b = torch.randn(O, generator=g) if with_bias else None
    go = torch.randn(B, O, Ho, Wo, generator=g)
    return x, off, mask, w, b, go


def _ref_grads(x, off, mask, w, b, go, stride, pad, dil, dg):
    """fp64 gradients and their magnitudes: (grads, mags), each a dict over x / offset / mask / weight / bias."""
    def run(xx, oo, mm, ww, bb, gg):
        leaves = {"x": xx.double().requires_grad_(), "offset": oo.double().requires_grad_(), "weight": ww.double().requires_grad_()}
        if mm is not None:
            leaves["mask"] = mm.double().requires_grad_()
        if bb is not None:
            leaves["bias"] = bb.double().requires_grad_()
        y = R.deform_conv(leaves["x"], leaves["offset"], leaves.get("mask"), leaves["weight"], leaves.get("bias"), stride, pad, dil, dg)
        y.backward(gg.double())
        return {k: v.grad for k, v in leaves.items()}
    ref = run(x, off, mask, w, b, go)
    mag = run(x.abs(), off, None if mask is None else mask.abs(), w.abs(), None if b is None else b.abs(), go.abs())
    mag["offset"] = R.deform_conv_offset_magnitude(x, off, mask, go, w, stride, pad, dil, dg)
    return ref, mag


# R50 DCN layers (input map, stride) at batch 2, channels cut to 32
R50_DCN = [("L1.0", 96, 160, 2), ("L1.2", 48, 80, 1), ("L2.0", 48, 80, 2), ("L2.2", 24, 40, 1), ("L2.4", 24, 40, 1), ("L3.0", 24, 40, 2),
           ("L3.2", 12, 20, 1)]


@pytest.mark.parametrize("case", [dict(name=n, H=h, W=w, s=s, C=32, dil=1, dg=1) for n, h, w, s in R50_DCN] + [
    dict(name="L3.2 full width", H=12, W=20, s=1, C=512, dil=1, dg=1),
    dict(name="dilation 2", H=24, W=40, s=1, C=32, dil=2, dg=1),
    dict(name="deformable_groups 2", H=24, W=40, s=2, C=32, dil=1, dg=2)], ids=lambda c: c["name"])
def test_dcnv2_gradients_match_fp64(case):
    st, dl = (case["s"],) * 2, (case["dil"],) * 2
    pad = dl
    x, off, mask, w, b, go = _dcn_case(2, case["C"], case["C"], case["H"], case["W"], (3, 3), st, pad, dl, case["dg"], seed=11)
    m = DCNv2(case["C"], case["C"], 3, st, pad, dl, case["dg"]).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    xg, og, mg = (t.to(DEV).requires_grad_() for t in (x, off, mask))
    m(xg, og, mg).backward(go.to(DEV))
    ref, mag = _ref_grads(x, off, mask, w, b, go, st, pad, dl, case["dg"])
    for name, got in (("x", xg.grad), ("offset", og.grad), ("mask", mg.grad), ("weight", m.weight.grad), ("bias", m.bias.grad)):
        _check(f"{case['name']} {name}", got, ref[name], mag[name])


@pytest.mark.parametrize("k", [(3, 3), (3, 5), (5, 3)])
@pytest.mark.parametrize("dg", [1, 2])
def test_deform_conv2d_v1_gradients_match_fp64(k, dg):
    pad = (k[0] // 2, k[1] // 2)
    x, off, _, w, _, go = _dcn_case(2, 32, 32, 24, 40, k, (1, 1), pad, (1, 1), dg, seed=12, with_mask=False, with_bias=False)
    m = DeformConv2d(32, 32, k, padding=pad, deform_groups=dg).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w)
    xg, og = x.to(DEV).requires_grad_(), off.to(DEV).requires_grad_()
    m(xg, og).backward(go.to(DEV))
    ref, mag = _ref_grads(x, off, None, w, None, go, (1, 1), pad, (1, 1), dg)
    for name, got in (("x", xg.grad), ("offset", og.grad), ("weight", m.weight.grad)):
        _check(f"{k} dg{dg} {name}", got, ref[name], mag[name])


def _dcn_module(C, stride, seed):
    g = _gen(seed)
    m = DCN(C, C, 3, stride, 1)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g) / (9 * C) ** 0.5)
        m.bias.copy_(torch.randn(C, generator=g))
        m.conv_offset_mask.weight.copy_(torch.randn(m.conv_offset_mask.weight.shape, generator=g) * 0.3)
        m.conv_offset_mask.bias.copy_(torch.randn(27, generator=g))
    return m


def _dcn_fused_fp64(m, x, stride, om_value=None):
    """dcn_v2.DCN.forward in fp64 on the CPU: conv_offset_mask, chunk / cat / sigmoid in torch, then the restatement.  om_value: the GPU's
    conv_offset_mask output, whose value the fp64 om takes (its graph stays fp64)."""
    om = nn.functional.conv2d(x, m.conv_offset_mask.weight, m.conv_offset_mask.bias, stride, 1)
    if om_value is not None:
        om = om + (om_value.detach().cpu().double() - om).detach()
    o1, o2, mk = torch.chunk(om, 3, dim=1)
    return om, R.deform_conv(x, torch.cat((o1, o2), 1), torch.sigmoid(mk), m.weight, m.bias, (stride, stride), (1, 1), (1, 1), 1)


class _Capture:
    """forward hook: keeps a module's output (and its gradient)."""

    def __init__(self, module):
        self.out = None
        module.register_forward_hook(self)

    def __call__(self, module, inputs, output):
        if output.requires_grad:
            output.retain_grad()
        self.out = output


@pytest.mark.parametrize("C,H,W,stride", [(32, 48, 80, 2), (64, 24, 40, 1)])
def test_dcn_fused_om_gradients_match_fp64(C, H, W, stride):
    m = _dcn_module(C, stride, seed=13)
    x = torch.randn(2, C, H, W, generator=_gen(14))
    mg = copy.deepcopy(m).to(DEV)
    cap = _Capture(mg.conv_offset_mask)
    xg = x.to(DEV).requires_grad_()
    y = mg(xg)
    go = torch.randn(y.shape, generator=_gen(15))
    y.backward(go.to(DEV))
    m64 = copy.deepcopy(m).double()
    x64 = x.double().requires_grad_()
    om, y64 = _dcn_fused_fp64(m64, x64, stride, cap.out)
    om.retain_grad()
    y64.backward(go.double())
    # magnitudes: the gradient w.r.t. the raw om channels (offsets, then mask logits) on absolute values
    K = 9
    omd = om.detach()
    s = torch.sigmoid(omd[:, 2 * K:])
    _, mag = _ref_grads(x, omd[:, :2 * K].float(), s.float(), m.weight.detach(), m.bias.detach(), go, (stride,) * 2, (1, 1), (1, 1), 1)
    mag_om = torch.cat([mag["offset"], mag["mask"] * s * (1 - s)], 1)
    _check("om", cap.out.grad, om.grad, mag_om)
    # parameters of conv_offset_mask: torch's convolution backward applied to the om gradient; the bound carries |input| * bound(om)
    mag_w = torch.nn.grad.conv2d_weight(x.double().abs(), m.conv_offset_mask.weight.shape, mag_om, stride, 1)
    _check("conv_offset_mask.weight", mg.conv_offset_mask.weight.grad, m64.conv_offset_mask.weight.grad, mag_w, rel=2e-5)
    _check("conv_offset_mask.bias", mg.conv_offset_mask.bias.grad, m64.conv_offset_mask.bias.grad, mag_om.sum((0, 2, 3)), rel=2e-5)
    _check("weight", mg.weight.grad, m64.weight.grad, mag["weight"])
    _check("bias", mg.bias.grad, m64.bias.grad, mag["bias"])
    assert xg.grad is not None and torch.isfinite(xg.grad).all()


def _rois(n_img, H, W, scale, seed):
    g = _gen(seed)
    Hs, Ws = H / scale, W / scale
    r = []
    for i in range(14):
        x1, y1 = (torch.rand(2, generator=g) * torch.tensor([Ws, Hs]) * 0.8).tolist()
        w, h = (torch.rand(2, generator=g) * torch.tensor([Ws, Hs]) * 0.6 + 1).tolist()
        r.append([i % n_img, x1, y1, x1 + w, y1 + h])
    r += [[0, -0.3 * Ws, -0.2 * Hs, 0.3 * Ws, 0.25 * Hs], [1, 0.7 * Ws, 0.8 * Hs, 1.3 * Ws, 1.25 * Hs],   # partly outside
          [1, 5.0, 6.0, 5.0, 6.0], [0, 3.0, 2.0, 3.25, 40.0]]                                              # degenerate
    return torch.tensor(r, dtype=torch.float32)


def _roi_grads(feat, rois, out_size, scale, sr, go):
    f = feat.double().requires_grad_()
    R.roi_align(f, rois, out_size, scale, sr).backward(go.double())
    fa = feat.double().abs().requires_grad_()
    R.roi_align(fa, rois, out_size, scale, sr).backward(go.double().abs())
    return f.grad, fa.grad


@pytest.mark.parametrize("sr", [0, 2])
def test_roi_align_gradients_match_fp64(sr):
    feat = torch.randn(2, 16, 24, 40, generator=_gen(16))
    rois = _rois(2, 24, 40, 0.5, seed=17)
    fg = feat.to(DEV).requires_grad_()
    y = RoIAlign((7, 7), 0.5, sr)(fg, rois.to(DEV))
    go = torch.randn(y.shape, generator=_gen(18))
    y.backward(go.to(DEV))
    ref, mag = _roi_grads(feat, rois, (7, 7), 0.5, sr, go)
    _check(f"feat sr{sr}", fg.grad, ref, mag)
    # zero RoIs: an all-zero gradient
    fz = feat.to(DEV).requires_grad_()
    yz = roi_align(fz, torch.zeros(0, 5, device=DEV), (7, 7), 0.5, sr)
    assert yz.shape == (0, 16, 7, 7) and yz.grad_fn is not None
    yz.sum().backward()
    assert fz.grad is not None and (fz.grad == 0).all()


@pytest.mark.parametrize("P,dil", [(11, 1), (11, 2), (5, 1), (5, 2)])
def test_correlation_gradients_match_fp64(P, dil):
    g = _gen(19)
    a, b = torch.randn(2, 16, 12, 20, generator=g), torch.randn(2, 16, 12, 20, generator=g)
    ag, bg = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    y = spatial_correlation_sample(ag, bg, 1, P, 1, 0, 1, dil)
    go = torch.randn(y.shape, generator=g)
    y.backward(go.to(DEV))
    grads = []
    for on_abs in (False, True):
        a64, b64 = (a.abs() if on_abs else a).double().requires_grad_(), (b.abs() if on_abs else b).double().requires_grad_()
        R.correlation(a64, b64, P, dil).backward(go.abs().double() if on_abs else go.double())
        grads.append((a64.grad, b64.grad))
    _check("in1", ag.grad, grads[0][0], grads[1][0])
    _check("in2", bg.grad, grads[0][1], grads[1][1])


# ---- the forward is unchanged; no graph without a reason ----------------------------------------------------------------------------------
def test_forward_under_autograd_is_bit_identical_and_no_grad_fn_without_requires_grad():
    x, off, mask, _, _, _ = _dcn_case(2, 32, 32, 24, 40, (3, 3), (1, 1), (1, 1), (1, 1), 1, seed=20)
    x, off, mask = x.to(DEV), off.to(DEV), mask.to(DEV)
    rois = _rois(2, 24, 40, 1.0, seed=21).to(DEV)
    dcn2 = DCNv2(32, 32, 3, 1, 1).to(DEV)
    dcn = _dcn_module(32, 2, seed=22).to(DEV)
    v1 = DeformConv2d(32, 32, (3, 5), padding=(1, 2)).to(DEV)
    off15 = _offsets(2, 1, 3, 5, 24, 40, 24, 40, (1, 1), (1, 2), (1, 1), _gen(23)).to(DEV)
    calls = [lambda t: dcn2(t, off, mask), lambda t: dcn(t), lambda t: v1(t, off15), lambda t: roi_align(t, rois, (7, 7), 1.0, 0),
             lambda t: spatial_correlation_sample(t, t.flip(0), 1, 11, 1, 0, 1, 1)]
    for i, f in enumerate(calls):
        with torch.no_grad():
            y0 = f(x)
        y1 = f(x.clone().requires_grad_())
        assert y1.grad_fn is not None and torch.equal(y0, y1), i
    for p in list(dcn2.parameters()) + list(dcn.parameters()) + list(v1.parameters()):
        p.requires_grad_(False)
    for i, f in enumerate(calls):
        assert f(x).grad_fn is None, i


def test_deterministic_gradients_are_bit_equal_and_atomic_ones_agree():
    x, off, mask, w, b, go = _dcn_case(2, 64, 64, 24, 40, (3, 3), (1, 1), (1, 1), (1, 1), 1, seed=24)
    m = DCNv2(64, 64, 3, 1, 1).to(DEV)
    runs = []
    for _ in range(2):
        m.zero_grad()
        xg, og, mg = (t.to(DEV).requires_grad_() for t in (x, off, mask))
        m(xg, og, mg).backward(go.to(DEV))
        runs.append((xg.grad.clone(), og.grad.clone(), mg.grad.clone(), m.weight.grad.clone()))
    for i, name in ((1, "offset"), (2, "mask"), (3, "weight")):
        assert torch.equal(runs[0][i], runs[1][i]), name
    mag_x = _ref_grads(x, off, mask, m.weight.detach().cpu(), None, go, (1, 1), (1, 1), (1, 1), 1)[1]["x"]
    _check("grad_x run to run", runs[1][0], runs[0][0].cpu().double(), mag_x)
    a, c = torch.randn(1, 32, 24, 40, generator=_gen(25)).to(DEV), torch.randn(1, 32, 24, 40, generator=_gen(26)).to(DEV)
    cg = []
    for _ in range(2):
        ag, bg = a.clone().requires_grad_(), c.clone().requires_grad_()
        spatial_correlation_sample(ag, bg, patch_size=11).square().sum().backward()
        cg.append((ag.grad, bg.grad))
    assert torch.equal(cg[0][0], cg[1][0]) and torch.equal(cg[0][1], cg[1][1])
    feat = torch.randn(2, 16, 24, 40, generator=_gen(27))
    rois = _rois(2, 24, 40, 0.5, seed=28)
    gf = []
    for _ in range(2):
        fg = feat.to(DEV).requires_grad_()
        roi_align(fg, rois.to(DEV), (7, 7), 0.5, 0).sum().backward()
        gf.append(fg.grad.cpu())
    mag = _roi_grads(feat, rois, (7, 7), 0.5, 0, torch.ones(rois.shape[0], 16, 7, 7))[1]
    _check("grad_feat run to run", gf[1], gf[0].double(), mag)


# ---- a small net of the drop-ins trains as its fp64 restatement does ---------------------------------------------------------------------
class TinyNet(nn.Module):
    """conv -> DCN (stride 2) -> DeformConv2d 3x5 with offsets from a conv (FCB-ada-like) -> roi_align of a few boxes and the correlation of
    the two frames' features -> a scalar loss."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 16, 3, padding=1)
        self.dcn = DCN(16, 16, 3, 2, 1)
        self.off = nn.Conv2d(16, 30, 3, padding=1)
        self.fcb = DeformConv2d(16, 16, (3, 5), padding=(1, 2))
        g = _gen(29)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.6 / p[0].numel() ** 0.5 if p.dim() > 1 else 0.1))

    def forward(self, x, rois, seen=None):
        """seen=None: the drop-ins (GPU).  Otherwise fp64 restatements, the sample positions taken from the GPU run's recorded values."""
        h = torch.relu(self.conv(x))
        if seen is None:
            h = torch.relu(self.dcn(h))
            h = self.fcb(h, self.off(h))
            r = roi_align(h, rois, (3, 3), 0.5, 0)
            c = spatial_correlation_sample(h[0:1], h[1:2], patch_size=5)
        else:
            _, h = _dcn_fused_fp64(self.dcn, h, 2, seen["om"])
            h = torch.relu(h)
            off = self.off(h)
            off = off + (seen["off"].detach().cpu().double() - off).detach()
            h = R.deform_conv(h, off, None, self.fcb.weight, None, (1, 1), (1, 2), (1, 1), 1)
            r = R.roi_align(h, rois, (3, 3), 0.5, 0)
            c = R.correlation(h[0:1], h[1:2], 5, 1)
        return (r - 0.2).square().mean() + (c / 16 - 0.1).square().mean()


def test_training_end_to_end_matches_the_fp64_restatement():
    """3 SGD steps on the GPU and on the CPU in fp64 from the same weights.  Stated tolerances: every gradient within 1e-4 of its largest
    element, every parameter within 1e-5 * (1 + its largest element) after each step, the loss within 1e-5 relative."""
    net = TinyNet()
    net64 = copy.deepcopy(net).double()
    netg = net.to(DEV)
    om_cap, off_cap = _Capture(netg.dcn.conv_offset_mask), _Capture(netg.off)
    x = torch.randn(2, 3, 16, 24, generator=_gen(30))
    rois = torch.tensor([[0, 1.0, 2.0, 14.0, 12.0], [1, 4.0, 0.5, 20.0, 15.0], [0, -3.0, 8.0, 9.0, 19.0], [1, 10.0, 3.0, 26.0, 18.0]])
    opt, opt64 = torch.optim.SGD(netg.parameters(), lr=0.5), torch.optim.SGD(net64.parameters(), lr=0.5)
    losses = []
    for step in range(3):
        opt.zero_grad()
        opt64.zero_grad()
        loss = netg(x.to(DEV), rois.to(DEV))
        loss64 = net64(x.double(), rois, seen={"om": om_cap.out, "off": off_cap.out})
        loss.backward()
        loss64.backward()
        assert abs(loss.item() - loss64.item()) <= 1e-5 * abs(loss64.item()), step
        for (n, p), (_, p64) in zip(netg.named_parameters(), net64.named_parameters()):
            assert p.grad is not None, f"step {step}: {n} has no gradient"
            d = (p.grad.cpu().double() - p64.grad).abs().max().item()
            assert d <= 1e-4 * p64.grad.abs().max().item() + 1e-9, f"step {step}: {n}.grad differs by {d}"
        opt.step()
        opt64.step()
        for (n, p), (_, p64) in zip(netg.named_parameters(), net64.named_parameters()):
            d = (p.detach().cpu().double() - p64.detach()).abs().max().item()
            assert d <= 1e-5 * (1 + p64.detach().abs().max().item()), f"step {step}: {n} differs by {d} after the update"
        losses.append(loss.item())
    assert losses[2] < losses[1] < losses[0], losses


# ---- argument checks ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    x = torch.randn(1, 8, 12, 20, device=DEV, requires_grad=True)
    m2 = DCNv2(8, 8, 3, 1, 1).to(DEV)
    with pytest.raises(ValueError, match="channel count"):
        m2(x, torch.zeros(1, 16, 12, 20, device=DEV), torch.zeros(1, 9, 12, 20, device=DEV))
    v1 = DeformConv2d(8, 8, (3, 5), padding=(1, 2)).to(DEV)
    with pytest.raises(AssertionError, match="offset has"):
        v1(x, torch.zeros(1, 18, 12, 20, device=DEV))
    with pytest.raises(StmError, match="float32"):
        v1(x.double(), torch.zeros(1, 30, 12, 20, device=DEV, dtype=torch.float64))
    with pytest.raises(StmError, match="float32"):
        spatial_correlation_sample(x.double(), x.double(), patch_size=5)
    with pytest.raises(StmError, match="float32"):
        roi_align(x.double(), torch.zeros(1, 5, device=DEV), (7, 7))
    d = DCN(8, 8, 3, 1, 1).to(DEV)
    d.fuse_relu = True
    with pytest.raises(RuntimeError, match="inference-only"):
        d(x)
    with torch.no_grad():
        assert d(x).min().item() >= 0.0             # the fused path itself still serves inference
    torch.cuda.synchronize()


def test_sampler_module_form_has_gradients():
    s = SpatialCorrelationSampler(1, 5, 1, 0, 1, 1)
    a = torch.randn(1, 8, 6, 10, device=DEV, requires_grad=True)
    s(a, a.detach()).sum().backward()
    assert a.grad is not None and torch.isfinite(a.grad).all() and a.grad.abs().sum() > 0
