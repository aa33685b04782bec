"""Gradients of the drop-ins where test_gpu_autograd.py deliberately does not go: sample positions ON integers and ON the borders -1 / H / W (the
state every DCN starts from: DCN.init_offset() zeroes conv_offset_mask, and with padding 1 the outer taps of the border outputs sit on -1 and
H), correlation maps wider than one 64-column tile and patches too large for the LDS tile, RoIAlign with aligned=False and workgroup counts that
are no multiple of 8, and the ways autograd really calls the Functions (expanded and strided grad_out, channels_last, sliced offsets, B = 1,
subsets of needs_input_grad, accumulation, double backward).

Yardstick: autograd_restate.deform_conv_corners, the fp64 four-corner rule of DCNv2 / mmcv 1.x (pinned on the CPU by test_autograd_cpu.py,
hand-worked vector included); grid_sample is not a yardstick at integer positions.  Tolerance: test_gpu_autograd._check,
|g - g64| <= 1e-5 * sum|terms| + 1e-7 on every element, sum|terms| from the same yardstick on absolute values.  Lattice positions are built so
that base + offset is exact in fp32 (autograd_restate.position_classes asserts it), so kernel and yardstick sample at the very same point.
"""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

import autograd_restate as R
import oracle
from stmask_amd import autograd as A
from stmask_amd import ops
from stmask_amd.dcn_v2 import DCN, DCNv2
from stmask_amd.mmcv_ops import DeformConv2d, RoIAlign, roi_align
from stmask_amd.spatial_correlation_sampler import spatial_correlation_sample
from test_gpu_autograd import R50_DCN, _Capture, _check, _gen, _rois

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _out_hw(H, W, k, st, pad, dl):
    return (H + 2 * pad[0] - (dl[0] * (k[0] - 1) + 1)) // st[0] + 1, (W + 2 * pad[1] - (dl[1] * (k[1] - 1) + 1)) // st[1] + 1


def _corner_grads(x, off, mask, w, b, go, st, pad, dl, dg):
    """fp64 four-corner gradients and their sums of |terms|: (grads, mags), dicts over x / offset / mask / weight / bias."""
    def leaf(t):
        return t.detach().double().clone().requires_grad_()

    def run(xx, mm, ww, bb, gg):
        leaves = {"x": leaf(xx), "offset": leaf(off), "weight": leaf(ww)}
        if mm is not None:
            leaves["mask"] = leaf(mm)
        if bb is not None:
            leaves["bias"] = leaf(bb)
        y = R.deform_conv_corners(leaves["x"], leaves["offset"], leaves.get("mask"), leaves["weight"], leaves.get("bias"), st, pad, dl, dg)
        y.backward(gg.double())
        return {k: v.grad for k, v in leaves.items()}
    ref = run(x, mask, w, b, go)
    mag = run(x.abs(), None if mask is None else mask.abs(), w.abs(), None if b is None else b.abs(), go.abs())
    mag["offset"] = R.deform_conv_corners_offset_magnitude(x, off, mask, go, w, st, pad, dl, dg)
    return ref, mag


# ---- 1. a freshly constructed DCN ----------------------------------------------------------------------------------------------------------
def _dcn_step_compare(tag, mg, x, go, stride, padding=1, dilation=1, check_forward=False):
    """One forward / backward of the GPU module mg against the fp64 four-corner restatement of dcn_v2.DCN.forward with mg's parameters; the fp64
    conv_offset_mask output takes the GPU's fp32 value (captured), its graph stays fp64.  stride / padding / dilation: a number or a pair
    (conv_offset_mask is built without the dilation, as in dcn_v2).  check_forward: also hold y to the oracle (_check_forward).  Returns
    (grad_x, grad_weight, grad_bias, the fp64 om value)."""
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    st, pad, dl = pair(stride), pair(padding), pair(dilation)
    dg, n_off = mg.deformable_groups, 2 * mg.deformable_groups * mg.kernel_size[0] * mg.kernel_size[1]
    cap = _Capture(mg.conv_offset_mask)
    mg.zero_grad()
    xg = x.to(DEV).requires_grad_()
    y = mg(xg)
    y.backward(go.to(DEV))
    cw64, cb64, w64, b64 = (p.detach().cpu().double().requires_grad_() for p in (mg.conv_offset_mask.weight, mg.conv_offset_mask.bias, mg.weight,
                                                                                 mg.bias))
    x64 = x.double().requires_grad_()
    om = F.conv2d(x64, cw64, cb64, st, pad)
    om = om + (cap.out.detach().cpu().double() - om).detach()
    om.retain_grad()
    o1, o2, mk = torch.chunk(om, 3, dim=1)
    R.deform_conv_corners(x64, torch.cat((o1, o2), 1), torch.sigmoid(mk), w64, b64, st, pad, dl, dg).backward(go.double())
    omd = om.detach()
    s = torch.sigmoid(omd[:, n_off:])
    w, b = mg.weight.detach().cpu(), mg.bias.detach().cpu()
    if check_forward:
        _check_forward(tag, y, x, omd[:, :n_off].float(), s.float(), w, b, st, pad, dl, dg)
    _, mag = _corner_grads(x, omd[:, :n_off].float(), s.float(), w, b, go, st, pad, dl, dg)
    mag_om = torch.cat([mag["offset"], mag["mask"] * s * (1 - s)], 1)
    cw = cw64.detach()
    _check(f"{tag} om", cap.out.grad, om.grad, mag_om)
    # through torch's convolution backward applied to the om gradient: the bound carries |input| * bound(om), at 2e-5 as in test_gpu_autograd.py
    mag_cw = torch.nn.grad.conv2d_weight(x.double().abs(), cw.shape, mag_om, st, pad)
    _check(f"{tag} conv_offset_mask.weight", mg.conv_offset_mask.weight.grad, cw64.grad, mag_cw, rel=2e-5)
    _check(f"{tag} conv_offset_mask.bias", mg.conv_offset_mask.bias.grad, cb64.grad, mag_om.sum((0, 2, 3)), rel=2e-5)
    _check(f"{tag} weight", mg.weight.grad, w64.grad, mag["weight"])
    _check(f"{tag} bias", mg.bias.grad, b64.grad, mag["bias"])
    # x: the sampler's scatter (1e-5) plus the om gradient sent back through conv_offset_mask by torch (2e-5 of |cw|^T bound(om))
    mag_x = mag["x"] + 2.0 * torch.nn.grad.conv2d_input(x.shape, cw.abs(), mag_om, st, pad)
    _check(f"{tag} x", xg.grad, x64.grad, mag_x)
    return xg.grad, mg.weight.grad, mg.bias.grad, omd


@pytest.mark.parametrize("case", [dict(name=n, H=h, W=w, s=s, C=32) for n, h, w, s in R50_DCN] + [dict(name="L3.2 full width", H=12, W=20, s=1, C=512)],
                         ids=lambda c: c["name"])
def test_fresh_dcn_gradients_match_the_four_corner_rule_and_a_plain_convolution(case):
    """DCN exactly as constructed: conv_offset_mask is zero, every sample sits on an integer position, the outer taps of the border outputs on
    -1 and H / W, every mask is sigmoid(0) = 0.5.  All gradients against the four-corner yardstick; x / weight / bias also against fp64 autograd
    of 0.5 * conv2d(x, w) + bias, which involves no sampling code at all.  Then one SGD step (offsets become tiny and fractional) and the
    four-corner comparison again."""
    C, H, W, s = case["C"], case["H"], case["W"], case["s"]
    torch.manual_seed(31)
    m = DCN(C, C, 3, s, 1)
    assert not m.conv_offset_mask.weight.any() and not m.conv_offset_mask.bias.any()
    x = torch.randn(2, C, H, W, generator=_gen(32))
    mg = copy.deepcopy(m).to(DEV)
    Ho, Wo = _out_hw(H, W, (3, 3), (s, s), (1, 1), (1, 1))
    go = torch.randn(2, C, Ho, Wo, generator=_gen(33))
    gx, gw, gb, om = _dcn_step_compare("fresh", mg, x, go, s)
    assert not om.any()                                                 # the GPU's conv_offset_mask output was exactly zero
    # the second yardstick: a plain convolution
    grads = []
    for on_abs in (False, True):
        leaves = [(t.abs() if on_abs else t).double().requires_grad_() for t in (x, m.weight.detach(), m.bias.detach())]
        y = 0.5 * F.conv2d(leaves[0], leaves[1], None, s, 1) + leaves[2].view(1, C, 1, 1)
        y.backward(go.abs().double() if on_abs else go.double())
        grads.append([t.grad for t in leaves])
    for name, got, ref, mag in zip(("x", "weight", "bias"), (gx, gw, gb), *grads):
        _check(f"fresh vs conv2d {name}", got, ref, mag)
    # a learning rate that moves the largest conv_offset_mask weight by 1 / (36 C): every |om| stays below sum|x| / (36 C), a fraction of a pixel
    lr = 1.0 / (36 * C * mg.conv_offset_mask.weight.grad.abs().max().item())
    torch.optim.SGD(mg.parameters(), lr=lr).step()
    assert mg.conv_offset_mask.weight.any()
    om = _dcn_step_compare("after one step", mg, x, go, s)[3]
    assert om.any() and om[:, :18].abs().max() < 1.0                    # tiny, fractional offsets


def test_zero_om_with_dilation_2_matches_the_four_corner_rule_and_a_plain_convolution():
    """The fresh state at dilation 2.  dcn_v2.DCN builds conv_offset_mask without the dilation, so its output cannot have the deformable
    convolution's size at dilation 2 (as in the original package); the fused Function is fed a zero om directly."""
    C, H, W, st, pad, dl = 32, 24, 40, (1, 1), (2, 2), (2, 2)
    g = _gen(34)
    x, w, b = torch.randn(2, C, H, W, generator=g), torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5, torch.randn(C, generator=g)
    go = torch.randn(2, C, H, W, generator=g)
    om = torch.zeros(2, 27, H, W)
    leaves = [t.to(DEV).requires_grad_() for t in (x, om, w, b)]
    A.modulated_deform_conv_fused(*leaves, st, pad, dl, 1).backward(go.to(DEV))
    ref, mag = _corner_grads(x, om[:, :18], torch.full((2, 9, H, W), 0.5), w, b, go, st, pad, dl, 1)
    ref_om, mag_om = torch.cat([ref["offset"], ref["mask"] * 0.25], 1), torch.cat([mag["offset"], mag["mask"] * 0.25], 1)
    for name, got, r, mg_ in (("x", leaves[0].grad, ref["x"], mag["x"]), ("om", leaves[1].grad, ref_om, mag_om),
                              ("weight", leaves[2].grad, ref["weight"], mag["weight"]), ("bias", leaves[3].grad, ref["bias"], mag["bias"])):
        _check(f"dilation 2 {name}", got, r, mg_)
    grads = []
    for on_abs in (False, True):
        l64 = [(t.abs() if on_abs else t).double().requires_grad_() for t in (x, w, b)]
        (0.5 * F.conv2d(l64[0], l64[1], None, st, pad, dl) + l64[2].view(1, C, 1, 1)).backward(go.abs().double() if on_abs else go.double())
        grads.append([t.grad for t in l64])
    for name, got, r, mg_ in zip(("x", "weight", "bias"), (leaves[0].grad, leaves[2].grad, leaves[3].grad), *grads):
        _check(f"dilation 2 vs conv2d {name}", got, r, mg_)


# ---- 2. lattice positions -----------------------------------------------------------------------------------------------------------------
def _lattice_case(B, C, O, H, W, k, st, pad, dl, dg, seed, with_mask, with_bias):
    g = _gen(seed)
    off = R.lattice_offsets(B, dg, k[0], k[1], H, W, st, pad, dl, g)
    for axis, shares in zip("yx", R.position_classes(off, dg, k[0], k[1], H, W, st, pad, dl)):      # also asserts base + offset exact in fp32
        assert min(shares.values()) >= 0.01, (axis, shares)
    Ho, Wo = off.shape[-2:]
    x = torch.randn(B, C, H, W, generator=g)
    mask = torch.rand(B, dg * k[0] * k[1], Ho, Wo, generator=g) if with_mask else None
    w = torch.randn(O, C, *k, generator=g) / (C * k[0] * k[1]) ** 0.5
    b = torch.randn(O, generator=g) if with_bias else None
    go = torch.randn(B, O, Ho, Wo, generator=g)
    return x, off, mask, w, b, go


def _check_forward(name, y, x, off, mask, w, b, st, pad, dl, dg):
    """|y - oracle| <= 1e-5 * sum|terms| + 1e-6 (the oracle accumulates in double and returns fp32)."""
    ref = oracle.deform_conv(x, off, mask, w, b, st, pad, dl, dg)
    mag = oracle.deform_conv(x.abs(), off, None if mask is None else mask.abs(), w.abs(), None if b is None else b.abs(), st, pad, dl, dg)
    worst = ((y.detach().cpu().double() - ref.double()).abs() / (1e-5 * mag.double() + 1e-6)).max().item()
    assert worst <= 1.0, f"{name}: forward worst |y - oracle| / bound = {worst:.3f}"


LATTICE_V2 = [dict(k=(3, 3), s=1, d=1, dg=1, B=2), dict(k=(3, 3), s=2, d=1, dg=2, B=2), dict(k=(3, 3), s=1, d=2, dg=1, B=2),
              dict(k=(3, 3), s=1, d=1, dg=1, B=1)]


@pytest.mark.parametrize("case", LATTICE_V2, ids=lambda c: "k{k[0]}x{k[1]} s{s} d{d} dg{dg} B{B}".format(**c))
def test_dcnv2_gradients_on_lattice_positions(case):
    k, st, dl, dg, B = case["k"], (case["s"],) * 2, (case["d"],) * 2, case["dg"], case["B"]
    pad = dl
    x, off, mask, w, b, go = _lattice_case(B, 32, 32, 10, 12, k, st, pad, dl, dg, 41, True, True)
    m = DCNv2(32, 32, 3, st, pad, dl, dg).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    ref, mag = _corner_grads(x, off, mask, w, b, go, st, pad, dl, dg)
    runs = []
    for _ in range(2):
        m.zero_grad()
        xg, og, mg = (t.to(DEV).requires_grad_() for t in (x, off, mask))
        y = m(xg, og, mg)
        y.backward(go.to(DEV))
        runs.append((og.grad.clone(), mg.grad.clone(), m.weight.grad.clone()))
    _check_forward("DCNv2", y, x, off, mask, w, b, st, pad, dl, dg)
    for name, got in (("x", xg.grad), ("offset", og.grad), ("mask", mg.grad), ("weight", m.weight.grad), ("bias", m.bias.grad)):
        _check(f"DCNv2 lattice {name}", got, ref[name], mag[name])
    for i, name in enumerate(("offset", "mask", "weight")):
        assert torch.equal(runs[0][i], runs[1][i]), name


@pytest.mark.parametrize("case", LATTICE_V2[:3], ids=lambda c: "k{k[0]}x{k[1]} s{s} d{d} dg{dg}".format(**c))
def test_fused_dcn_gradients_on_lattice_positions(case):
    """The fused Function fed directly: om = (lattice offsets, mask logits); the sigmoid is the kernel's."""
    k, st, dl, dg = case["k"], (case["s"],) * 2, (case["d"],) * 2, case["dg"]
    pad = dl
    x, off, logit, w, b, go = _lattice_case(2, 32, 32, 10, 12, k, st, pad, dl, dg, 42, True, True)
    logit = (logit - 0.5) * 6
    om = torch.cat([off, logit], 1)
    s = torch.sigmoid(logit.double())
    ref, mag = _corner_grads(x, off, s, w, b, go, st, pad, dl, dg)
    ref_om = torch.cat([ref["offset"], ref["mask"] * s * (1 - s)], 1)
    mag_om = torch.cat([mag["offset"], mag["mask"] * s * (1 - s)], 1)
    runs = []
    for _ in range(2):
        leaves = [t.to(DEV).requires_grad_() for t in (x, om, w, b)]
        y = A.modulated_deform_conv_fused(*leaves, st, pad, dl, dg)
        y.backward(go.to(DEV))
        runs.append((leaves[1].grad, leaves[2].grad))
    _check_forward("fused DCN", y, x, off, s.float(), w, b, st, pad, dl, dg)
    for name, got, r, mg_ in (("x", leaves[0].grad, ref["x"], mag["x"]), ("om", leaves[1].grad, ref_om, mag_om),
                              ("weight", leaves[2].grad, ref["weight"], mag["weight"]), ("bias", leaves[3].grad, ref["bias"], mag["bias"])):
        _check(f"fused DCN lattice {name}", got, r, mg_)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("k", [(3, 3), (3, 5), (5, 3)])
@pytest.mark.parametrize("dg", [1, 2])
@pytest.mark.parametrize("stride", [1, 2])
def test_deform_conv2d_v1_gradients_on_lattice_positions(k, dg, stride):
    st, pad, dl = (stride, stride), (k[0] // 2, k[1] // 2), (1, 1)
    x, off, _, w, _, go = _lattice_case(2, 32, 32, 10, 12, k, st, pad, dl, dg, 43, False, False)
    m = DeformConv2d(32, 32, k, stride=stride, padding=pad, deform_groups=dg).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w)
    ref, mag = _corner_grads(x, off, None, w, None, go, st, pad, dl, dg)
    runs = []
    for _ in range(2):
        m.zero_grad()
        xg, og = x.to(DEV).requires_grad_(), off.to(DEV).requires_grad_()
        y = m(xg, og)
        y.backward(go.to(DEV))
        runs.append((og.grad.clone(), m.weight.grad.clone()))
    _check_forward("v1", y, x, off, None, w, None, st, pad, dl, dg)
    for name, got in (("x", xg.grad), ("offset", og.grad), ("weight", m.weight.grad)):
        _check(f"v1 lattice {name}", got, ref[name], mag[name])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---- 3. correlation backward: several tiles, odd channel counts, maps below the radius, the global-memory form -------------------------------
def _corr_lds_bytes(P, dil):
    """(grad_in1, grad_in2): P * P rows of 64 (+ 2R for grad_in2) floats; above 64 KB the kernel reads global memory instead."""
    return P * P * 64 * 4, P * P * (64 + 2 * (P // 2) * dil) * 4


CORR = [dict(B=1, C=32, H=6, W=64, P=11, dil=1), dict(B=1, C=32, H=6, W=65, P=11, dil=1), dict(B=2, C=32, H=5, W=80, P=11, dil=2),
        dict(B=1, C=32, H=4, W=130, P=11, dil=1), dict(B=1, C=1, H=6, W=20, P=11, dil=1), dict(B=1, C=6, H=6, W=70, P=5, dil=2),
        dict(B=1, C=9, H=7, W=65, P=11, dil=1), dict(B=1, C=256, H=6, W=80, P=11, dil=1), dict(B=1, C=32, H=3, W=5, P=11, dil=2),
        dict(B=3, C=9, H=6, W=20, P=11, dil=1), dict(B=1, C=8, H=20, W=70, P=17, dil=1, lds=(False, False)),
        dict(B=1, C=8, H=40, W=70, P=11, dil=7, lds=(True, True)), dict(B=1, C=6, H=40, W=70, P=11, dil=8, lds=(True, False))]


@pytest.mark.parametrize("case", CORR, ids=lambda c: "B{B} C{C} {H}x{W} P{P} dil{dil}".format(**c))
def test_correlation_gradients_tiles_channels_and_global_form(case):
    B, C, H, W, P, dil = (case[k] for k in ("B", "C", "H", "W", "P", "dil"))
    if "lds" in case:
        assert tuple(n <= 64 * 1024 for n in _corr_lds_bytes(P, dil)) == case["lds"]
    g = _gen(51)
    a, b = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    # the forward at this shape first (test_correlation_known_answers_and_generic_path's bound, times max(1, C / 64))
    fwd = ops.corr_patch(a.to(DEV), b.to(DEV), P, dil).cpu()
    err = (fwd - oracle.corr_patch(a, b, P, dil)).abs().max().item()
    assert err < 1e-5 * max(1.0, C / 64), f"forward: {err:.3e}"
    ag, bg = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    y = spatial_correlation_sample(ag, bg, 1, P, 1, 0, 1, dil)
    assert torch.equal(y.detach().cpu(), fwd)
    go = torch.randn(y.shape, generator=g)
    y.backward(go.to(DEV))
    grads = []
    for on_abs in (False, True):
        a64, b64 = (a.abs() if on_abs else a).double().requires_grad_(), (b.abs() if on_abs else b).double().requires_grad_()
        R.correlation(a64, b64, P, dil).backward(go.abs().double() if on_abs else go.double())
        grads.append((a64.grad, b64.grad))
    _check("in1", ag.grad, grads[0][0], grads[1][0])
    _check("in2", bg.grad, grads[0][1], grads[1][1])
    # only one input requiring grad: the bit-same tensor, nothing for the other
    a1, b1 = a.to(DEV).requires_grad_(), b.to(DEV)
    spatial_correlation_sample(a1, b1, 1, P, 1, 0, 1, dil).backward(go.to(DEV))
    assert torch.equal(a1.grad, ag.grad) and b1.grad is None
    a2, b2 = a.to(DEV), b.to(DEV).requires_grad_()
    spatial_correlation_sample(a2, b2, 1, P, 1, 0, 1, dil).backward(go.to(DEV))
    assert torch.equal(b2.grad, bg.grad) and a2.grad is None


# ---- 4. RoIAlign backward: aligned=False, other bins, samples on the borders, workgroup counts off the multiple of 8 ---------------------------
def _roi_grads(feat, rois, out_size, scale, sr, go, aligned):
    f = feat.double().requires_grad_()
    R.roi_align(f, rois, out_size, scale, sr, aligned).backward(go.double())
    fa = feat.double().abs().requires_grad_()
    R.roi_align(fa, rois, out_size, scale, sr, aligned).backward(go.double().abs())
    return f.grad, fa.grad


def _border_rois(n_img, H, W, PH, PW):
    """RoIs with integer corners, 2 * PH high and 2 * PW wide: with aligned=False, sampling_ratio 1 and scale 1 a bin is 2 wide and its one sample
    sits on start + 1 + 2 p.  The starts put the first sample on -1 or 0, or the last on H-1 or H (W-1 or W)."""
    r = []
    for i, (sy, sx) in enumerate(itertools.product((-2, -1, H - 2 * PH, H - 2 * PH + 1), (-2, -1, W - 2 * PW, W - 2 * PW + 1))):
        r.append([i % n_img, sx, sy, sx + 2 * PW, sy + 2 * PH])
    return torch.tensor(r, dtype=torch.float32)


ROI = [dict(out=(7, 3), sr=1, n=20, C=15, mod=1, border=True), dict(out=(1, 1), sr=1, n=22, C=96, mod=1, border=True),
       dict(out=(7, 3), sr=0, n=18, C=11, mod=1), dict(out=(7, 3), sr=3, n=18, C=10, mod=7), dict(out=(7, 7), sr=0, n=19, C=9, mod=1),
       dict(out=(1, 1), sr=3, n=21, C=280, mod=7), dict(out=(7, 7), sr=0, n=100, C=256, mod=4)]
# aligned=False throughout (it has no other gradient test); the workgroup tails also with aligned=True
ROI = [dict(c, aligned=False) for c in ROI] + [dict(c, aligned=True) for c in ROI if not c.get("border") and c["n"] != 100]


@pytest.mark.parametrize("case", ROI, ids=lambda c: "{out[0]}x{out[1]} sr{sr} n{n} C{C} aligned={aligned}".format(**c))
def test_roi_align_gradients_not_aligned_bins_borders_and_workgroup_tails(case):
    (PH, PW), sr, n, C, aligned = case["out"], case["sr"], case["n"], case["C"], case["aligned"]
    H, W, scale = 24, 40, 1.0 if case.get("border") else 0.5
    assert -(-n * C * PH * PW // 256) % 8 == case["mod"]                # workgroups: 8k+1, 8k+7 (the XCD remap's tail), one large case
    rois = _rois(2, H, W, scale, seed=61)
    if case.get("border"):
        rois = torch.cat([_border_rois(2, H, W, PH, PW), rois])
        ys = torch.cat([p[1] for p in R._roi_positions(rois[:16], PH, PW, scale, sr, aligned)])
        xs = torch.cat([p[2] for p in R._roi_positions(rois[:16], PH, PW, scale, sr, aligned)])
        for v, size in ((ys, H), (xs, W)):
            for target in (-1, 0, size - 1, size):
                assert (v == target).sum() >= 1, (target, size)
    while rois.shape[0] < n:
        rois = torch.cat([rois, _rois(2, H, W, scale, seed=62 + rois.shape[0])])
    rois = rois[:n]
    feat = torch.randn(2, C, H, W, generator=_gen(63))
    fg = feat.to(DEV).requires_grad_()
    y = RoIAlign((PH, PW), scale, sr, aligned=aligned)(fg, rois.to(DEV))
    ref_y = oracle.roi_align(feat, rois, (PH, PW), scale, sr, "avg", aligned)
    assert (y.detach().cpu() - ref_y).abs().max() < 1e-5                # test_roi_align_vs_oracle_and_known_answers' bound
    go = torch.randn(y.shape, generator=_gen(64))
    y.backward(go.to(DEV))
    ref, mag = _roi_grads(feat, rois, (PH, PW), scale, sr, go, aligned)
    _check("feat", fg.grad, ref, mag)


# ---- 5. how autograd really calls the Functions ---------------------------------------------------------------------------------------------
class _Op:
    """One drop-in with its inputs: fn(**tensors) -> y on the GPU; yardstick(go) -> (fp64 gradients, sums of |terms|) as dicts over the inputs;
    `atomic` = inputs whose gradient is a scatter of atomic adds (held to the run-to-run bound 1e-5 * sum|terms| + 1e-7; the others are
    deterministic and compared bit for bit)."""

    def __init__(self, name, inputs, fn, yardstick, atomic, no_grad=()):
        self.name, self.inputs, self.fn, self.yardstick, self.atomic, self.no_grad = name, inputs, fn, yardstick, atomic, no_grad
        self.names = [k for k in inputs if k not in no_grad]

    def run(self, req=None, go=None, inputs=None, backward=None):
        """-> (y, {name: grad or None}); req: names requiring grad (default all); go: grad_out (a CPU or GPU tensor)."""
        inputs = inputs or self.inputs
        req = self.names if req is None else req
        leaves = {k: v.to(DEV).clone().requires_grad_(k in req) for k, v in inputs.items()}
        y = self.fn(**leaves)
        if backward is not None:
            backward(y)
        else:
            y.backward(go.to(DEV))
        return y, {k: leaves[k].grad for k in self.names}

    def same(self, what, got, base, mag, factor=1.0):
        for k in self.names:
            if base[k] is None:
                assert got[k] is None, f"{self.name} {what}: {k} has a gradient nobody asked for"
            elif k in self.atomic:
                _check(f"{self.name} {what} {k}", got[k], base[k].cpu().double() * factor, mag[k] * factor)
            else:
                assert got[k] is not None and torch.equal(got[k], base[k] * factor), f"{self.name} {what}: {k} is not bit-equal"


def _ops():
    g = _gen(71)
    st, pad, dl = (1, 1), (1, 1), (1, 1)
    B, C, H, W = 2, 32, 10, 12
    x, off, mask, w, b, _ = _lattice_case(B, C, C, H, W, (3, 3), st, pad, dl, 1, 72, True, True)
    off = torch.where(torch.rand(off.shape, generator=g) < 0.5, off, torch.round(torch.randn(off.shape, generator=g) * 2048) / 1024)
    R.position_classes(off, 1, 3, 3, H, W, st, pad, dl)                # base + offset exact in fp32
    logit = (mask - 0.5) * 6
    sg = torch.sigmoid(logit.double())
    off15 = R.lattice_offsets(B, 1, 3, 5, H, W, st, (1, 2), dl, g)
    w15 = torch.randn(C, C, 3, 5, generator=g) / (15 * C) ** 0.5
    feat = torch.randn(2, 16, 24, 40, generator=g)
    rois = _rois(2, 24, 40, 0.5, seed=73)
    f1, f2 = torch.randn(B, 12, 9, 70, generator=g), torch.randn(B, 12, 9, 70, generator=g)

    def fused_yardstick(go):
        ref, mag = _corner_grads(x, off, sg, w, b, go, st, pad, dl, 1)
        return tuple(dict(x=d["x"], om=torch.cat([d["offset"], d["mask"] * sg * (1 - sg)], 1), weight=d["weight"], bias=d["bias"]) for d in (ref, mag))

    def roi_yardstick(go):
        return tuple(dict(input=t) for t in _roi_grads(feat, rois, (7, 7), 0.5, 2, go, True))

    def corr_yardstick(go):
        out = []
        for on_abs in (False, True):
            a64, b64 = ((t.abs() if on_abs else t).double().requires_grad_() for t in (f1, f2))
            R.correlation(a64, b64, 11, 1).backward(go.abs().double() if on_abs else go.double())
            out.append(dict(input1=a64.grad, input2=b64.grad))
        return tuple(out)

    return [
        _Op("DCNv2", dict(x=x, offset=off, mask=mask, weight=w, bias=b),
            lambda x, offset, mask, weight, bias: A.modulated_deform_conv(x, offset, mask, weight, bias, st, pad, dl, 1),
            lambda go: _corner_grads(x, off, mask, w, b, go, st, pad, dl, 1), atomic=("x",)),
        _Op("fused DCN", dict(x=x, om=torch.cat([off, logit], 1), weight=w, bias=b),
            lambda x, om, weight, bias: A.modulated_deform_conv_fused(x, om, weight, bias, st, pad, dl, 1), fused_yardstick, atomic=("x",)),
        _Op("DeformConv2d v1", dict(x=x, offset=off15, weight=w15),
            lambda x, offset, weight: A.deform_conv(x, offset, weight, st, (1, 2), dl, 1),
            lambda go: _corner_grads(x, off15, None, w15, None, go, st, (1, 2), dl, 1), atomic=("x",)),
        _Op("roi_align", dict(input=feat, rois=rois), lambda input, rois: roi_align(input, rois, (7, 7), 0.5, 2), roi_yardstick,
            atomic=("input",), no_grad=("rois",)),
        _Op("correlation", dict(input1=f1, input2=f2), lambda input1, input2: spatial_correlation_sample(input1, input2, 1, 11, 1, 0, 1, 1),
            corr_yardstick, atomic=()),
    ]


@pytest.mark.parametrize("i", range(5), ids=["DCNv2", "fused DCN", "DeformConv2d v1", "roi_align", "correlation"])
def test_calling_conventions_of_autograd(i):
    op = _ops()[i]
    with torch.no_grad():
        shape = op.fn(**{k: v.to(DEV) for k, v in op.inputs.items()}).shape
    go = torch.randn(shape, generator=_gen(74))
    ones, mean = torch.ones(shape), torch.full(shape, 1.0 / go.numel())
    (ref, mag), mag1 = op.yardstick(go), op.yardstick(ones)[1]
    magm = {k: v / go.numel() for k, v in mag1.items()}                 # sums of |terms| are linear in |grad_out|
    y0, base = op.run(go=go)
    for k in op.names:                                                 # the dense, contiguous call itself is right
        _check(f"{op.name} {k}", base[k], ref[k], mag[k])
    # an expanded (stride-0) grad_out: y.sum() and y.mean()
    op.same("y.sum()", op.run(backward=lambda y: y.sum().backward())[1], op.run(go=ones)[1], mag1)
    op.same("y.mean()", op.run(backward=lambda y: y.mean().backward())[1], op.run(go=mean)[1], magm)
    # grad_out in another memory layout: channels_last (channels_last_3d for the 5-D correlation), and a transposed view
    gd = go.to(DEV)
    cl = gd.contiguous(memory_format=torch.channels_last if gd.dim() == 4 else torch.channels_last_3d)
    tv = gd.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not tv.is_contiguous() and (not cl.is_contiguous() or cl.shape[1] == 1)
    op.same("channels_last grad_out", op.run(go=cl)[1], base, mag)
    op.same("transposed grad_out", op.run(go=tv)[1], base, mag)
    # the first input in channels_last
    first = op.names[0]
    xcl = op.inputs[first].to(DEV).contiguous(memory_format=torch.channels_last)
    assert not xcl.is_contiguous()
    ycl, gcl = op.run(go=go, inputs=dict(op.inputs, **{first: xcl}))
    assert torch.equal(ycl, y0)
    op.same(f"channels_last {first}", gcl, base, mag)
    # two backward passes over one graph accumulate: exactly twice the deterministic gradients
    def twice(y):
        y.backward(gd, retain_graph=True)
        y.backward(gd)
    op.same("two backward passes", op.run(backward=twice)[1], base, mag, factor=2.0)
    # every subset of the inputs requiring grad: what is asked for is the all-on run's, the rest is None
    for r in range(1, len(op.names)):
        for req in itertools.combinations(op.names, r):
            got = op.run(req=req, go=go)[1]
            op.same(f"requires_grad only on {req}", got, {k: (base[k] if k in req else None) for k in op.names}, mag)


def test_offsets_and_masks_that_are_slices_of_wider_tensors():
    """offset = t[:, a:b] of a wider tensor (a channel slice is not contiguous across the batch): the same gradients, and zero elsewhere in t."""
    dcn2, _, v1 = _ops()[:3]
    for op, parts in ((dcn2, ("offset", "mask")), (v1, ("offset",))):
        shape = op.run(go=None, backward=lambda y: None)[0].shape
        go = torch.randn(shape, generator=_gen(75))
        _, mag = op.yardstick(go)
        base = op.run(go=go)[1]
        wide = {k: torch.cat([torch.randn(v.shape[0], 3, *v.shape[2:]), v, torch.randn(v.shape[0], 2, *v.shape[2:])], 1).to(DEV).requires_grad_()
                for k, v in op.inputs.items() if k in parts}
        leaves = {k: (wide[k][:, 3:3 + v.shape[1]] if k in parts else v.to(DEV).requires_grad_()) for k, v in op.inputs.items()}
        assert not leaves["offset"].is_contiguous()
        op.fn(**leaves).backward(go.to(DEV))
        got = {k: (wide[k].grad[:, 3:3 + v.shape[1]] if k in parts else leaves[k].grad) for k, v in op.inputs.items()}
        op.same("sliced", got, base, mag)
        for k in parts:
            n = op.inputs[k].shape[1]
            assert not wide[k].grad[:, :3].any() and not wide[k].grad[:, 3 + n:].any()


# ---- 6. second order is refused, not dropped -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(5), ids=["DCNv2", "fused DCN", "DeformConv2d v1", "roi_align", "correlation"])
def test_double_backward_raises(i):
    """The backward kernels have no derivative: differentiating a gradient made with create_graph=True must raise, not return a result with the
    second-order term silently missing.  Three forms: the gradient of y.sum() on its own; the gradient of a nonlinear loss (grad_out then depends
    on the inputs); and the gradient of y.sum() times the input, where only the saved tensors carry the dependence (grad_x depends on the weight
    and the offsets) -- RoIAlign is linear in its one differentiable input, so there that last form has no second-order term to drop."""
    op = _ops()[i]

    def grad_of(loss):
        leaves = {k: v.to(DEV).clone().requires_grad_(k not in op.no_grad) for k, v in op.inputs.items()}
        first = leaves[op.names[0]]
        (gx,) = torch.autograd.grad(loss(op.fn(**leaves)), first, create_graph=True)
        return gx, first

    gx, first = grad_of(lambda y: y.sum())
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    gx, first = grad_of(lambda y: y.square().sum())
    with pytest.raises(RuntimeError, match="not differentiable"):
        (gx * first.detach()).sum().backward()
    if op.name != "roi_align":
        gx, first = grad_of(lambda y: y.sum())
        with pytest.raises(RuntimeError, match="not differentiable"):
            (gx * first).sum().backward()
