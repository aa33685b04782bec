"""The drop-in ops at UNEQUAL stride / padding / dilation pairs, spatial scales and patch sizes (tests/geometry_cases.py): every kernel form
that works out `ho*sh - ph + i*dh` and `wo*sw - pw + j*dw` for itself -- the three im2col variants and the automatic dispatch, the planar
samplers in their register-gather and LDS-staged forms, the fused deformable convolution, col2im and col2im_coord behind the modules' backward
-- against the CPU oracle and the fp64 restatements, which test_geometry_cpu.py holds to each other at the same cases.  Every other GPU test of
these ops passes sh == sw, dh == dw and "same" padding; a form that took one axis' value for the other's passes them all
(test_geometry_cpu.test_every_unequal_pair_is_told_apart shows that these inputs would not let it).  With them RoIAlign over three images at
four spatial scales and bin shapes, and correlation patches from 1 to 21 at patch dilations 1 to 3.

No tolerance is new.  Each is the one an existing test applies to the same quantity; the source is named where it is used.
"""
import ctypes

import pytest
import torch

import geometry_cases as G
import oracle
from stmask_amd import _lib, ops
from stmask_amd._lib import DeformGeom, StmError, c_f, c_i, c_p
from stmask_amd.dcn_v2 import DCN, DCNv2
from stmask_amd.mmcv_ops import DeformConv2d, RoIAlign, roi_align
from stmask_amd.spatial_correlation_sampler import SpatialCorrelationSampler, spatial_correlation_sample
from test_gpu_autograd import _Capture, _check, _gen
from test_gpu_autograd_edges import _check_forward, _corner_grads, _dcn_step_compare, _roi_grads
from test_gpu_dcn_fused import fused
import autograd_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _d(t):
    return None if t is None else t.to(DEV)


# ---- (a) stm_deform_im2col_f32: variants 1, 2, 3 and the automatic dispatch ---------------------------------------------------------------------
@pytest.mark.parametrize("c", G.DEFORM_CASES, ids=G.case_id)
def test_deform_im2col_variants_at_unequal_pairs(c):
    """With mask, without, and with DCN's raw conv_offset_mask logits.  Each variant against the oracle's columns: < 2e-5 absolute on O(1) data
    (test_deform_im2col_vs_oracle); the variants among themselves: bit-equal (test_deform_im2col_variants_agree_bitwise) -- also where a forced
    variant falls back (C/dg % 4 != 0 takes the direct kernel, variant 3 without 16-byte rows takes variant 2's kernel)."""
    x, off, mask, _, _, _ = G.deform_inputs(c)
    logit = torch.randn(mask.shape, generator=_gen(c["seed"] + 7)) * 1.5
    geom = (c["k"], c["st"], c["pad"], c["dl"], c["dg"])
    for mode, m_ref, kwargs in (("mask", mask, dict(offset=_d(off), mask=_d(mask))), ("no mask", None, dict(offset=_d(off), mask=None)),
                                ("fused om", torch.sigmoid(logit), dict(offset=None, mask=None, fused_om=_d(torch.cat([off, logit], 1))))):
        ref = oracle.deform_im2col(x, off, m_ref, *geom)
        got = {v: ops.deform_im2col(_d(x), kwargs["offset"], kwargs["mask"], *geom, variant=v, fused_om=kwargs.get("fused_om")) for v in (1, 2, 3, 0)}
        for v, cols in got.items():
            assert cols.shape == ref.shape, (mode, v)
            err = (cols.cpu() - ref).abs().max().item()
            print(f"{c['name']} {mode} variant {v}: max |col - oracle| = {err:.3e}")
            assert err < 2e-5, (mode, v, err)
        for v in (2, 3, 0):
            assert torch.equal(got[1], got[v]), (mode, v)


# ---- (b), (c) the modules, built with the pair arguments: forward and all gradients ----------------------------------------------------------------
def _check_grads(tag, got, ref, mag):
    """test_gpu_autograd._check on every gradient: |g - g64| <= 1e-5 * sum|terms| + 1e-7."""
    for name, g in got.items():
        _check(f"{tag} {name}", g, ref[name], mag[name])


@pytest.mark.parametrize("c", G.DEFORM_CASES, ids=G.case_id)
def test_dcnv2_module_forward_and_gradients(c):
    """dcn_v2.DCNv2(stride=(sh, sw), padding=(ph, pw), dilation=(dh, dw)): the forward within test_gpu_autograd_edges._check_forward's bound of the
    oracle, the five gradients within test_gpu_autograd._check's bound of the four-corner restatement (these offsets include integer and border
    positions), and the deterministic ones bit-equal over two runs (as test_dcnv2_gradients_on_lattice_positions)."""
    x, off, mask, w, b, go = G.deform_inputs(c)
    args = (c["st"], c["pad"], c["dl"], c["dg"])
    m = DCNv2(c["C"], c["O"], c["k"], *args).to(DEV)
    assert (m.stride, m.padding, m.dilation) == (c["st"], c["pad"], c["dl"])
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    ref, mag = _corner_grads(x, off, mask, w, b, go, *args)
    runs = []
    for _ in range(2):
        m.zero_grad()
        xg, og, mg = (t.to(DEV).requires_grad_() for t in (x, off, mask))
        y = m(xg, og, mg)
        y.backward(go.to(DEV))
        runs.append((og.grad.clone(), mg.grad.clone(), m.weight.grad.clone()))
    _check_forward(c["name"], y, x, off, mask, w, b, *args)
    with torch.no_grad():
        assert torch.equal(m(_d(x), _d(off), _d(mask)), y)                                  # the no-grad launch: the same values
    _check_grads(c["name"], dict(x=xg.grad, offset=og.grad, mask=mg.grad, weight=m.weight.grad, bias=m.bias.grad), ref, mag)
    for i, name in enumerate(("offset", "mask", "weight")):
        assert torch.equal(runs[0][i], runs[1][i]), name


@pytest.mark.parametrize("c", G.DEFORM_CASES, ids=G.case_id)
def test_deform_conv2d_module_forward_and_gradients(c):
    """mmcv.ops.DeformConv2d (no mask, no bias) with the pair arguments: bounds and determinism as test_deform_conv2d_v1_gradients_on_lattice_positions."""
    x, off, _, w, _, go = G.deform_inputs(c, with_mask=False, with_bias=False)
    args = (c["st"], c["pad"], c["dl"], c["dg"])
    m = DeformConv2d(c["C"], c["O"], c["k"], stride=c["st"], padding=c["pad"], dilation=c["dl"], deform_groups=c["dg"]).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w)
    ref, mag = _corner_grads(x, off, None, w, None, go, *args)
    runs = []
    for _ in range(2):
        m.zero_grad()
        xg, og = x.to(DEV).requires_grad_(), off.to(DEV).requires_grad_()
        y = m(xg, og)
        y.backward(go.to(DEV))
        runs.append((og.grad.clone(), m.weight.grad.clone()))
    _check_forward(c["name"], y, x, off, None, w, None, *args)
    _check_grads(c["name"], dict(x=xg.grad, offset=og.grad, weight=m.weight.grad), ref, mag)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def _dcn_can_run(c):
    """dcn_v2.DCN builds conv_offset_mask without the dilation (as the original package): its output has the deformable convolution's size only
    where, per axis, the dilation is 1 or the kernel has one tap.  The other cases are refused (test_refusals_...)."""
    return all(d == 1 or k == 1 for d, k in zip(c["dl"], c["k"]))


DCN_CASES = [c for c in G.DEFORM_CASES if _dcn_can_run(c)]
DCN_REFUSED = [c for c in G.DEFORM_TABLE if not _dcn_can_run(c)]


@pytest.mark.parametrize("c", DCN_CASES, ids=G.case_id)
def test_dcn_module_forward_and_gradients(c):
    """dcn_v2.DCN with a randomised conv_offset_mask (offsets of scale 2, as the other cases'): test_gpu_autograd_edges._dcn_step_compare, the helper
    of the fresh-DCN test, with the pair arguments -- forward, the gradient w.r.t. the raw conv_offset_mask output, the parameters of both
    layers and x, at that helper's own bounds.  Two runs: the om and weight gradients bit-equal."""
    g = _gen(c["seed"] + 11)
    K = c["k"][0] * c["k"][1]
    m = DCN(c["C"], c["O"], c["k"], c["st"], c["pad"], c["dl"], c["dg"])
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g) / (c["C"] * K) ** 0.5)
        m.bias.copy_(torch.randn(c["O"], generator=g))
        m.conv_offset_mask.weight.copy_(torch.randn(m.conv_offset_mask.weight.shape, generator=g) * 2.0 / (c["C"] * K) ** 0.5)
        m.conv_offset_mask.bias.copy_(torch.randn(m.conv_offset_mask.bias.shape, generator=g))
    m = m.to(DEV)
    cap = _Capture(m.conv_offset_mask)
    x = torch.randn(c["B"], c["C"], c["H"], c["W"], generator=g)
    go = torch.randn(c["B"], c["O"], *G.out_hw(c), generator=g)
    runs = []
    for _ in range(2):
        _, gw, _, om = _dcn_step_compare(c["name"], m, x, go, c["st"], c["pad"], c["dl"], check_forward=True)
        runs.append((cap.out.grad.clone(), gw.clone()))
    assert om[:, :2 * c["dg"] * K].std() > 0.5                                             # offsets that move the samples
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---- (d) the planar samplers ------------------------------------------------------------------------------------------------------------------------
def _planar_inputs(c, scale=1.5):
    g = _gen(c["C"] + c["H"])
    Ho, Wo = G.out_hw(c)
    x = torch.randn(c["B"], c["C"], c["H"], c["W"], generator=g)
    om = torch.randn(c["B"], 27, Ho, Wo, generator=g) * scale
    return x, om, Ho, Wo


@pytest.mark.parametrize("c", G.PLANAR_CASES, ids=G.case_id)
def test_dcn_sample_planar_equals_im2col_at_unequal_pairs(c, tunables):
    """dcn_sample_planar in formats 0, 1, 2 and through the `_f16` entry: bit-equal to the im2col columns rearranged to [pixel, tap*C + c] and split
    (the property of test_dcn_sample_planar_equals_im2col); the columns themselves within 2e-5 of the oracle (same test).  Then with
    STM_DCN_LDS=1, whose launcher takes only dh == dw == 1 and sh == sw in {1, 2}: the cases it takes and the cases it must decline both equal
    the register-gather planes bit for bit (test_dcn_sample_planar_lds_form_equals_register_gather), with offsets inside its halo and far
    outside it."""
    B, C = c["B"], c["C"]
    geom = (c["st"], c["pad"], c["dl"])
    for scale in (1.5, 6.0):
        x, om, Ho, Wo = _planar_inputs(c, scale)
        cols = ops.deform_im2col(_d(x), None, None, 3, *geom, 1, fused_om=_d(om))                                      # [B, C*9, Ho*Wo]
        o_cols = oracle.deform_im2col(x, om[:, :18].contiguous(), torch.sigmoid(om[:, 18:]), 3, *geom, 1)
        assert (cols.cpu() - o_cols).abs().max().item() < 2e-5
        ref = cols.view(B, C, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, 9 * C).contiguous()               # [pixel, k*C + c]
        x_nhwc, om_pix = _d(x.permute(0, 2, 3, 1).contiguous()), _d(om.permute(0, 2, 3, 1).reshape(-1, 27).contiguous())
        tunables.set(STM_DCN_LDS="0")
        planes = {fmt: ops.dcn_sample_planar(x_nhwc, om_pix, *geom, fmt=fmt) for fmt in (0, 1, 2)}
        assert planes[0].shape == (3, 9 * C // 32, B * Ho * Wo, 32)
        assert torch.equal(ops.planes_to_f32(planes[0]), ref)
        for fmt in (1, 2):
            assert torch.equal(planes[fmt], ops.split_planes(ref, fmt=fmt).view_as(planes[fmt])), fmt
        f16 = torch.empty_like(planes[2])
        geo = DeformGeom(B, C, c["H"], c["W"], 3, 3, *c["st"], *c["pad"], *c["dl"], 1, Ho, Wo)
        _lib.check(_lib.lib().stm_dcn_sample_planar_f16(c_p(x_nhwc.data_ptr()), c_p(om_pix.data_ptr()), c_i(27), c_p(f16.data_ptr()), c_i(B * Ho * Wo),
                                                        ctypes.c_longlong(0), ctypes.byref(geo), ops._stream()), "stm_dcn_sample_planar_f16")
        assert torch.equal(f16, planes[2])
        tunables.set(STM_DCN_LDS="1")
        for fmt in (0, 1, 2):
            assert torch.equal(ops.dcn_sample_planar(x_nhwc, om_pix, *geom, fmt=fmt), planes[fmt]), ("STM_DCN_LDS=1", fmt, c["lds"])
        tunables.clear("STM_DCN_LDS")


@pytest.mark.parametrize("c", G.SAMPLE_PLANAR_CASES, ids=lambda c: "k{k[0]}x{k[1]}_p{pad[0]}{pad[1]}".format(**c))
def test_deform_sample_planar_equals_im2col_with_padding_above_same(c, tunables):
    """deform_sample_planar (mask-free, stride 1, dilation 1, H x W outputs) with unequal padding above "same": the first H x W outputs of the
    deformable convolution with that padding, so bit-equal to those im2col columns rearranged and split
    (test_deform_sample_planar_mask_free_equals_im2col's property); register-gather and LDS-staged form."""
    B, C, H, W = 2, 256, 7, 9
    (kh, kw), (ph, pw) = c["k"], c["pad"]
    K = kh * kw
    Hf, Wf = H + 2 * ph - kh + 1, W + 2 * pw - kw + 1
    assert Hf >= H and Wf >= W and (Hf, Wf) != (H, W)
    g = _gen(kh * 10 + pw)
    x = torch.randn(B, C, H, W, generator=g)
    off = torch.randn(B, 2 * K, H, W, generator=g) * 1.5
    off_full = torch.zeros(B, 2 * K, Hf, Wf)
    off_full[:, :, :H, :W] = off
    cols = ops.deform_im2col(_d(x), _d(off_full), None, (kh, kw), 1, (ph, pw), 1, 1).view(B, C, K, Hf, Wf)[:, :, :, :H, :W]
    o_cols = oracle.deform_im2col(x, off_full, None, (kh, kw), 1, (ph, pw), 1, 1).view(B, C, K, Hf, Wf)[:, :, :, :H, :W]
    assert (cols.cpu() - o_cols).abs().max().item() < 2e-5
    ref = cols.reshape(B, C, K, H * W).permute(0, 3, 2, 1).reshape(B * H * W, K * C).contiguous()
    x_pix = _d(x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous())
    off_pix = _d(off.permute(0, 2, 3, 1).reshape(B * H * W, 2 * K).contiguous())
    for lds in ("0", "1"):
        tunables.set(STM_DCN_LDS=lds)
        for fmt in (0, 1):
            out = torch.zeros(ops.plane_layout(fmt)[0], K * C // 32, B * H * W, 32, device=DEV, dtype=ops.plane_layout(fmt)[1])
            ops.deform_sample_planar(x_pix, B, H, W, C, off_pix, (kh, kw), (ph, pw), out, 0, fmt)
            assert torch.equal(out, ops.split_planes(ref, fmt=fmt).view_as(out)), (lds, fmt)
    tunables.clear("STM_DCN_LDS")


# ---- (e) the fused deformable convolution -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.FUSED_CASES, ids=G.case_id)
def test_fused_deform_conv_at_unequal_pairs(c, tunables):
    """stm_deform_conv_fused_planar_f32 against the oracle: |y - ref| / (mag + 1e-3) < 4e-6 in the fp16 x 2 format
    (test_fused_deform_conv_vs_oracle_and_pair) and < 1e-3 in the fp16 x 1 format (test_fused_deform_conv_planes_formats: one plane holds 11
    bits); 64 x 256 tiles and, with STM_DCN_FUSED_WIDE=0, 128 x 128 tiles: bit-equal (test_fused_deform_conv_wide_tiles_equal_narrow_tiles)."""
    x, off, mask, w, b, _ = G.deform_inputs(c)
    wm, O = c["mask"], c["O"]
    logit = torch.randn(mask.shape, generator=_gen(c["seed"] + 7))
    m_ref = torch.sigmoid(logit) if wm else None
    om = torch.cat([off, logit], 1) if wm else off
    bias = b if wm else None
    geom = (c["st"], c["pad"], c["dl"], 1)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, O)
    ref = flat(oracle.deform_conv(x, off, m_ref, w, bias, *geom))
    mag = flat(oracle.deform_conv(x.abs(), off, m_ref, w.abs(), None if bias is None else bias.abs(), *geom))
    for fmt, tol in ((1, 4e-6), (2, 1e-3)):
        tunables.clear("STM_DCN_FUSED_WIDE")
        n0 = _lib.lib().stm_debug_launch_count(1)
        wide = fused(x, om, w, bias, c["st"], c["pad"], wm, False, fmt=fmt, dil=c["dl"])
        assert _lib.lib().stm_debug_launch_count(1) == n0 + 1
        assert wide.shape == ref.shape
        err = ((wide - ref).abs() / (mag + 1e-3)).max().item()
        print(f"{c['name']} fmt {fmt}: max |y - oracle| / (mag + 1e-3) = {err:.3e}")
        assert err < tol, (fmt, err)
        tunables.set(STM_DCN_FUSED_WIDE=0)
        narrow = fused(x, om, w, bias, c["st"], c["pad"], wm, False, fmt=fmt, dil=c["dl"])
        assert torch.equal(wide, narrow), fmt
    tunables.clear("STM_DCN_FUSED_WIDE")


# ---- (f) RoIAlign ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.roi_cases(), ids=G.case_id)
def test_roi_align_scales_bins_and_images(c):
    """mmcv_ops.roi_align and the RoIAlign module over three images (every batch index, rows not sorted by image), spatial_scale 0.25 .. 2, four bin
    shapes, sampling_ratio 0 .. 4, aligned or not.  Forward against oracle.roi_align: < 1e-5 (test_roi_align_vs_oracle_and_known_answers);
    backward against the restatement under test_gpu_autograd._check, as test_roi_align_gradients_not_aligned_bins_borders_and_workgroup_tails."""
    feat = torch.randn(G.ROI_B, c["C"], G.ROI_H, G.ROI_W, generator=_gen(81))
    rois = G.rois(c["scale"])
    ref = oracle.roi_align(feat, rois, c["out"], c["scale"], c["sr"], "avg", c["aligned"])
    with torch.no_grad():
        y0 = roi_align(_d(feat), _d(rois), c["out"], c["scale"], c["sr"], "avg", c["aligned"])
    err = (y0.cpu() - ref).abs().max().item()
    print(f"{c['name']}: max |y - oracle| = {err:.3e}")
    assert y0.shape == ref.shape and err < 1e-5
    # each image's RoIs alone, against that image alone: the batch index addresses the image it names
    for b in range(G.ROI_B):
        sel = rois[:, 0] == b
        alone = rois[sel].clone()
        alone[:, 0] = 0
        with torch.no_grad():
            assert torch.equal(roi_align(_d(feat[b:b + 1]), _d(alone), c["out"], c["scale"], c["sr"], "avg", c["aligned"]), y0[_d(sel)]), b
    fg = feat.to(DEV).requires_grad_()
    y = RoIAlign(c["out"], c["scale"], c["sr"], aligned=c["aligned"])(fg, _d(rois))
    assert torch.equal(y.detach(), y0)
    go = torch.randn(y.shape, generator=_gen(82))
    y.backward(go.to(DEV))
    g64, mag = _roi_grads(feat, rois, c["out"], c["scale"], c["sr"], go, c["aligned"])
    _check(f"{c['name']} feat", fg.grad, g64, mag)


# ---- (g) correlation ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.CORR_CASES, ids=G.case_id)
def test_correlation_patch_sizes_and_dilations(c):
    """spatial_correlation_sample at patch sizes 1 .. 21 and patch dilations 1 .. 3, NCHW and channels_last inputs.  Forward against the oracle:
    < 1e-5 (test_correlation_known_answers_and_generic_path, the bound of every patch size but 11; test_correlation_vs_oracle's 1e-4 * max(1, C / 64)
    is implied); gradients under test_gpu_autograd._check as test_correlation_gradients_tiles_channels_and_global_form; the channels_last
    call gives the same bits (test_calling_conventions_of_autograd)."""
    B, C, H, W, P, dil = (c[k] for k in ("B", "C", "H", "W", "P", "dil"))
    g = _gen(91)
    a, b = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    ref = oracle.corr_patch(a, b, P, dil)
    with torch.no_grad():
        y0 = spatial_correlation_sample(_d(a), _d(b), 1, P, 1, 0, 1, dil)
    err = (y0.cpu() - ref).abs().max().item()
    print(f"{c['name']}: max |y - oracle| = {err:.3e}")
    assert y0.shape == (B, P, P, H, W) and err < 1e-5
    go = torch.randn(y0.shape, generator=g)
    grads = []
    for on_abs in (False, True):
        a64, b64 = ((t.abs() if on_abs else t).double().requires_grad_() for t in (a, b))
        R.correlation(a64, b64, P, dil).backward(go.abs().double() if on_abs else go.double())
        grads.append((a64.grad, b64.grad))
    got = []
    for layout in (torch.contiguous_format, torch.channels_last):
        ag, bg = (t.to(DEV).contiguous(memory_format=layout).requires_grad_() for t in (a, b))
        assert C == 1 or ag.is_contiguous() == (layout == torch.contiguous_format)
        y = SpatialCorrelationSampler(1, P, 1, 0, 1, dil)(ag, bg)
        assert torch.equal(y.detach(), y0), layout
        y.backward(go.to(DEV))
        _check(f"{c['name']} in1", ag.grad, grads[0][0], grads[1][0])
        _check(f"{c['name']} in2", bg.grad, grads[0][1], grads[1][1])
        got.append((ag.grad, bg.grad))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


# ---- (h) what a signature accepts and the library does not implement raises ---------------------------------------------------------------------------
def test_refusals_of_unimplemented_arguments(tunables):
    """Beyond test_bad_arguments_are_refused_before_any_launch and test_fused_deform_conv_rejects_bad_arguments: groups, the correlation's kernel
    arguments, pool_mode, and -- for the fused kernel and the planar samplers -- deformable groups, channel and tap counts outside what they
    are built for, and offsets sized for the transposed geometry.  All raise; the fused kernel's launch counter does not move."""
    x = torch.randn(2, 8, 12, 20, device=DEV)
    with pytest.raises(NotImplementedError, match="groups"):
        DeformConv2d(8, 8, 3, padding=1, groups=2)
    with pytest.raises(StmError, match="groups"):
        ops.deform_conv(x, torch.zeros(2, 18, 12, 20, device=DEV), None, torch.zeros(8, 4, 3, 3, device=DEV), None, 1, 1)
    for kw in (dict(kernel_size=3), dict(stride=2), dict(padding=1), dict(dilation=2)):
        with pytest.raises(NotImplementedError, match="hot path"):
            spatial_correlation_sample(x, x, **dict(dict(kernel_size=1, patch_size=3, stride=1, padding=0, dilation=1, dilation_patch=2), **kw))
        with pytest.raises(NotImplementedError, match="hot path"):
            SpatialCorrelationSampler(**dict(dict(patch_size=3), **kw))(x, x)
    rois = torch.tensor([[0, 1.0, 1.0, 9.0, 7.0]], device=DEV)
    with pytest.raises(NotImplementedError, match="avg"):
        roi_align(x, rois, (3, 5), 0.5, 2, "max", True)
    with pytest.raises(NotImplementedError, match="avg"):
        RoIAlign((3, 5), 0.5, 2, pool_mode="max")(x, rois)
    # offsets sized for the transposed geometry: im2col, the modules
    c = G.DEFORM_TABLE[0]
    xc, off, mask, w, b, _ = (_d(t) for t in G.deform_inputs(c))
    t = G.transposed(c, "st")
    assert G.out_hw(t) != G.out_hw(c)
    with pytest.raises(StmError, match="offset shape"):
        ops.deform_im2col(xc, off, mask, t["k"], t["st"], t["pad"], t["dl"], t["dg"])
    with pytest.raises(StmError, match="offset shape"):
        DCNv2(c["C"], c["O"], c["k"], t["st"], t["pad"], t["dl"], t["dg"]).to(DEV)(xc, off, mask)
    with pytest.raises(StmError, match="offset shape"):
        DeformConv2d(c["C"], c["O"], c["k"], stride=t["st"], padding=t["pad"], dilation=t["dl"]).to(DEV)(xc.requires_grad_(), off)
    # dcn_v2.DCN where conv_offset_mask (built without the dilation) cannot have the deformable convolution's size
    assert DCN_REFUSED
    for r in DCN_REFUSED:
        with pytest.raises(StmError, match="conv_offset_mask output"):
            DCN(r["C"], r["O"], r["k"], r["st"], r["pad"], r["dl"], r["dg"]).to(DEV)(torch.randn(r["B"], r["C"], r["H"], r["W"], device=DEV))
    # the planar samplers
    p = G.PLANAR_CASES[0]
    xp, om, Ho, Wo = _planar_inputs(p)
    x_nhwc, om_pix = _d(xp.permute(0, 2, 3, 1).contiguous()), _d(om.permute(0, 2, 3, 1).reshape(-1, 27).contiguous())
    pt = G.transposed(p, "st")
    assert G.out_hw(pt)[0] * G.out_hw(pt)[1] != Ho * Wo
    with pytest.raises(StmError, match="does not match"):
        ops.dcn_sample_planar(x_nhwc, om_pix, pt["st"], pt["pad"], pt["dl"])
    with pytest.raises(StmError, match="C must be 128, 256 or 512"):
        ops.dcn_sample_planar(x_nhwc[..., :64].contiguous(), om_pix, p["st"], p["pad"], p["dl"])
    lib, stream = _lib.lib(), ops._stream()
    M = p["B"] * Ho * Wo
    planes = torch.zeros(3, 9 * p["C"] // 32, M, 32, device=DEV, dtype=torch.bfloat16)

    def sampler(C, k, dg, has_mask, om_ld=27):
        geo = DeformGeom(p["B"], C, p["H"], p["W"], *k, *p["st"], *p["pad"], *p["dl"], dg, Ho, Wo)
        return lib.stm_deform_sample_planar_f32(c_p(x_nhwc.data_ptr()), c_i(p["C"]), c_p(om_pix.data_ptr()), c_i(om_ld), c_i(has_mask),
                                                c_p(planes.data_ptr()), c_i(M), c_i(0), ctypes.c_longlong(0), ctypes.byref(geo), c_i(0), stream)
    for args, what in (((p["C"], (3, 3), 2, 1), "one deformable group"), ((p["C"], (7, 7), 1, 0), "3x3 taps"), ((p["C"], (3, 5), 1, 1), "without mask"),
                       ((p["C"], (3, 3), 1, 0), "mask-free form is built for C = 256"), ((96, (3, 3), 1, 1), "C must be 128, 256 or 512")):
        with pytest.raises(StmError, match=what):
            _lib.check(sampler(*args), "stm_deform_sample_planar_f32")
    assert not planes.any()
    # the fused kernel
    f = G.FUSED_CASES[0]
    xf, off, mask, w, b, _ = G.deform_inputs(f)
    fHo, fWo = G.out_hw(f)
    ft = G.transposed(f, "st")
    assert G.out_hw(ft)[0] * G.out_hw(ft)[1] != fHo * fWo
    x_pix = _d(xf.permute(0, 2, 3, 1).reshape(-1, f["C"]).contiguous())
    om_pix = _d(torch.cat([off, mask], 1).permute(0, 2, 3, 1).reshape(-1, 27).contiguous())
    packed, sc = ops.conv_pack_weights(_d(w), tile_n=128, fmt=1)
    n0 = lib.stm_debug_launch_count(1)
    B, C, H, W, O = (f[k] for k in ("B", "C", "H", "W", "O"))
    with pytest.raises(StmError, match="do not match"):                                     # om sized for (sh, sw), geometry (sw, sh)
        ops.deform_conv_fused_planar(x_pix, B, H, W, C, om_pix, packed, sc, None, O, f["k"], ft["st"], f["pad"], f["dl"], has_mask=True, fmt=1)
    with pytest.raises(StmError, match="C a multiple of 64"):
        ops.deform_conv_fused_planar(x_pix[:, :48].contiguous(), B, H, W, 48, om_pix, packed, sc, None, O, f["k"], f["st"], f["pad"], f["dl"],
                                     has_mask=True, fmt=1)
    zeros = lambda n: torch.zeros(B * H * W, n, device=DEV)                                  # stride 1, "same" padding: H x W outputs
    with pytest.raises(StmError, match="9 with mask"):                                      # 15 taps with mask
        ops.deform_conv_fused_planar(x_pix, B, H, W, C, zeros(45), packed, sc, None, O, (3, 5), 1, (1, 2), 1, has_mask=True, fmt=1)
    with pytest.raises(StmError, match="<= 15 taps"):
        ops.deform_conv_fused_planar(x_pix, B, H, W, C, zeros(98), packed, sc, None, O, (7, 7), 1, 3, 1, has_mask=False, fmt=1)
    assert not ops.deform_conv_fused_supported(f["C"], f["O"], 3, True, 1, deformable_groups=2)
    out = torch.zeros(2, f["O"] // 32, om_pix.shape[0], 32, device=DEV, dtype=torch.float16)
    geo = DeformGeom(f["B"], f["C"], f["H"], f["W"], 3, 3, *f["st"], *f["pad"], *f["dl"], 2, fHo, fWo)
    rc = lib.stm_deform_conv_fused_planar_f32(c_p(x_pix.data_ptr()), c_i(f["C"]), c_p(om_pix.data_ptr()), c_i(27), c_i(1), c_p(packed.data_ptr()), c_p(0),
                                              c_p(out.data_ptr()), c_i(om_pix.shape[0]), c_i(0), ctypes.c_longlong(0), c_i(f["O"]), c_i(0), c_f(sc), ctypes.byref(geo),
                                              c_i(1), c_i(1), stream)
    with pytest.raises(StmError, match="one deformable group"):
        _lib.check(rc, "stm_deform_conv_fused_planar_f32")
    assert lib.stm_debug_launch_count(1) == n0 and not out.any()
    torch.cuda.synchronize()
