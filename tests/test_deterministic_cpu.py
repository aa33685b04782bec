"""The deterministic backward without a GPU: the exponent rule of csrc/det_accum.h swept through the library's host function, the numpy restatements
of tests/det_restate.py against their own float64 oracles (and torch's CPU backward as the anchor of the upsample bound), the switch of
stmask_amd.autograd, which calls the mode routes through which table, and the package-private binding of csrc/det_backward.h."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import det_restate as D
from kernel_resources import kernel_resources
from conftest import ROOT
from stmask_amd import _lib, autograd, ops
from stmask_amd._lib import StmError
from stmask_amd.config import get_cfg
from stmask_amd.layers.modules import FPN, InterpolateModule

UPSAMPLE_CASES = [((4, 6), (8, 12), None), ((5, 7), (12, 17), None), ((3, 5), (3, 5), None), ((6, 10), None, 2.0), ((1, 1), (4, 4), None),
                  ((2, 3), (5, 4), None)]


@pytest.fixture(autouse=True)
def mode_as_found():
    yield
    autograd.set_deterministic(None)
    torch.use_deterministic_algorithms(False)


def host_exponent(bits_a, bits_b, terms, mass):
    """stm_det_exponent -> (return code, state, p, q)"""
    fn = ctypes.CDLL(_lib.LIB_PATH).stm_det_exponent
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 3
    p, state, q = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    rc = fn(bits_a, bits_b, terms, mass, ctypes.byref(p), ctypes.byref(state), ctypes.byref(q))
    return rc, state.value, p.value, q.value


# ---- the exponent rule ------------------------------------------------------------------------------------------------------------------------
MAXIMA = [1, 2, 3, 0x7FFFFF, 0x800000, 0x800001, 0x3F7FFFFF, 0x3F800000, 0x3F800001, 0x40490FDB, 0x4B000000, 0x5F000000, 0x7F000000, 0x7F7FFFFF]
BOUNDS = [1, 2, 3, 81 * 9, 34560, 2 ** 24 - 1, 2 ** 24, 2 ** 25, 2 ** 26 - 1, 2 ** 26, 2 ** 26 + 1, 2 ** 27, 2 ** 31 - 1, 2 ** 31]


def test_exponent_rule_never_overflows_is_maximal_and_refuses_below_the_floor():
    seen_refused = seen_floor = 0
    for mass in BOUNDS:
        for terms in BOUNDS:
            q = D.shape_bits(terms, mass)
            # q is the largest exponent that cannot overflow: the condition holds at q and fails at q + 1 (Python integers: exact)
            assert 2 * mass * 2 ** q + terms < 2 ** 63 <= 2 * mass * 2 ** (q + 1) + terms
            for a in MAXIMA:
                for b in (D.ONE_BITS, 0x40490FDB, 0x7F7FFFFF, 1):
                    rc, state, p, got_q = host_exponent(a, b, terms, mass)
                    assert got_q == q, (a, b, terms, mass)
                    if q < D.MIN_BITS:
                        assert rc == -5 and (state, p) == (0, 0)                             # STM_EUNSUPPORTED, nothing derived
                        seen_refused += 1
                        continue
                    seen_floor += q == D.MIN_BITS
                    assert rc == 0 and (state, p, q) == D.exponent(a, b, terms, mass), (a, b, terms, mass)
                    if state != D.FINITE:
                        assert D.value_of_bits(a) * D.value_of_bits(b) > 3.4028234e38 and p == 0     # the product of the maxima overflows fp32
                        continue
                    # no term exceeds 2^E, E = q - p, and that bound is within a factor 4 of the product of the maxima (a factor 2 per maximum)
                    va, vb = D.value_of_bits(a), D.value_of_bits(b)
                    E = q - p
                    assert va * vb <= 2.0 ** E and (2.0 ** (E - 2) < va * vb if E > -290 else True)
                    # the worst case the bounds allow: `terms` terms that share a mass of `mass` maxima, each rounded up by half a unit
                    worst = mass * 2 ** E * 2 ** p + (terms + 1) // 2 if p >= -E else None
                    assert worst is None or worst < 2 ** 62
    assert seen_refused and seen_floor                                                       # both sides of the 36-bit floor were visited


def test_exponent_rule_special_values_and_arguments():
    n = 9 * 81
    for b in (0x7F800000, 0x7F800001, 0x7FC00000, 0x7FFFFFFF):                               # inf and NaN patterns in either word
        assert host_exponent(b, D.ONE_BITS, n, n)[:3] == (0, D.NONFINITE, 0)
        assert host_exponent(0x3F000000, b, n, n)[:3] == (0, D.NONFINITE, 0)
    assert host_exponent(0, D.ONE_BITS, n, n)[:3] == (0, D.ZERO, 0) and host_exponent(0x3F800000, 0, n, n)[:3] == (0, D.ZERO, 0)
    assert host_exponent(0, 0x7F800000, n, n)[:3] == (0, D.NONFINITE, 0)                     # not finite wins over zero
    # 1.0 is its own bound, the next value up is bounded by 2; the smallest subnormal by itself
    q = D.shape_bits(n, n)
    assert host_exponent(0x3F800000, D.ONE_BITS, n, n) == (0, 0, q, q) and host_exponent(0x3F800001, D.ONE_BITS, n, n) == (0, 0, q - 1, q)
    assert host_exponent(1, D.ONE_BITS, n, n) == (0, 0, q + 149, q) and host_exponent(1, 1, n, n) == (0, 0, q + 298, q)
    assert host_exponent(0x7F7FFFFF, D.ONE_BITS, n, n) == (0, 0, q - 128, q)
    assert q == 62 - 10 and n < 2 ** 10                                                      # 729 terms: ten bits of head room
    for args in ((-1, D.ONE_BITS, n, n), (1, -1, n, n), (1, 1, -1, n), (1, 1, n, 0)):
        assert host_exponent(*args)[0] == -1                                                 # STM_EINVAL
    fn = ctypes.CDLL(_lib.LIB_PATH).stm_det_exponent
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 3
    assert fn(1, 1, n, n, None, None, None) == -2                                            # STM_ENULL


def test_the_models_shapes_leave_42_bits_or_more():
    # DCN at the largest R50 level of a 384 x 640 frame (48 x 80, 3 x 3); RoIAlign of the shift loss with 4096 positives, 7 x 7 bins
    assert D.shape_bits(*D.col2im_bounds((3, 3), 48, 80)) >= 42
    assert D.shape_bits(*D.roi_bounds(4096, 7, 7, 0)) >= 42
    size = ctypes.CDLL(_lib.LIB_PATH).stm_det_workspace_bytes
    size.restype, size.argtypes = ctypes.c_size_t, [ctypes.c_int64]
    assert size(0) == 8 and size(1000) == 8008 and size(-1) == 0


# ---- the restatements -------------------------------------------------------------------------------------------------------------------------
def col2im_case(seed, mask_scale=None, logit=False):
    g = np.random.default_rng(seed)
    B, C, H, W, dg, k = 2, 8, 7, 9, 2, (3, 3)
    geom = dict(B=B, C=C, H=H, W=W, k=k, st=(1, 1), pad=(1, 1), dl=(1, 1), dg=dg)
    K, HWo = 9, H * W
    gcols = g.standard_normal((B, C * K, HWo)).astype(np.float32)
    off = (g.standard_normal((B, dg * 2 * K, H, W)) * 2).astype(np.float32)
    mask = None if mask_scale is None else (g.standard_normal((B, dg * K, H, W)) * mask_scale).astype(np.float32)
    return geom, gcols, off, mask, logit


@pytest.mark.parametrize("mask_scale,logit", [(None, False), (3.0, False), (2.0, True)], ids=["v1", "explicit_mask_above_1", "logit_mask"])
def test_fixed_point_col2im_is_order_free_and_inside_its_bound(mask_scale, logit):
    geom, gcols, off, mask, logit = col2im_case(5, mask_scale, logit)
    dest, t32, t64 = D.col2im_terms(gcols, off, mask, mask_logit=logit, **geom)
    numel = geom["B"] * geom["C"] * geom["H"] * geom["W"]
    assert dest.min() >= 0 and dest.max() < numel and len(dest) > 10 * numel
    bounds = D.col2im_bounds(geom["k"], geom["H"], geom["W"])
    assert np.bincount(dest, minlength=numel).max() <= bounds[0]                              # the terms bound holds on the case
    b_bits = D.absmax_bits(mask) if (mask is not None and not logit) else D.ONE_BITS
    got, state, p = D.det_result(dest, t32, numel, D.absmax_bits(gcols), b_bits, *bounds)
    assert state == D.FINITE and np.abs(t32).max() <= 2.0 ** (D.shape_bits(*bounds) - p)      # no term exceeds the power-of-two bound
    perm = np.random.default_rng(1).permutation(len(dest))
    assert np.array_equal(D.bits(got), D.bits(D.fixed_point(dest[perm], t32[perm], numel, p)))   # any arrival order: the same bits
    ref, tol = D.scatter_oracle(dest, t64, numel, p)
    assert (np.abs(got - ref) <= tol).all()
    # ... and the bound is about fp32, not about the fixed point: the integer part of it is far below one fp32 ulp of the result
    assert (np.bincount(dest, minlength=numel) * 2.0 ** -(p + 1)).max() < 1e-3 * D.EPS * np.abs(ref).max()
    # the plain fp32 sum in index order sits in the same bound only with the summation error added: the two differ, by less than that
    plain = np.zeros(numel, np.float32)
    np.add.at(plain, dest, t32)
    assert not np.array_equal(D.bits(plain), D.bits(got))


def test_fixed_point_edge_states():
    geom, gcols, off, mask, _ = col2im_case(6, 3.0)
    dest, t32, _ = D.col2im_terms(gcols, off, mask, **geom)
    numel = geom["B"] * geom["C"] * geom["H"] * geom["W"]
    bounds = D.col2im_bounds(geom["k"], geom["H"], geom["W"])
    out, state, _ = D.det_result(dest, t32, numel, 0, D.absmax_bits(mask), *bounds)
    assert state == D.ZERO and not out.any()
    bad = gcols.copy()
    bad[1, 3, 5] = np.inf
    out, state, _ = D.det_result(dest, t32, numel, D.absmax_bits(bad), D.absmax_bits(mask), *bounds)
    assert state == D.NONFINITE and np.isnan(out).all()
    bad[1, 3, 5] = np.nan
    assert D.absmax_bits(bad) > 0x7F800000


@pytest.mark.parametrize("aligned,sr", [(True, 0), (False, 2)])
def test_roi_restatement_is_the_adjoint_of_torchvision_style_roi_align(aligned, sr):
    import autograd_restate as R
    g = torch.Generator().manual_seed(3)
    B, C, H, W, n = 2, 3, 8, 11, 6
    rois = torch.tensor([[0, 1.0, 1.5, 7.5, 6.0], [1, -2.0, 0.5, 5.0, 9.5], [0, 3.0, 2.0, 3.2, 2.4], [1, 6.0, 4.0, 13.0, 7.9], [0, 0.0, 0.0, 11.0, 8.0],
                         [1, 2.2, 2.2, 4.9, 6.1]])
    gout = torch.randn(n, C, 3, 3, generator=g)
    feat = torch.randn(B, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    (R.roi_align(feat, rois, (3, 3), 1.0, sr, aligned) * gout.double()).sum().backward()
    dest, t32, t64 = D.roi_terms(gout.numpy(), rois.numpy(), B, C, H, W, 3, 3, 1.0, sr, aligned)
    numel = B * C * H * W
    terms, mass = D.roi_bounds(n, 3, 3, sr)
    got, state, p = D.det_result(dest, t32, numel, D.absmax_bits(gout.numpy()), D.ONE_BITS, terms, mass)
    ref, tol = D.scatter_oracle(dest, t64, numel, p)
    assert state == D.FINITE and (np.abs(got - ref) <= tol).all()
    # the float64 sum of the restated terms is the float64 autograd gradient of the project's RoIAlign oracle (positions rounded as fp32 there too)
    assert np.abs(ref - feat.grad.numpy().ravel()).max() < 1e-5
    cnt = np.bincount(dest, minlength=numel)
    mag = np.zeros(numel)
    np.add.at(mag, dest, np.abs(t64))
    assert cnt.max() <= terms and mag.max() <= mass * float(gout.abs().max())                # both bounds hold on the case


@pytest.mark.parametrize("in_hw,size,sf", UPSAMPLE_CASES, ids=[f"{i[0]}x{i[1]}" for i, _, _ in UPSAMPLE_CASES])
def test_upsample_restatement_bounds_torchs_own_cpu_backward(in_hw, size, sf):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, *in_hw, generator=g, requires_grad=True)
    y = F.interpolate(x, size=size, scale_factor=sf, mode="bilinear", align_corners=False)
    go = torch.randn(y.shape, generator=g)
    y.backward(go)
    ref, tol = D.upsample_adjoint(go.numpy(), *in_hw, scale_factor=sf)
    err = np.abs(x.grad.numpy().astype(np.float64) - ref)
    print(f"\n{in_hw} -> {tuple(y.shape[2:])}: torch's fp32 CPU backward at {float((err / tol).max()):.3f} of the bound")
    assert (err <= tol).all()
    # ... and the float64 restatement is torch's float64 backward to rounding
    x64 = x.detach().double().requires_grad_(True)
    F.interpolate(x64, size=size, scale_factor=sf, mode="bilinear", align_corners=False).backward(go.double())
    assert np.abs(x64.grad.numpy() - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())


# ---- the switch -------------------------------------------------------------------------------------------------------------------------------
def test_switch_follows_torchs_flag_unless_overridden():
    assert autograd.is_deterministic() is False
    torch.use_deterministic_algorithms(True)
    assert autograd.is_deterministic() is True
    torch.use_deterministic_algorithms(True, warn_only=True)
    assert autograd.is_deterministic() is True
    autograd.set_deterministic(False)
    assert autograd.is_deterministic() is False
    torch.use_deterministic_algorithms(False)
    autograd.set_deterministic(True)
    assert autograd.is_deterministic() is True
    autograd.set_deterministic(None)
    assert autograd.is_deterministic() is False
    for bad in (1, "on", 0):
        with pytest.raises(ValueError, match="True, False or None"):
            autograd.set_deterministic(bad)


@pytest.fixture
def recorded(monkeypatch):
    """ops with its launches recorded instead of made: names through _lib.call (the public tables) and through _lib.private_call."""
    calls = {"public": [], "private": []}
    monkeypatch.setattr(ops, "call", lambda name, *a: calls["public"].append(name))
    monkeypatch.setattr(_lib, "private_call", lambda name, *a: calls["private"].append(name))
    monkeypatch.setattr(ops, "_dev", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    return calls


def scatter_calls():
    g = ops._geom(torch.zeros(1, 4, 5, 6), (3, 3), 1, 1, 1, 1)
    ops.deform_col2im(torch.zeros(1, 36, 30), torch.zeros(1, 18, 5, 6), None, g)
    ops.roi_align_backward(torch.zeros(2, 4, 7, 7), torch.zeros(2, 5), (1, 4, 5, 6), 7)


def test_mode_is_read_where_the_launch_is_chosen(recorded):
    scatter_calls()
    assert recorded == {"public": ["stm_deform_col2im_f32", "stm_roi_align_backward_f32"], "private": []}     # off: today's launches, nothing new
    autograd.set_deterministic(True)
    scatter_calls()
    assert recorded["private"] == ["stm_deform_col2im_det_f32", "stm_roi_align_backward_det_f32"] and len(recorded["public"]) == 2
    autograd.set_deterministic(None)
    torch.use_deterministic_algorithms(True)                # torch's flag alone
    scatter_calls()
    assert len(recorded["private"]) == 4 and len(recorded["public"]) == 2
    # the override wins over the flag: the atomic launches are chosen -- and, being the one thing under torch's flag that is not deterministic,
    # they report as torch's own operators do: a RuntimeError before anything is launched, a warning with warn_only
    autograd.set_deterministic(False)
    with pytest.raises(RuntimeError, match=r"stm_deform_col2im_f32 does not have a deterministic implementation.*set_deterministic\(False\)"):
        scatter_calls()
    g = ops._geom(torch.zeros(1, 4, 5, 6), (3, 3), 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match="stm_roi_align_backward_f32 does not have a deterministic implementation"):
        ops.roi_align_backward(torch.zeros(2, 4, 7, 7), torch.zeros(2, 5), (1, 4, 5, 6), 7)
    assert len(recorded["private"]) == 4 and len(recorded["public"]) == 2
    torch.use_deterministic_algorithms(True, warn_only=True)
    with pytest.warns(UserWarning, match="does not have a deterministic implementation"):
        scatter_calls()
    assert len(recorded["private"]) == 4 and len(recorded["public"]) == 4
    torch.use_deterministic_algorithms(False)               # without torch's flag, off is off: today's launches, no word
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        scatter_calls()
    assert len(recorded["private"]) == 4 and len(recorded["public"]) == 6


def test_cpu_tensors_never_take_a_kernel_route(monkeypatch):
    private = []
    monkeypatch.setattr(_lib, "private_call", lambda name, *a: private.append(name))
    monkeypatch.setattr(autograd.UpsampleBilinearFunction, "apply", lambda *a: pytest.fail("the kernel route on a CPU tensor"))
    autograd.set_deterministic(True)
    torch.use_deterministic_algorithms(True)
    cfg = get_cfg("STMask_plus_resnet50_config")
    fpn = FPN([8, 12, 16], cfg)
    feats = [torch.randn(1, c, s, s + 2, requires_grad=True) for c, s in ((8, 12), (12, 6), (16, 3))]
    sum(o.sum() for o in fpn(feats)).backward()
    assert all(f.grad is not None for f in feats)
    up = InterpolateModule(scale_factor=2, mode="bilinear", align_corners=False)
    x = torch.randn(1, 2, 3, 4, requires_grad=True)
    up(x).sum().backward()
    assert torch.equal(up(x), F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)) and private == []
    assert not autograd.takes_upsample_kernel(x, "bilinear", False)
    with pytest.raises(StmError, match="no CPU fallback"):
        ops.upsample_bilinear_backward(torch.zeros(1, 2, 6, 8), (1, 2, 3, 4))


def test_upsample_route_conditions():
    class Cuda(torch.Tensor):          # a CPU tensor that says it is on the GPU: the conditions, without one
        is_cuda = True
    x = torch.randn(1, 2, 3, 4, requires_grad=True).as_subclass(Cuda)
    assert not autograd.takes_upsample_kernel(x, "bilinear", False)                          # the mode is off
    autograd.set_deterministic(True)
    assert autograd.takes_upsample_kernel(x, "bilinear", False)
    assert not autograd.takes_upsample_kernel(x, "nearest", None) and not autograd.takes_upsample_kernel(x, "bilinear", True)
    assert not autograd.takes_upsample_kernel(x, "bilinear", None)
    assert not autograd.takes_upsample_kernel(x.detach(), "bilinear", False)                 # nobody wants a gradient
    with torch.no_grad():
        assert not autograd.takes_upsample_kernel(x, "bilinear", False)
    assert not autograd.takes_upsample_kernel(x.double(), "bilinear", False)


# ---- the private binding ----------------------------------------------------------------------------------------------------------------------
def test_private_call_resolves_the_entries_and_refusals_launch_nothing():
    with pytest.raises(StmError, match="takes 10 arguments, got 2"):
        _lib.private_call("stm_upsample_bilinear_backward_f32", None, None)
    with pytest.raises(StmError, match="takes 11 arguments, got 1"):
        _lib.private_call("stm_deform_col2im_det_f32", None)
    with pytest.raises(StmError, match="code -1:.*bad sizes"):
        _lib.private_call("stm_upsample_bilinear_backward_f32", None, None, 1, 0, 4, 4, 4, 0.0, 0.0, None)
    with pytest.raises(StmError, match="code -2:.*non-NULL"):
        _lib.private_call("stm_upsample_bilinear_backward_f32", None, None, 1, 2, 4, 4, 4, 0.0, 0.0, None)
    with pytest.raises(StmError, match="code -5:.*above"):
        _lib.private_call("stm_upsample_bilinear_backward_f32", 8, 8, 1, 2, 4, 2 ** 20 + 1, 4, 0.0, 0.0, None)
    g = _lib.DeformGeom(1, 4, 5, 6, 3, 3, 1, 1, 1, 1, 1, 1, 1, 5, 6)
    with pytest.raises(StmError, match="code -4:.*workspace is NULL"):
        _lib.private_call("stm_deform_col2im_det_f32", 8, 8, 18 * 30, None, 0, 0, 8, ctypes.byref(g), None, 0, None)
    with pytest.raises(StmError, match="code -4:.*workspace of 8 bytes < 968"):
        _lib.private_call("stm_deform_col2im_det_f32", 8, 8, 18 * 30, None, 0, 0, 8, ctypes.byref(g), 8, 8, None)
    # shapes that leave fewer than 36 bits: 2^22 RoIs of 14 x 14 bins (the pointers are never read)
    with pytest.raises(StmError, match="code -5:.*fewer than 36"):
        _lib.private_call("stm_roi_align_backward_det_f32", 8, 8, 8, 1, 1, 2, 2, 2 ** 22, 14, 14, 1.0, 64, 1, 8, 8 * 5, None)


def test_det_kernels_use_no_scratch_and_no_lds():
    rows = kernel_resources("det_backward.hip")
    assert len(rows) == 5
    for name, r in rows.items():
        assert r.scratch == 0, name
        assert r.lds == 0, name


def test_training_scripts_take_the_flag():
    for script in ("train_ytvis.py", "train_synthetic.py"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--help"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "--deterministic" in out.stdout, script
