"""Every case of tests/conv_rows_cases.py on the GPU against the fp64 CPU oracle (oracle.conv2d_nhwc): the kernel rows of the planar
convolution that no oracle test launched -- format 0's three-product mode on all three tile forms, the two-source product on the two-buffer
128 x 64 tiles and on the 256 x 128 tiles -- and the shared head's geometry (five levels, grouped layers, a narrow group) on the 128-wide tiles
of the fp16x2 format: the ring kernel at both tile heights, conv_planar_kx3_kernel, and split-K with its finishing kernel.
tests/test_conv_rows_cpu.py holds each case to the kernel it names here.

Bounds, the project's stated ones (tests/test_gpu_conv.py, include/stmask_hip.h): |y - y64| <= 2e-6 sum |x w| for format 0 with three planes
and for format 1, 1e-3 sum |x w| for format 2; planes output against fp32 output bit-equal (format 0), within 2^-21 (format 1) / 2^-10
(format 2) of max(1, |y| max); split-K against the unsplit run 1e-6 sum |x w|; the kx-reuse kernel against the ring kernel bit for bit.
The three-product mode's bound is derived in the docstring of test_case_vs_oracle."""
import functools
from ctypes import c_int

import pytest
import torch

import conv_rows_cases as rc
import oracle
from conv_oracle import DEV, THREE_PRODUCT_REL, bf16_split2, level_group_oracle, planar_conv_vs_oracle, rnd, three_product_model
from stmask_amd import _lib, ops
from stmask_amd.planar import PlanarConv

pytestmark = pytest.mark.gpu
TOL = {0: 2e-6, 1: 2e-6, 2: 1e-3}                       # against the oracle, of sum |x w|
PLANES_TOL = {0: 0.0, 1: 2.0 ** -21, 2: 2.0 ** -10}      # planes output against fp32 output, of max(1, |y| max)
SPLITK_TOL = 1e-6                                        # split-K against the unsplit run, of sum |x w|
_RUNS = {}                                               # case name -> its outputs (CPU), for the cases that are another case's partner


def kx3_count():
    return _lib.lib().stm_debug_launch_count(c_int(0))


class switched:
    """The switches of a case around its launches; the kx-reuse kernel's launch counter moves, by one, exactly when the case names that kernel."""

    def __init__(self, tunables, case):
        self.t, self.case = tunables, case

    def __enter__(self):
        self.t.set(**self.case["env"])
        self.n0 = kx3_count()

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        moved = kx3_count() - self.n0
        self.t.clear(*self.case["env"])
        if exc[0] is None:
            assert moved == (1 if self.case["expect"][0][0] == rc.KX3 else 0), (moved, self.case["expect"])


def planes_vs_f32(ypl, y32, fmt):
    back = ops.planes_to_f32(ypl)[:, :y32.shape[1]]
    if fmt == 0:
        assert torch.equal(back, y32)
    else:
        assert (back - y32).abs().max().item() <= PLANES_TOL[fmt] * max(1.0, y32.abs().max().item())


# ---- format 0, planes = 2 ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def three_data(i):
    """Inputs of three-product shape i, the oracle's y64 and sum |x w| (+ |bias| + |residual|), and the restated arithmetic."""
    B, H, W, C, O, kh, kw, s, pad, has_bias, _, relu = rc.THREE_SHAPES[i]
    has_res = rc.CASES[f"three_{i}_t64"]["call"]["res"] is not None
    x = rnd(B, H, W, C, seed=0)
    w = rnd(O, C, kh, kw, seed=1, scale=(C * kh * kw) ** -0.5)
    b = rnd(O, seed=2) if has_bias else None
    Ho, Wo = ops.conv_out_hw(H, W, kh, kw, s, s, pad[0], pad[1], 1, 1)
    r = rnd(B, Ho, Wo, O, seed=3) if has_res else None
    ref = oracle.conv2d_nhwc(x, w, b, r, stride=s, padding=pad, relu=relu)
    mag = oracle.conv2d_nhwc(x.abs(), w.abs(), b.abs() if has_bias else None, r.abs() if has_res else None, stride=s, padding=pad)
    model = three_product_model(x, w, s, pad)
    if has_bias:
        model = model + b.double()
    if has_res:
        model = model + r.double()
    if relu:
        model = model.clamp_min(0)
    return x, w, b, r, ref, mag, model


def check_three(name, tunables):
    """Format 0 with planes = 2: see test_case_vs_oracle."""
    case = rc.CASES[name]
    c, i = case["call"], int(name.split("_")[1])
    x, w, b, r, ref, mag, model = three_data(i)
    (B, H, W, _), O, has_res = x.shape, w.shape[0], r is not None
    shape, hw = tuple(w.shape), (B, H, W)
    kw = dict(stride=c["stride"], padding=c["pad"], relu=c["relu"], tile_n=c["tile_n"])
    xp = ops.split_planes(x.to(DEV))
    # the restated split is the device's
    (p0, p1), (q0, q1) = bf16_split2(x), bf16_split2(w)
    xpc = xp.cpu().float()
    assert torch.equal(xpc[0].permute(1, 0, 2).reshape(-1, x.shape[3]), p0.view(-1, x.shape[3]))
    assert torch.equal(xpc[1].permute(1, 0, 2).reshape(-1, x.shape[3]), p1.view(-1, x.shape[3]))
    wpc = ops.split_planes(w.reshape(-1, 32).to(DEV)).cpu().float()
    assert torch.equal(wpc[0, 0], q0.reshape(-1, 32)) and torch.equal(wpc[1, 0], q1.reshape(-1, 32))
    pk2 = ops.conv_pack_weights(w.to(DEV), planes=2, tile_n=c["tile_n"])
    pk3 = ops.conv_pack_weights(w.to(DEV), planes=3, tile_n=c["tile_n"])
    assert pk2.numel() * 3 == pk3.numel() * 2
    bd, rd = (b.to(DEV) if b is not None else None), (r.to(DEV) if has_res else None)
    xp2, poisoned = xp[:2].contiguous(), xp.clone()                                      # the first two planes; all three, the third never to be read
    poisoned[2] = float("nan")
    with switched(tunables, case):
        y32, ypl = ops.conv2d_planar(xp2, pk2, shape, hw, bd, rd, planes=2, out="both", **kw)
        y3 = ops.conv2d_planar(xp, pk3, shape, hw, bd, rd, planes=3, out="f32", **kw).cpu().view(ref.shape)
        yp = ops.conv2d_planar(poisoned, pk2, shape, hw, bd, rd, planes=2, out="f32", **kw).cpu()
        yr = ops.conv2d_planar(xp2, pk2, shape, hw, bd, ops.split_planes(rd), planes=2, out="f32", **kw).cpu() if has_res else None
    y32, ypl = y32.cpu(), ypl.cpu()
    assert torch.equal(yp, y32)                                                          # (d)
    planes_vs_f32(ypl, y32, 0)
    if has_res:
        assert torch.equal(yr, y32)
    y = y32.view(ref.shape).double()
    m = mag.double().clamp_min(1e-6)
    e_model, e_ref, e_three = ((y - model).abs() / m).max().item(), ((y - ref.double()).abs() / m).max().item(), ((y3.double() - ref.double()).abs() / m).max().item()
    print(f"{name}: |y - model| {e_model:.3e} of sum|xw| (bound {TOL[0]:.1e}), |y - y64| {e_ref:.3e} (bound {THREE_PRODUCT_REL + TOL[0]:.3e}), "
          f"three planes {e_three:.3e}")
    assert e_model < TOL[0]                                                              # (a)
    assert e_ref < THREE_PRODUCT_REL + TOL[0]                                            # (b)
    assert e_three < TOL[0] and e_ref > e_three                                          # (c)


# ---- two sources -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dual_data(tag):
    """Inputs of the two-source shape `tag` and the oracle of the two convolutions, before the residual and the ReLU."""
    B, H2, W2, P, Cin, O, s, _ = next(row[1] for row in rc.DUAL_ROWS if row[0] == tag)
    Ho, Wo = (H2 - 1) // s + 1, (W2 - 1) // s + 1
    mid, x = rnd(B, Ho, Wo, P, seed=90), rnd(B, H2, W2, Cin, seed=91)
    w3, wd = rnd(O, P, 1, 1, seed=92, scale=P ** -0.5), rnd(O, Cin, 1, 1, seed=93, scale=Cin ** -0.5)
    b3, bd = rnd(O, seed=94), rnd(O, seed=95)
    r = rnd(B * Ho * Wo, O, seed=96)
    xs = x[:, ::s, ::s].contiguous()
    lin = (oracle.conv2d_nhwc(mid, w3, b3, None).double() + oracle.conv2d_nhwc(xs, wd, bd, None).double()).view(-1, O)
    mag = (oracle.conv2d_nhwc(mid.abs(), w3.abs(), b3.abs(), None).double() + oracle.conv2d_nhwc(xs.abs(), wd.abs(), bd.abs(), None).double()).view(-1, O)
    return mid, x, w3, wd, b3, bd, r, lin, mag


def run_dual(name, tunables):
    """The case without a residual, with an fp32 residual and with one in planes, each against relu(conv3 + projection + residual) in fp64 (the
    residual the oracle adds is the value the kernel is given: the fp32 tensor, or what its planes hold) -> {residual form: (y32, planes)}."""
    if name in _RUNS:
        return _RUNS[name]
    case = rc.CASES[name]
    c, fmt, tag = case["call"], case["call"]["fmt"], name.split("_")[1]
    mid, x, w3, wd, b3, bd, r, lin, mag = dual_data(tag)
    (B, Ho, Wo, _), (_, H2, W2, _), s = mid.shape, x.shape, c["dual"][3]
    conv = PlanarConv(torch.cat([w3, wd], 1).to(DEV), (b3 + bd).to(DEV), 1, 0, relu=True, fmt=fmt, tile_n=c["tile_n"])
    midp, xp = ops.split_planes(mid.to(DEV), fmt), ops.split_planes(x.to(DEV), fmt)
    rpl = ops.split_planes(r.to(DEV), fmt)
    given = {None: (None, None), "f32": (r.to(DEV), r), "planes": (rpl, ops.planes_to_f32(rpl.cpu()))}
    outs = {}
    with switched(tunables, case):
        for form, (res, _) in given.items():
            y32, ypl = conv(midp, ("img", B, Ho, Wo), out="both", x2=(xp, H2, W2, s), residual=res)
            outs[form] = (y32.cpu(), ypl.cpu())
    for form, (_, held) in given.items():
        y32, ypl = outs[form]
        ref = (lin + held.double() if held is not None else lin).clamp_min(0)
        m = (mag + held.double().abs() if held is not None else mag).clamp_min(1e-6)
        worst = ((y32.double() - ref).abs() / m).max().item()
        print(f"{name} residual {form}: {worst:.3e} of sum|xw| (bound {TOL[fmt]:.0e})")
        assert worst < TOL[fmt], (form, worst)
        planes_vs_f32(ypl, y32, fmt)
    _RUNS[name] = outs
    return outs


def check_dual(name, tunables):
    """The two-source rows: see test_case_vs_oracle."""
    outs = run_dual(name, tunables)
    partner = rc.CASES[name]["partner"]
    if partner:
        _, _, _, _, _, _, r, _, mag = dual_data(name.split("_")[1])
        base = run_dual(partner[0], tunables)
        for form, (y32, _) in outs.items():
            m = (mag + r.double().abs() if form else mag).clamp_min(1e-6)
            assert ((y32 - base[form][0]).double().abs() / m).max().item() < SPLITK_TOL, form      # only the summation order differs


# ---- the head's geometry -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_data(data):
    """Inputs of the head cases that share the data name, the (level, group) oracle and sum |x w| over the whole output (inf at padded channels)."""
    c = next(case["call"] for case in rc.CASES.values() if case["data"] == data)
    G, C, O, B, sizes = c["groups"], c["C"], c["O"], c["B"], c["sizes"]
    cg = O // G
    real = tuple(c["group_cout"] or [cg] * G)
    xs = [rnd(B, h, w, G * C, seed=40 + i) for i, (h, w) in enumerate(sizes)]
    wts = rnd(O, C, c["kh"], c["kw"], seed=50, scale=(C * c["kh"] * c["kw"]) ** -0.5)
    for g in range(G):
        wts[g * cg + real[g]:(g + 1) * cg] = 0.0                      # zero-padded groups, as planar.py builds them
    bias = rnd(O, seed=51)
    refs = level_group_oracle(xs, sizes, B, wts, bias, c["pad"], c["relu"], C, G, cg, real)
    mag = torch.full((rc.level_starts(B, sizes)[-1], O), float("inf"))
    for rows, cols, ref, m in refs:
        mag[rows, cols] = m.reshape(-1, m.shape[-1])
    return xs, wts, bias, cg, real, refs, mag


def run_head(name, tunables):
    if name in _RUNS:
        return _RUNS[name]
    case = rc.CASES[name]
    c = case["call"]
    xs, wts, bias, cg, real, refs, _ = head_data(case["data"])
    conv = PlanarConv(wts.to(DEV), bias.to(DEV), 1, c["pad"], relu=c["relu"], groups=c["groups"], group_cout=c["group_cout"], tile_n=c["tile_n"], fmt=1)
    conv.kxr = False                                                  # (stm_conv2d_planar_kxr_f32 is another kernel family)
    with switched(tunables, case):
        y32, ypl, worst = planar_conv_vs_oracle(conv, xs, c["sizes"], c["B"], wts, bias, c["pad"], c["relu"], c["C"], c["groups"], cg, real, 1, TOL[1], refs=refs)
    print(f"{name}: {worst:.3e} of sum|xw| (bound {TOL[1]:.0e})")
    planes_vs_f32(ypl, y32, 1)
    _RUNS[name] = (y32, ypl)
    return y32, ypl


def check_head(name, tunables):
    """The head's geometry: see test_case_vs_oracle."""
    case = rc.CASES[name]
    y32, ypl = run_head(name, tunables)
    _, _, bias, cg, real, _, mag = head_data(case["data"])
    for g, n in enumerate(real):
        pad = slice(g * cg + n, (g + 1) * cg)
        assert torch.equal(y32[:, pad], bias[pad].clamp_min(0).expand(y32.shape[0], -1))
    if case["partner"]:
        other, relation = case["partner"]
        b32, bpl = run_head(other, tunables)
        if relation == "bitwise":
            assert torch.equal(y32, b32) and torch.equal(ypl, bpl)
        else:
            assert ((y32 - b32).abs() / mag.clamp_min(1e-6)).max().item() < SPLITK_TOL


# ---- the one test --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_case_vs_oracle(name, tunables):
    """three_*: Format 0 with planes = 2 (include/stmask_hip.h: "three products"): conv_planar_kernel<2, MG, NJ, 0, 2> reads planes 0 and 1 of the bf16
    split of x and of the weights and adds p0 q0 + p0 q1 + p1 q0 in fp32.

    The arithmetic, restated on the CPU: p0 = RN_bf16(x), p1 = RN_bf16(x - p0) -- asserted equal to planes 0 and 1 of ops.split_planes(x), and
    the same split of w to the planes of ops.split_planes over the weight values -- and model = sum (p0 q0 + p0 q1 + p1 q0) in fp64.  The kernel
    must sit (a) within the accumulation bound of the other formats, 2e-6 sum |x w|, of model and (b) within a derived bound of the oracle's y64:

      With u = 2^-9 (bf16 keeps 8 significand bits, round to nearest) and no underflow: p0 = x (1 + d1), p1 = (x - p0)(1 + d2), |d| <= u, so
      |p1| <= u (1 + u) |x| and ex = x - p0 - p1 has |ex| <= u^2 |x|; likewise q1 and ew for w.  Then
        x w - (p0 q0 + p0 q1 + p1 q0) = p1 q1 + x ew + ex w - ex ew,
      at most u^2 |x w| ((1 + u)^2 + 2 + u^2) <= 3 u^2 (1 + u) |x w| = 3 * 2^-18 (1 + 2^-9) |x w| = 1.147e-5 |x w|: two 8-bit roundings per
      operand (u^2 each) plus the dropped p1 q1 term (u^2).  That is 2^-16.4, the header's "~2^-16".  So
        |y - y64| <= (3 * 2^-18 (1 + 2^-9) + 2e-6) sum |x w|.

    (c) The error against y64 is larger than that of the three-plane run of the same inputs on the same tiles: the case cannot have run the
    six-product kernel unnoticed.  (d) The input is planes 0 and 1 alone; given all three, plane 2 is not read: poisoned with NaN it changes
    nothing.  Both outputs, bit-equal (the epilogue writes all three planes of the fp32 result); the residual of shape 0 given as fp32 and as
    planes, bit-equal.  (Observed: |y - model| 5e-8 .. 7e-8, |y - y64| 1.6e-6 .. 1.8e-6, the three-plane run 5e-8 .. 8e-8 of sum |x w|.)

    dual_*: stm_conv2d_planar_dual_f32 on the rows the small shapes of test_conv_dual_source_vs_oracle never get: the two-buffer loop of the 128 x 64
    tiles (what plan_conv gives a short-K layer on a large grid) and the 256 x 128 tiles (three double tiles, the last with 8 pixels), unsplit
    and split along K with the workspace PlanarConv brings; with and without a residual in either form.

    head_*: The level, image-row and group decoding of the kernels the head's towers get -- conv_planar_kernel<2, 1, 2, 1, 3> at one clip,
    conv_planar_kx3_kernel or <2, 2, 2, 1, 3> at batch -- against the oracle per (level, group), not only against each other: 969 pixels in five
    levels of three images, the last two smaller than the kernel's halo, tiles across image rows, images and levels, a partial last tile; 3x3,
    5x3 and 1x3 kernels; four, two and one group; K split by the switch and by the rule (the finishing kernel over groups and levels).
    The kx-reuse kernel equals the ring kernel bit for bit, split-K the unsplit run to 1e-6 sum |x w|.  A group with 41 real channels of 128
    keeps the ring kernel at both tile heights; its padded channels carry zero weights, so they hold relu(bias) exactly and the oracle
    comparison reads the real ones only."""
    {"three": check_three, "dual": check_dual, "head": check_head}[name.split("_")[0]](name, tunables)
