"""One case list for the kernel rows of the planar convolution, read by tests/test_conv_rows_cpu.py (which kernel does each case launch?) and
tests/test_gpu_conv_rows.py (is what that kernel computes the fp64 oracle's convolution?).

A case is a CALL -- geometry, format, planes, tile width, groups and their real channels, levels or one image size, second source, residual
form, whether PlanarConv's split-K workspace comes with it -- the STM_CONV_* switches it runs under, and the launch line(s) it is meant to
produce: EXPECT = [(kernel, splitk)], the finishing kernel last where K is split.  plan_case turns a case into a case of
tests/conv_plan_cases.py, so the dry run is that module's dry_run over that module's placeholder addresses.

The shapes of the fp64-oracle tests that were in tests/test_gpu_conv.py before this list live here too, as data (CONV_CASES, LOOP_CASES,
DUAL_CASES, KX3_CASES, WINDOW_TEST), with existing_launches() saying how those tests call the launcher: the coverage claim of
test_conv_rows_cpu.py -- every shipped kernel is compared with the oracle by some GPU test -- is computed from them, not copied."""
import conv_plan_cases as cc
from stmask_amd.planar import PlanarConv, border_windows

WS_BYTES = PlanarConv.SPLITK_WS_BYTES       # the workspace every PlanarConv call brings
RING = "conv_planar_kernel<%d,%d,%d,%d,%d,0,%d,0>"      # NPL, MG, NJ, DT, ST, DUAL
KX3 = "conv_planar_kx3_kernel<0,0>"
FINISH = "planar_splitk_finish_kernel"

# ---- the shapes of the tests in tests/test_gpu_conv.py -----------------------------------------------------------------------------------
CONV_CASES = [
    # B, H,  W,  C, Cout, kh, kw, stride, pad(h,w), bias, residual, relu
    (2, 12, 20, 32, 64, 3, 3, 1, (1, 1), True, False, True),      # head-tower-like 3x3
    (1, 24, 40, 64, 256, 1, 1, 1, (0, 0), True, True, True),      # bottleneck conv3 + residual
    (2, 13, 17, 32, 27, 3, 3, 2, (1, 1), True, False, False),     # conv_offset_mask-like: stride 2, Cout 27, odd sizes
    (1, 6, 10, 64, 41, 3, 5, 1, (1, 2), True, False, False),      # FCB trailing conv 3x5 -> 41 classes
    (1, 3, 5, 32, 130, 5, 3, 1, (2, 1), False, False, True),      # P7: 15 pixels, 5x3, Cout just over one tile
    (3, 9, 11, 96, 4, 3, 3, 1, (1, 1), True, False, False),       # bbox layer: Cout 4
    (1, 48, 80, 256, 256, 3, 3, 1, (1, 1), True, False, True),    # the P3 tower layer at full size
]
# test_conv_planar_fp16_loop_variants_agree_bitwise: B, H, W, C, O, k and the switches of each variant
LOOP_CASES = [(2, 24, 40, 64, 128, 3), (8, 48, 80, 128, 256, 3), (1, 12, 20, 512, 64, 1), (2, 6, 10, 1024, 128, 3)]
LOOP_VARIANTS = [("ring", {}), ("two-buffer", {"STM_CONV_RING": "2", "STM_CONV_RING64": "2"}), ("ring64", {"STM_CONV_RING64": "4"}),
                 ("splitk", {"STM_CONV_SPLITK": "3"})]
# test_conv_dual_source_vs_oracle: B, H2, W2, P, Cin, O, s2, tile_n
DUAL_CASES = [(2, 24, 40, 64, 64, 256, 1, 64), (2, 25, 39, 128, 256, 512, 2, 64), (1, 12, 20, 256, 512, 1024, 2, 128), (3, 6, 10, 512, 1024, 2048, 2, 128)]
KX3_CASES = [
    # B, sizes (levels) or one (H, W), C per group, O, groups, kh, residual
    ("img 48x80", 8, [(48, 80)], 128, 256, 1, 3, False),
    ("img 37x53 odd, residual, partial last tile", 19, [(37, 53)], 64, 128, 1, 3, True),
    ("levels, grouped towers", 6, [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)], 64, 512, 4, 3, False),
    ("levels 5x3 kernel", 5, [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)], 64, 128, 1, 5, False),
    ("1x3 kernel", 4, [(40, 64)], 96, 128, 1, 1, False),
]
KX3_ENV = {"STM_CONV_MG": "2", "STM_CONV_SPLITK": "1"}                       # (the kx3 test adds STM_CONV_KX3 = 0 / 1)
# test_conv_window_launches_equal_the_padded_convolution: n maps of each size, the nine border classes as one window set
WINDOW_TEST = dict(n=37, C=64, O=128, hw=[(7, 7), (5, 9), (3, 3)])
# kernels no convolution test of these two files launches, with the test that compares them with a reference
REACHED_ELSEWHERE = {"conv_planar_kernel<2,2,2,1,3,0,0,2>": ("test_gpu_head_shapes.py", "test_gated_window_set_equals_the_full_window_gated_launch")}


# ---- a call ------------------------------------------------------------------------------------------------------------------------------
def call(C, O, k, B=1, hw=None, sizes=None, stride=1, pad=None, fmt=1, planes=None, tile_n=128, groups=1, group_cout=None, dual=None, res=None,
         ws=True, bias=True, relu=True):
    """A planar convolution call.  C: input channels per group (both sources together for a two-source call); k: kh or (kh, kw); hw: one image
    size, or sizes: the levels of a multi-level launch, B images each; pad: "same" unless given; dual = (C2, H2, W2, s2): the last C2 input channels
    come from a second tensor of B images H2 x W2 read at stride s2; res: None / "f32" / "planes"; ws: PlanarConv's workspace comes with the call
    (ops.conv2d_planar brings none)."""
    kh, kw = (k, k) if isinstance(k, int) else k
    pad = ((kh - 1) // 2, (kw - 1) // 2) if pad is None else pad
    assert (hw is None) != (sizes is None)
    return dict(C=C, O=O, kh=kh, kw=kw, B=B, hw=hw, sizes=sizes, stride=stride, pad=tuple(pad), fmt=fmt, planes=cc.PLANES[fmt] if planes is None else planes,
                tile_n=tile_n, groups=groups, group_cout=list(group_cout) if group_cout else None, dual=dual, res=res, ws=ws, bias=bias, relu=relu)


def level_starts(B, sizes):
    starts = [0]
    for h, w in sizes:
        starts.append(starts[-1] + B * h * w)
    return starts


def plan_case(c, env=None):
    """The call as a case of conv_plan_cases (geometry as ops.conv2d_planar / PlanarConv fill it, placeholder addresses, both outputs)."""
    s = c["stride"]
    g = dict(C=c["C"], Cout=c["O"], kh=c["kh"], kw=c["kw"], sh=s, sw=s, ph=c["pad"][0], pw=c["pad"][1], planes=c["planes"], fmt=c["fmt"], tile_n=c["tile_n"],
             groups=c["groups"])
    if c["group_cout"]:
        g["group_cout"] = c["group_cout"]
    if c["sizes"] is not None:
        g.update(n_levels=len(c["sizes"]), lvl_h=[h for h, _ in c["sizes"]], lvl_w=[w for _, w in c["sizes"]], lvl_start=level_starts(c["B"], c["sizes"]))
    else:
        H, W = c["hw"]
        g.update(B=c["B"], H=H, W=W, Ho=(H + 2 * c["pad"][0] - c["kh"]) // s + 1, Wo=(W + 2 * c["pad"][1] - c["kw"]) // s + 1)
    dual = None
    if c["dual"]:
        C2, H2, W2, s2 = c["dual"]
        dual = dict(x2=cc.X2, C2=C2, H2=H2, W2=W2, s2=s2, np=0, ps=0)
    return dict(g=g, env=env or {}, x=cc.X, w=cc.WT, bias=cc.BIAS if c["bias"] else 0, res32=cc.RES32 if c["res"] == "f32" else 0,
                respl=cc.RESPL if c["res"] == "planes" else 0, out32=cc.OUT32, outpl=cc.OUTPL, relu=int(c["relu"]), ws=cc.WS if c["ws"] else 0,
                ws_bytes=WS_BYTES if c["ws"] else 0, dual=dual, windows=None, wptrs=None, pool=0, gate=0, n_windows=None)


def launches(lib, case):
    """[(kernel, splitk or None)] of the dry run of a conv_plan_cases case.  The caller has set the case's switches and reloaded them."""
    rc, text, err = cc.dry_run(lib, case)
    assert rc == 0, (rc, err)
    out = []
    for line in text.splitlines():
        kernel, rest = (line.split(" ", 1) + [""])[:2]
        sk = [int(f.split("=")[1]) for f in rest.split() if f.startswith("splitk=")]
        out.append((kernel, sk[0] if sk else None))
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
# name -> dict(call, env, expect, data: the inputs' name (cases of one data name run the same tensors), partner: (case, "bitwise" | "splitk") --
# the case whose output this one is also compared with)
CASES = {}


def add(name, c, env, expect, data, partner=None):
    assert name not in CASES, name
    CASES[name] = dict(call=c, env=env, expect=expect, data=data, partner=partner)


# Three-product mode: fmt 0 with planes = 2, through ops.conv2d_planar (no workspace).  Shapes of CONV_CASES 0, 2 and 4; the first also with a
# residual (given as fp32 and as planes).
THREE_SHAPES = [CONV_CASES[0], CONV_CASES[2], CONV_CASES[4]]
for i, (B, H, W, C, O, kh, kw, s, pad, has_bias, _, relu) in enumerate(THREE_SHAPES):
    for tag, tile_n, env, (mg, nj) in (("t64", 64, {}, (1, 1)), ("t128_mg1", 128, {"STM_CONV_MG": "1"}, (1, 2)), ("t128_mg2", 128, {"STM_CONV_MG": "2"}, (2, 2))):
        add(f"three_{i}_{tag}", call(C, O, (kh, kw), B=B, hw=(H, W), stride=s, pad=pad, fmt=0, planes=2, tile_n=tile_n, ws=False, bias=has_bias, relu=relu,
                                     res="f32" if i == 0 else None), env, [(RING % (2, mg, nj, 0, 2, 0), 1)], f"three_{i}")

# Two-source (conv3 + projection): B, H2, W2, P, Cin, O, s2, tile_n as DUAL_CASES; every case runs without a residual, with an fp32 one and with
# a planar one (the GPU test loops; the plan does not depend on it)
DUAL_ROWS = [("a", (2, 25, 39, 128, 256, 512, 2, 64), {"STM_CONV_RING64": "2"}, (1, 1, 2), 1, None),
             ("b", (2, 25, 39, 64, 128, 256, 2, 128), {"STM_CONV_MG": "2"}, (2, 2, 3), 1, None),
             ("c", (2, 25, 39, 256, 512, 256, 2, 128), {"STM_CONV_MG": "2"}, (2, 2, 3), 2, "splitk"),
             ("c_unsplit", (2, 25, 39, 256, 512, 256, 2, 128), {"STM_CONV_MG": "2", "STM_CONV_SPLITK": "1"}, (2, 2, 3), 1, None)]
for fmt in (1, 2):
    for tag, (B, H2, W2, P, Cin, O, s2, tile_n), env, (mg, nj, st), sk, rel in DUAL_ROWS:
        Ho, Wo = (H2 - 1) // s2 + 1, (W2 - 1) // s2 + 1
        add(f"dual_{tag}_f{fmt}", call(P + Cin, O, 1, B=B, hw=(Ho, Wo), fmt=fmt, tile_n=tile_n, dual=(Cin, H2, W2, s2)), env,
            [(RING % (3 - fmt, mg, nj, 1, st, 1), sk)] + ([(FINISH, None)] if sk > 1 else []), f"dual_{tag[0]}_f{fmt}",
            (f"dual_c_unsplit_f{fmt}", rel) if rel else None)

# The head's geometry on the 128-wide tiles, fmt 1: five levels of three images, 969 pixels -- 8 tiles of 128 (the last holds 73) or 4 of 256 (the
# last holds 201); tiles span image rows, images and levels, and the last two levels are smaller than the kernel's halo.
HEAD_SIZES = [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]
HEAD_B = 3
MAIN = call(64, 512, 3, B=HEAD_B, sizes=HEAD_SIZES, groups=4)
add("head_main_ring", MAIN, {}, [(RING % (2, 1, 2, 1, 3, 0), 1)], "head_main")
add("head_main_mg2ring", MAIN, {"STM_CONV_MG": "2", "STM_CONV_KX3": "0"}, [(RING % (2, 2, 2, 1, 3, 0), 1)], "head_main")
add("head_main_kx3", MAIN, {"STM_CONV_MG": "2"}, [(KX3, 1)], "head_main", ("head_main_mg2ring", "bitwise"))
add("head_main_splitk", MAIN, {"STM_CONV_SPLITK": "2"}, [(RING % (2, 1, 2, 1, 3, 0), 2), (FINISH, None)], "head_main", ("head_main_ring", "splitk"))
add("head_main_mg2splitk", MAIN, {"STM_CONV_SPLITK": "2", "STM_CONV_MG": "2"}, [(RING % (2, 2, 2, 1, 3, 0), 2), (FINISH, None)], "head_main",
    ("head_main_mg2ring", "splitk"))
G2 = call(64, 256, (5, 3), B=HEAD_B, sizes=HEAD_SIZES, groups=2)                       # 30 K-slabs on 16 tiles: the rule itself splits K in two
add("head_g2_5x3_unsplit", G2, {"STM_CONV_SPLITK": "1"}, [(RING % (2, 1, 2, 1, 3, 0), 1)], "head_g2_5x3")
add("head_g2_5x3_splitk", G2, {}, [(RING % (2, 1, 2, 1, 3, 0), 2), (FINISH, None)], "head_g2_5x3", ("head_g2_5x3_unsplit", "splitk"))
K1X3 = call(96, 128, (1, 3), B=HEAD_B, sizes=HEAD_SIZES)
add("head_1x3_mg2ring", K1X3, {"STM_CONV_MG": "2", "STM_CONV_KX3": "0"}, [(RING % (2, 2, 2, 1, 3, 0), 1)], "head_1x3")
add("head_1x3_kx3", K1X3, {"STM_CONV_MG": "2"}, [(KX3, 1)], "head_1x3", ("head_1x3_mg2ring", "bitwise"))
# one group narrower than its 128 channels: not `full`, so never the kx-reuse kernel, whatever the tile height
NARROW = call(64, 512, 3, B=HEAD_B, sizes=HEAD_SIZES, groups=4, group_cout=[128, 128, 41, 128])
add("head_narrow_ring", NARROW, {}, [(RING % (2, 1, 2, 1, 3, 0), 1)], "head_narrow")
add("head_narrow_mg2", NARROW, {"STM_CONV_MG": "2"}, [(RING % (2, 2, 2, 1, 3, 0), 1)], "head_narrow", ("head_narrow_ring", "bitwise"))

# the seven rows that no fp64-oracle test launched before this list, with the cases that launch them now
SEVEN_ROWS = {RING % (2, 1, 1, 0, 2, 0): "three_*_t64", RING % (2, 1, 2, 0, 2, 0): "three_*_t128_mg1", RING % (2, 2, 2, 0, 2, 0): "three_*_t128_mg2",
              RING % (2, 1, 1, 1, 2, 1): "dual_a_f1", RING % (1, 1, 1, 1, 2, 1): "dual_a_f2", RING % (2, 2, 2, 1, 3, 1): "dual_b_f1, dual_c_f1, dual_c_unsplit_f1",
              RING % (1, 2, 2, 1, 3, 1): "dual_b_f2, dual_c_f2, dual_c_unsplit_f2"}


# ---- how the tests of tests/test_gpu_conv.py call the launcher ---------------------------------------------------------------------------
def existing_launches():
    """[(test, env, conv_plan_cases case)] of the oracle tests that were there before this list: test_conv_planar_vs_oracle, the two fp16-format
    tests, the loop variants, the two-source test, the kx3 test and the window-set test."""
    out = []
    for (B, H, W, C, O, kh, kw, s, pad, has_bias, has_res, relu) in CONV_CASES:
        shape = dict(B=B, hw=(H, W), stride=s, pad=pad, bias=has_bias, relu=relu, res="f32" if has_res else None)
        for tile_n, env in ((128, {"STM_CONV_MG": "1"}), (128, {"STM_CONV_MG": "2"}), (64, {})):
            out.append(("test_conv_planar_vs_oracle", env, plan_case(call(C, O, (kh, kw), fmt=0, tile_n=tile_n, ws=False, **shape))))
        for tile_n in (64, 128):
            out.append(("test_conv_planar_fp16_two_plane_format", {}, plan_case(call(C, O, (kh, kw), fmt=1, tile_n=tile_n, ws=False, **shape))))
            out.append(("test_conv_planar_fp16_one_plane_format", {}, plan_case(call(C, O, (kh, kw), fmt=2, tile_n=tile_n, **shape))))
    for fmt in (1, 2):
        for tile_n in (64, 128):
            for (B, H, W, C, O, k) in LOOP_CASES:
                for _, env in LOOP_VARIANTS:
                    out.append(("test_conv_planar_fp16_loop_variants_agree_bitwise", env, plan_case(call(C, O, k, B=B, hw=(H, W), fmt=fmt, tile_n=tile_n))))
        for (B, H2, W2, P, Cin, O, s2, tile_n) in DUAL_CASES:
            hw = ((H2 - 1) // s2 + 1, (W2 - 1) // s2 + 1)
            out.append(("test_conv_dual_source_vs_oracle", {}, plan_case(call(P + Cin, O, 1, B=B, hw=hw, fmt=fmt, tile_n=tile_n, dual=(Cin, H2, W2, s2)))))
    for _, B, sizes, C, O, groups, kh, with_res in KX3_CASES:
        where = dict(sizes=sizes) if len(sizes) > 1 else dict(hw=sizes[0])
        for kx3 in ("0", "1"):
            out.append(("test_conv_planar_kx3_staging_is_bit_equal_to_the_ring_kernel", {**KX3_ENV, "STM_CONV_KX3": kx3},
                        plan_case(call(C, O, (kh, 3), B=B, groups=groups, res="planes" if with_res else None, **where))))
    wt = WINDOW_TEST
    for h, w in wt["hw"]:
        case = dict(cc.CASES["windows_one"], g=cc.window_set(h, w, wt["n"], C=wt["C"], O=wt["O"]), windows=[win for _, win in border_windows(h, w)],
                    out32=cc.OUT32)
        out.append(("test_conv_window_launches_equal_the_padded_convolution", {}, case))
    return out
