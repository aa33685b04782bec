"""The case list of tests/test_conv_plan_cpu.py: planar convolution calls described by their geometry, which pointers are present and how they are
aligned, the workspace, the second source, the window set, the gate and the STM_CONV_* switches.  No case touches a tensor: the pointers are
placeholder addresses, and neither the launcher's checks nor its launch plan read through them.

CASES is an ordered {name: case}.  dry_run(lib, case) asks stm_debug_conv2d_planar_plan for the case's launch lines; scripts/make_conv_plan_golden.py
drives the public entries of a patched build of the refactor's parent over the same list to write tests/golden/conv_plan.json."""
import ctypes
import os
import re

from stmask_amd import _lib
from stmask_amd.planar import border_windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, WT, BIAS, RES32, RESPL, OUT32, OUTPL, WS, X2, POOL, GATE = (0x10000 * i for i in range(1, 12))   # placeholder addresses, 16-byte aligned
BIG = 1 << 40                                                                                         # "sufficient" workspace bytes
TUNABLES = ("STM_CONV_RING", "STM_CONV_RING64", "STM_CONV_SPLITK", "STM_CONV_MG", "STM_CONV_KX3")
PLANES = {0: 3, 1: 2, 2: 1}

# conv_planar_kernel<NPL, MG, NJ, DT, ST, ABL, DUAL, CLS> of the default build: the 26 rows of PLANAR_ROWS (csrc/conv_bf16x.hip) and the window-set pair
ROWS = ([(3, 1, 1, 0, 2, 0), (2, 1, 1, 0, 2, 0)] + [(npl, 1, 1, 1, st, dual) for npl in (2, 1) for st in (2, 3) for dual in (0, 1)] +
        [(npl, mg, 2, 0, 2, 0) for npl in (3, 2) for mg in (1, 2)] + [(npl, mg, 2, 1, st, 0) for npl in (2, 1) for mg in (1, 2) for st in (2, 3)] +
        [(npl, mg, 2, 1, 3, 1) for npl in (2, 1) for mg in (1, 2)])
KERNELS = (["conv_planar_kernel<%d,%d,%d,%d,%d,0,%d,0>" % r for r in ROWS] +
           ["conv_planar_kernel<2,2,2,1,3,0,0,1>", "conv_planar_kernel<2,2,2,1,3,0,0,2>", "conv_planar_kx3_kernel<0,0>", "conv_planar_kx3_kernel<0,1>",
            "planar_splitk_finish_kernel"])

CASES = {}


def conv(M, C, O, k=1, s=1, fmt=1, tile=128, groups=1, **kw):
    """Geometry of a "same"-padded k x k / stride s layer with M output pixels (one image of Ho x Wo, Ho the largest divisor of M up to its root)."""
    ho = max(d for d in range(1, int(M ** 0.5) + 1) if M % d == 0)
    wo = M // ho
    kh, kw_ = (k, k) if isinstance(k, int) else k
    g = dict(B=1, H=ho * s, W=wo * s, C=C, Ho=ho, Wo=wo, Cout=O, kh=kh, kw=kw_, sh=s, sw=s, ph=(kh - 1) // 2, pw=(kw_ - 1) // 2, planes=PLANES[fmt],
             fmt=fmt, tile_n=tile, groups=groups)
    g.update(kw)
    return g


def add(name, g, env=None, **kw):
    """One case.  Keyword arguments replace the defaults: every tensor of a plain call present and aligned, planes out, no workspace."""
    assert name not in CASES, name
    case = dict(g=g, env=env or {}, x=X, w=WT, bias=BIAS, res32=0, respl=0, out32=0, outpl=OUTPL, relu=1, ws=0, ws_bytes=0, dual=None, windows=None,
                wptrs=None, pool=0, gate=0, n_windows=None)
    assert not set(kw) - set(case), kw
    case.update(kw)
    CASES[name] = case


def geom(case):
    if case["g"] is None:
        return None
    g = _lib.ConvGeom()
    for key, val in case["g"].items():
        if isinstance(val, (list, tuple)):
            for i, v in enumerate(val):
                getattr(g, key)[i] = v
        else:
            setattr(g, key, val)
    return g


def window_args(case):
    """(packed weight pointers, windows, count) of a case's window set, as ctypes arrays."""
    wins = case["windows"]
    arr = (_lib.ConvWindow * max(len(wins), 1))()
    for i, w in enumerate(wins):
        arr[i].kh, arr[i].kw, arr[i].ph, arr[i].pw, arr[i].Ho, arr[i].Wo, arr[i].y0, arr[i].x0 = w
    ptrs = case["wptrs"] if case["wptrs"] is not None else [WT + 0x100 * i for i in range(len(wins))]
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs), arr, case["n_windows"] if case["n_windows"] is not None else len(wins)


def dry_run(lib, case):
    """(status, launch lines, error text) of stm_debug_conv2d_planar_plan for the case.  The caller has set the case's switches."""
    g = geom(case)
    d = case["dual"] or dict(x2=0, C2=0, H2=0, W2=0, s2=0, np=0, ps=0)
    wp, wins, n = window_args(case) if case["windows"] is not None else (None, None, 0)
    buf = ctypes.create_string_buffer(4096)
    rc = lib.stm_debug_conv2d_planar_plan(case["x"], case["w"], case["bias"], case["res32"], case["respl"], case["out32"], case["outpl"],
                                          ctypes.byref(g) if g is not None else None, case["relu"], case["ws"], case["ws_bytes"],
                                          d["x2"], d["C2"], d["H2"], d["W2"], d["s2"], d["np"], d["ps"], wp, wins, n, case["pool"], case["gate"],
                                          buf, len(buf))
    return rc, buf.value.decode(), (lib.stm_last_error_string().decode() if rc else "")


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
# every kernel row: tile width x format x mixing mode x dual x pixel-tile group x loop, over a small and a large grid
for tile in (64, 128):
    for fmt, planes in ((0, 3), (0, 2), (1, 2), (2, 1)):
        for M in (1024, 256 * 300):
            for ring in ("3", "2"):
                env = {"STM_CONV_RING": ring, "STM_CONV_RING64": ring} if ring == "2" else {}
                add(f"rows_t{tile}_f{fmt}p{planes}_M{M}_ring{ring}", conv(M, 256, 256, 1, fmt=fmt, tile=tile, planes=planes), env)
                if fmt:
                    add(f"rows_dual_t{tile}_f{fmt}_M{M}_ring{ring}", conv(M, 256 + 128, 256, 1, fmt=fmt, tile=tile), env,
                        dual=dict(x2=X2, C2=128, H2=2 * conv(M, 32, 32)["Ho"], W2=2 * conv(M, 32, 32)["Wo"], s2=2, np=0, ps=0))

# 64-wide tiles: tile counts on both sides of 40, 128, 256 and 512, full and narrow groups, with and without a workspace
for t in (40, 41, 128, 129, 256, 257, 512, 513):
    for O in (64, 32):                                  # 32 real channels of a 64-wide tile: not "full"
        for ws in (0, WS):
            add(f"t64_tiles{t}_O{O}_ws{int(bool(ws))}", conv(128 * t, 256, O, 3, tile=64), ws=ws, ws_bytes=BIG)
# ... K lengths on both sides of 12, 24 and 40 slabs: a large grid (the ring rule) and a small one with a workspace (the split-K rule)
for slabs in (11, 12, 23, 24, 40, 41):
    add(f"t64_slabs{slabs}_large", conv(128 * 600, 32 * slabs, 64, 1, tile=64))
    for t in (40, 100):
        add(f"t64_slabs{slabs}_tiles{t}", conv(128 * t, 32 * slabs, 64, 1, tile=64), ws=WS, ws_bytes=BIG)
        add(f"t64_slabs{slabs}_tiles{t}_narrow", conv(128 * t, 32 * slabs, 64, 1, tile=64, group_cout=[41]), ws=WS, ws_bytes=BIG)
add("t64_full_groups", conv(1024, 256, 256, 3, tile=64, groups=4, group_cout=[64, 64, 64, 64]), ws=WS, ws_bytes=BIG)
add("t64_narrow_group", conv(1024, 256, 256, 3, tile=64, groups=4, group_cout=[64, 64, 5, 64]), ws=WS, ws_bytes=BIG)

# 128-wide tiles: 191 / 192 double tiles, 127 / 128 tiles
for n in (191, 192):
    add(f"t128_t2_{n}", conv(256 * n, 256, 128, 3))
    add(f"t128_t2_{n}_f2", conv(256 * n, 256, 128, 1, fmt=2))
for n in (127, 128):
    add(f"t128_tiles{n}", conv(128 * n, 256, 128, 3), ws=WS, ws_bytes=BIG)
for slabs in (23, 24):
    add(f"t128_slabs{slabs}", conv(128 * 16, 32 * slabs, 512, 1), ws=WS, ws_bytes=BIG)

# the workspace: absent, one byte short, misaligned, sufficient.  2048 pixels x 512 channels in 128-pixel tiles: 64 tiles of 72 slabs, four K parts
NEED = 4 * 2048 * 512 * 4
for name, ws, nbytes in (("absent", 0, NEED), ("short", WS, NEED - 1), ("misaligned", WS + 8, BIG), ("sufficient", WS, NEED)):
    add(f"ws_{name}", conv(2048, 256, 512, 3), ws=ws, ws_bytes=nbytes)
    add(f"ws_{name}_t64", conv(2048, 256, 512, 3, tile=64), ws=ws, ws_bytes=BIG if nbytes == BIG else nbytes - NEED // 2)     # 128 tiles: two K parts
add("gate_no_splitk", conv(2048, 256, 512, 3), ws=WS, ws_bytes=BIG, gate=GATE)
add("gate_no_splitk_t64", conv(2048, 256, 64, 3, tile=64), ws=WS, ws_bytes=BIG, gate=GATE)
add("gate_kx3", conv(256 * 300, 64, 128, 3), gate=GATE)

# kx-reuse eligibility: the layer that takes it, then each term failed on its own
KX3 = dict(M=256 * 300, C=64, O=128, k=3)
add("kx3_yes", conv(**KX3))
add("kx3_yes_5x3", conv(**{**KX3, "k": (5, 3)}))
add("kx3_pw0", conv(**KX3) | dict(pw=0, Wo=conv(**KX3)["Wo"] - 2))
add("kx3_stride2", conv(**KX3, s=2))
add("kx3_ph0", conv(**KX3) | dict(ph=0, Ho=conv(**KX3)["Ho"] - 2))
add("kx3_kh7", conv(**{**KX3, "k": (7, 3)}))
add("kx3_kw5", conv(**{**KX3, "k": (3, 5)}))
add("kx3_not_full", conv(**KX3, group_cout=[100]))
add("kx3_fmt2", conv(**KX3, fmt=2))
add("kx3_fmt0", conv(**KX3, fmt=0))
add("kx3_splitk", conv(**KX3), {"STM_CONV_SPLITK": "3"}, ws=WS, ws_bytes=BIG)
add("kx3_mg1", conv(**KX3), {"STM_CONV_MG": "1"})
add("kx3_small_mg2", conv(2048, 64, 128, 3), {"STM_CONV_MG": "2"})
add("kx3_small", conv(2048, 64, 128, 3))
add("kx3_ring2", conv(**KX3), {"STM_CONV_RING": "2"})
add("kx3_off", conv(**KX3), {"STM_CONV_KX3": "0"})
add("kx3_window", conv(**KX3) | dict(win_h=conv(**KX3)["Ho"], win_w=conv(**KX3)["Wo"], win_y0=0, win_x0=0))
# (a second source is a 1x1 launch: the "dual" term cannot fail without kw = 3 failing too; the case shows where such a launch goes instead)
add("kx3_dual_1x1", conv(256 * 300, 64 + 32, 128, 1), dual=dict(x2=X2, C2=32, H2=conv(**KX3)["Ho"], W2=conv(**KX3)["Wo"], s2=1, np=0, ps=0))

# the switches, each value the tests use
for env in ({"STM_CONV_RING": "2"}, {"STM_CONV_RING64": "2"}, {"STM_CONV_RING64": "4"}, {"STM_CONV_SPLITK": "1"}, {"STM_CONV_SPLITK": "3"},
            {"STM_CONV_SPLITK": "5"}, {"STM_CONV_MG": "1"}, {"STM_CONV_MG": "2"}, {"STM_CONV_KX3": "0"}):
    tag = "_".join(f"{k[9:].lower()}{v}" for k, v in env.items())
    for tile in (64, 128):
        for M in (2048, 256 * 300):
            for fmt in (1, 2):
                add(f"env_{tag}_t{tile}_M{M}_f{fmt}", conv(M, 256, 256, 3, fmt=fmt, tile=tile), env, ws=WS, ws_bytes=BIG)
    add(f"env_{tag}_t64_slabs72_large", conv(128 * 600, 256, 64, 3, tile=64), env)
    add(f"env_{tag}_t64_slabs8_small", conv(1024, 256, 64, 1, tile=64), env)

# multi-level launches (the shared head over the FPN levels) and the single window launch
LEVELS = dict(n_levels=5, lvl_h=[48, 24, 12, 6, 3], lvl_w=[80, 40, 20, 10, 5], lvl_start=[0, 3840, 4800, 5040, 5100, 5115])
for tile, O, k in ((128, 256, 3), (64, 192, 3), (128, 256, (3, 5)), (128, 256, (5, 3))):
    add(f"levels_t{tile}_k{k}".replace(" ", ""), conv(5115, 256, O, k, tile=tile) | LEVELS, ws=WS, ws_bytes=BIG)
add("levels_x8", conv(5115 * 8, 256, 256, 3) | {**LEVELS, "lvl_start": [8 * v for v in LEVELS["lvl_start"]]})
add("window_single", dict(conv(25 * 40, 256, 256, 3), B=40, H=7, W=7, Ho=5, Wo=5, ph=0, pw=0, win_h=7, win_w=7, win_y0=1, win_x0=1))
add("window_single_t64", dict(conv(25 * 40, 256, 256, 3, tile=64), B=40, H=7, W=7, Ho=5, Wo=5, ph=0, pw=0, win_h=7, win_w=7, win_y0=1, win_x0=1))
add("out_fmt_2_to_1", conv(4096, 256, 256, 1, fmt=2, out_fmt_plus1=2))
add("fp32_out_and_residuals", conv(4096, 256, 256, 1), out32=OUT32, res32=RES32, respl=RESPL)
add("fp32_out_unaligned", conv(4096, 256, 256, 1), out32=OUT32 + 4, outpl=0)


# window sets: TemporalNet's border classes, plain and pooled, with and without the kx-reuse form
def window_set(h, w, B, C=256, O=256, **kw):
    return dict(B=B, H=h, W=w, C=C, Cout=O, sh=1, sw=1, planes=2, fmt=1, tile_n=128, win_h=h, win_w=w, out_scale=0.5, **kw)


for h, w in ((7, 7), (5, 9), (3, 3)):
    wins = [win for _, win in border_windows(h, w)]
    for B in (4, 200):
        for env in ({}, {"STM_CONV_KX3": "0"}):
            tag = f"{h}x{w}_B{B}" + ("_kx3off" if env else "")
            add(f"windows_{tag}", window_set(h, w, B, C=640), env, windows=wins)
            add(f"windows_pool_{tag}", window_set(h, w, B), env, windows=wins, pool=POOL, outpl=0)
add("windows_one", window_set(7, 7, 30), windows=[(3, 3, 0, 0, 5, 5, 1, 1)])
add("windows_wide_rows", window_set(4, 200, 8), windows=[(3, 3, 0, 0, 2, 198, 1, 1)])          # 200 + 2 staged pixels per row: over the 384 rows
add("windows_kh7", window_set(9, 9, 8), windows=[(7, 3, 0, 0, 3, 7, 3, 1)])
# the sparse head's patch towers as PlanarConv.window_segments builds them: one window per kernel shape, 5x5 patches, valid 3x3 convolutions
SEGS = [(ho, wo, y0, x0) for ho, wo, y0, x0 in ((3, 3, 0, 0), (3, 1, 0, 1), (1, 3, 1, 0))]
for groups in (1, 2):
    add(f"gated_segments_g{groups}", dict(window_set(3, 3, 3 * 500, groups=groups), kh=3, kw=3, Ho=3, Wo=3, H=5, W=5),
        windows=[(3, 3, -y0, -x0, ho, wo, y0, x0) for ho, wo, y0, x0 in SEGS], wptrs=[WT] * 3, gate=GATE)
add("gated_segments_small", dict(window_set(3, 3, 3, groups=1), kh=3, kw=3, Ho=3, Wo=3, H=5, W=5),
    windows=[(3, 3, -y0, -x0, ho, wo, y0, x0) for ho, wo, y0, x0 in SEGS], wptrs=[WT] * 3, gate=GATE)


# the convolution rows of the recorded layer tables that ran on this launcher (tile column 64 or 128)
def layer_rows(path):
    rows = []
    for line in open(os.path.join(ROOT, "profiles", path)):
        m = re.match(r"\s*(\d+)\s+(\d+)\s+(\d+)\s+(\d)\s+(\d)\s+(\d)\s+(64|128)\s+\d+\s", line)
        if m:
            rows.append(tuple(int(v) for v in m.groups()))
    return rows


for path in ("r03_layer_table_32clips.txt", "r02_layer_table_8clips.txt"):
    for M, C, O, k, s, groups, tile in layer_rows(path):
        for fmt in (1, 2):
            name = f"layer_{M}_{C}_{O}_k{k}s{s}g{groups}_t{tile}_f{fmt}"
            if name not in CASES:
                g = conv(M, C, O, k, s, fmt=fmt, tile=tile, groups=groups)
                if (C, k, s) == (32, 7, 2):
                    # the stem's row: its 7x7 / stride 2 runs as a 7 x 1 convolution, stride (2, 1), padding (3, 0), over row patches whose 32 channels
                    # are the 7 column taps x 3 colours (planar.PlanarBackbone); the table prints kh and the row stride only
                    g = conv(M, C, O, (7, 1), fmt=fmt, tile=tile) | dict(sh=2)
                    g["H"] = 2 * g["Ho"]
                add(name, g, ws=WS, ws_bytes=BIG)

# every refusal, once
OK = conv(4096, 256, 256, 3)
add("bad_x_null", OK, x=0)
add("bad_w_null", OK, w=0)
add("bad_no_output", OK, outpl=0)
add("bad_geom_null", None)
add("bad_channels", OK | dict(C=48))
add("bad_cout_groups", OK | dict(groups=3))
add("bad_planes", OK | dict(planes=4))
add("bad_tile_n", OK | dict(tile_n=32))
add("bad_group_width", OK | dict(groups=4))                      # 64 channels per group on 128-wide tiles
add("bad_levels_stride", conv(5115, 256, 256, 3, s=2) | LEVELS)
add("bad_levels_count", conv(5115, 256, 256, 3) | {**LEVELS, "n_levels": 9})
add("bad_levels_start", conv(5115, 256, 256, 3) | {**LEVELS, "lvl_start": [1, 3841, 4801, 5041, 5101, 5116]})
add("bad_levels_images", conv(5115, 256, 256, 3) | {**LEVELS, "lvl_start": [0, 3841, 4801, 5041, 5101, 5116]})
add("bad_geometry", OK | dict(B=0))
add("bad_window_outside", OK | dict(win_h=64, win_w=64, win_y0=1, win_x0=0))
add("bad_conv_arithmetic", OK | dict(Ho=63))
add("bad_out_ld", OK | dict(out_ld=128), out32=OUT32)
add("bad_window_residual", OK | dict(win_h=64, win_w=64), respl=RESPL)
add("bad_x_np", OK | dict(x_np=4095))
add("bad_x_alignment", OK, x=X + 8)
add("bad_w_alignment", OK, w=WT + 4)
DUAL = dict(x2=X2, C2=128, H2=128, W2=128, s2=2, np=0, ps=0)
add("bad_dual_kernel", conv(4096, 384, 256, 3), dual=DUAL)
add("bad_dual_fmt0", conv(4096, 384, 256, 1, fmt=0), dual=DUAL)
add("bad_dual_size", conv(4096, 384, 256, 1), dual={**DUAL, "H2": 126})
add("bad_dual_channels", conv(4096, 384, 256, 1), dual={**DUAL, "C2": 384})
add("bad_dual_alignment", conv(4096, 384, 256, 1), dual={**DUAL, "x2": X2 + 8})
add("bad_dual_np", conv(4096, 384, 256, 1), dual={**DUAL, "np": 100})
add("bad_dual_window", conv(4096, 384, 256, 1) | dict(win_h=64, win_w=64), dual=DUAL)
add("bad_plane_2gib", conv(1 << 20, 1024, 256, 1))
add("bad_pixels_2_30", dict(conv(1, 32, 128, 1), ph=16384, pw=16384, Ho=32769, Wo=32769))
add("bad_pixels_2_24", dict(conv(1, 32, 128, 1), ph=2048, pw=2048, Ho=4097, Wo=4097))
add("bad_x_plane_stride", OK | dict(x_plane_stride=4096 * 8 * 32 + 4))
add("bad_taps", conv(4096, 256, 256, 6) | dict(ph=2, pw=2, Ho=63, Wo=63))
add("bad_out_fmt", conv(4096, 256, 256, 1, out_fmt_plus1=1))
add("bad_out_fmt_3", conv(4096, 256, 256, 1, fmt=2, out_fmt_plus1=4))
add("bad_fmt_planes", conv(4096, 256, 256, 1, fmt=1, planes=3))
add("bad_fmt0_planes", conv(4096, 256, 256, 1, fmt=0, planes=1))
W77 = [win for _, win in border_windows(7, 7)]
add("bad_windows_null", None, windows=W77)
add("bad_windows_count0", window_set(7, 7, 8), windows=W77, n_windows=0)
add("bad_windows_count", window_set(7, 7, 8), windows=W77 + W77[:1])
add("bad_windows_fmt", window_set(7, 7, 8) | dict(fmt=2, planes=1), windows=W77)
add("bad_windows_stride", window_set(7, 7, 8) | dict(sh=2), windows=W77)
add("bad_windows_weight_null", window_set(7, 7, 8), windows=W77, wptrs=[WT] * 8 + [0])
add("bad_windows_weight_alignment", window_set(7, 7, 8), windows=W77, wptrs=[WT] * 8 + [WT + 8])
add("bad_windows_groups", window_set(7, 7, 8, groups=2), windows=W77)
add("bad_windows_outside", window_set(7, 7, 8), windows=W77[:8] + [(2, 2, 0, 0, 1, 1, 7, 6)])
add("bad_windows_taps", window_set(7, 7, 8), windows=W77[:8] + [(6, 6, 0, 0, 1, 1, 0, 0)])
add("bad_windows_first_outside", window_set(7, 7, 8), windows=[(2, 2, 0, 0, 1, 1, 7, 6)] + W77[1:])
add("bad_windows_pixels", window_set(6, 6, 1 << 19, C=32, O=128), windows=[(1, 1, 0, 0, 1, 1, 0, 0), (1, 1, 0, 0, 6, 6, 0, 0)])
add("bad_windows_x_null", window_set(7, 7, 8), windows=W77, x=0)
add("bad_windows_no_output", window_set(7, 7, 8), windows=W77, pool=0, outpl=0)
add("bad_pool_cout", window_set(7, 7, 8, O=192), windows=W77, pool=POOL, outpl=0)
add("bad_pool_image", window_set(200, 200, 1), windows=[(3, 3, 0, 0, 198, 198, 1, 1)], pool=POOL, outpl=0)
add("bad_pool_alignment", window_set(7, 7, 8), windows=W77, pool=POOL + 4, outpl=0)
add("bad_pool_gate", window_set(7, 7, 8), windows=W77, pool=POOL, outpl=0, gate=GATE)
GSEG = dict(window_set(3, 3, 6), kh=3, kw=3, Ho=3, Wo=3, H=5, W=5)
GWIN = [(3, 3, -y0, -x0, ho, wo, y0, x0) for ho, wo, y0, x0 in SEGS]
add("bad_gated_segments", GSEG | dict(B=7), windows=GWIN, wptrs=[WT] * 3, gate=GATE)
add("bad_gated_kernel", GSEG, windows=GWIN[:2] + [(2, 3, -1, 0, 1, 3, 1, 0)], wptrs=[WT] * 3, gate=GATE)
add("bad_gated_outside", GSEG, windows=GWIN[:2] + [(3, 3, -1, 0, 3, 3, 1, 0)], wptrs=[WT] * 3, gate=GATE)
add("bad_gated_reads_outside", GSEG, windows=GWIN[:2] + [(3, 3, 0, 1, 1, 3, 1, 0)], wptrs=[WT] * 3, gate=GATE)
add("bad_gated_weight_alignment", GSEG, windows=GWIN, wptrs=[WT, WT, WT + 8], gate=GATE)
