"""The launch plan of the planar convolution (csrc/conv_plan.h, conv2d_planar_impl in csrc/conv_bf16x.hip) on the CPU: for every case of
tests/conv_plan_cases.py the dry run stm_debug_conv2d_planar_plan answers with the lines, or the status and error text, recorded in
tests/golden/conv_plan.json.  The golden was written by scripts/make_conv_plan_golden.py from the launcher as it was BEFORE the rules moved into
conv_plan.h (its launch sites patched to print instead of launching), so it is the behaviour the refactor had to keep, not the new code's
opinion of itself.  The coverage tests below read the golden, never the library: they say which kernels, thresholds, switches and refusals the case
list reaches."""
import json
import os
import re

import pytest

import conv_plan_cases as cc
from conftest import GOLDEN
from stmask_amd import _lib

with open(os.path.join(GOLDEN, "conv_plan.json")) as _f:
    GOLD = json.load(_f)

ROWS, KERNELS = cc.ROWS, cc.KERNELS      # (the kernels of the default build; tests/test_conv_rows_cpu.py reads the same list)


def lines(name):
    assert GOLD[name]["rc"] == 0, (name, GOLD[name])
    return GOLD[name]["text"].splitlines()


def first(name):
    """The first launch of a case as (kernel, {field: int})."""
    kernel, rest = lines(name)[0].split(" ", 1)
    return kernel, {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)(?= |$)", rest)}


def kernel_args(name):
    return tuple(int(v) for v in re.search(r"<(.*)>", first(name)[0]).group(1).split(","))


def test_case_list_and_golden_are_the_same_list():
    assert sorted(cc.CASES) == sorted(GOLD) and 300 <= len(GOLD) <= 800


def test_dry_run_equals_the_recorded_launcher(monkeypatch):
    lib = _lib.lib()
    wrong = []
    try:
        for name, case in cc.CASES.items():
            for k in cc.TUNABLES:
                monkeypatch.delenv(k, raising=False)
            for k, v in case["env"].items():
                monkeypatch.setenv(k, v)
            lib.stm_debug_reload_tunables()
            rc, text, err = cc.dry_run(lib, case)
            want = GOLD[name]
            if (rc, "" if rc else text, err) != (want["rc"], want["text"], want["error"]):
                wrong.append((name, rc, text, err, want))
    finally:
        monkeypatch.undo()
        lib.stm_debug_reload_tunables()
    assert not wrong, (len(wrong), wrong[:5])


def test_dry_run_reports_a_short_buffer_and_leaves_no_gate():
    import ctypes
    lib = _lib.lib()
    case = cc.CASES["ws_sufficient"]
    g = cc.geom(case)
    args = [case["x"], case["w"], case["bias"], 0, 0, 0, case["outpl"], ctypes.byref(g), 1, case["ws"], case["ws_bytes"], 0, 0, 0, 0, 0, 0, 0, None, None, 0, 0]
    buf = ctypes.create_string_buffer(40)
    assert lib.stm_debug_conv2d_planar_plan(*args, cc.GATE, buf, len(buf)) == -1 and b"does not fit 40 bytes" in lib.stm_last_error_string()
    assert lib.stm_debug_conv2d_planar_plan(*args, 0, None, 0) == -2
    # the gate of the first call was dropped with it: this one plans split-K again
    rc, text, _ = cc.dry_run(lib, case)
    assert rc == 0 and text == GOLD["ws_sufficient"]["text"] and "splitk=4" in text


# ---- what the case list reaches, read off the golden ---------------------------------------------------------------------------------------
def test_every_kernel_of_the_library_is_chosen():
    seen = {line.split()[0] for v in GOLD.values() if v["rc"] == 0 for line in v["text"].splitlines()}
    assert seen == set(KERNELS) and len(KERNELS) == 31 and len(set(ROWS)) == 26


def test_64_wide_tile_count_thresholds():
    for t, split in ((40, 6), (41, 4)):                                 # 72 slabs: min(256 / 40, 72 / 10) parts up to 40 tiles, min(256 / 41, 72 / 16) beyond
        assert first(f"t64_tiles{t}_O64_ws1")[1]["splitk"] == split
    assert first("t64_tiles128_O64_ws1")[1]["splitk"] == 2 and first("t64_tiles129_O64_ws1")[1]["splitk"] == 1      # full groups: up to 128 tiles
    assert first("t64_tiles256_O32_ws1")[1]["splitk"] == 3 and first("t64_tiles257_O32_ws1")[1]["splitk"] == 1      # narrow groups: up to 256 tiles
    assert first("t64_tiles128_O32_ws1")[1]["splitk"] == 6 and first("t64_tiles129_O32_ws1")[1]["splitk"] == 5      # (768 / tiles parts)
    # 72 slabs, no split: the ring (ST = 3) up to 512 workgroups, the two-buffer loop beyond; never for narrow groups
    assert kernel_args("t64_tiles512_O64_ws0")[4] == 3 and kernel_args("t64_tiles513_O64_ws0")[4] == 2
    assert kernel_args("t64_tiles512_O32_ws0")[4] == 2
    for t in (40, 41, 128, 129, 256, 257, 512, 513):
        assert first(f"t64_tiles{t}_O64_ws0")[1]["splitk"] == 1 and first(f"t64_tiles{t}_O64_ws0")[1]["m_tiles"] == t


def test_64_wide_slab_thresholds():
    st = {s: kernel_args(f"t64_slabs{s}_large")[4] for s in (11, 12, 23, 24, 40, 41)}
    assert st == {11: 2, 12: 3, 23: 3, 24: 3, 40: 3, 41: 2}              # 600 workgroups: the ring from 12 to 40 slabs
    for t in (40, 100):
        assert first(f"t64_slabs23_tiles{t}_narrow")[1]["splitk"] == 1 and first(f"t64_slabs24_tiles{t}_narrow")[1]["splitk"] == 2
    assert first("t64_slabs23_tiles40")[1]["splitk"] == 1 and first("t64_slabs24_tiles40")[1]["splitk"] == 2
    assert first("t64_slabs24_tiles100")[1]["splitk"] == 1 and first("t64_slabs41_tiles100")[1]["splitk"] == 2      # full groups past 40 tiles: 16 slabs per part
    assert first("t64_slabs40_tiles40")[1]["splitk"] == 4 and first("t64_slabs40_tiles100")[1]["splitk"] == 2
    # "full" against a narrow group of the same layer
    assert kernel_args("t64_full_groups")[4] == 3 and kernel_args("t64_narrow_group")[4] == 2
    assert first("t64_full_groups")[1]["splitk"] == 7 == first("t64_narrow_group")[1]["splitk"]      # 32 tiles x 72 slabs: 72 / 10 parts either way


def test_128_wide_thresholds():
    assert kernel_args("t128_t2_191")[1] == 1 and first("t128_t2_191")[0].startswith("conv_planar_kernel<")
    assert first("t128_t2_192")[0] == "conv_planar_kx3_kernel<0,0>" and first("t128_t2_192")[1]["block"] == 512
    assert kernel_args("t128_t2_191_f2")[1] == 1 and kernel_args("t128_t2_192_f2")[1] == 2
    assert first("t128_tiles127")[1]["splitk"] == 2 and first("t128_tiles128")[1]["splitk"] == 1
    assert first("t128_slabs23")[1]["splitk"] == 1 and first("t128_slabs24")[1]["splitk"] == 2


def test_workspace_and_gate():
    for suffix, parts in (("", 4), ("_t64", 2)):
        for name in ("absent", "short", "misaligned"):
            assert first(f"ws_{name}{suffix}")[1]["splitk"] == 1 and len(lines(f"ws_{name}{suffix}")) == 1
        assert first(f"ws_sufficient{suffix}")[1]["splitk"] == parts
        assert lines(f"ws_sufficient{suffix}")[1].startswith("planar_splitk_finish_kernel ")
    for name in ("gate_no_splitk", "gate_no_splitk_t64"):
        assert first(name)[1]["splitk"] == 1 and len(lines(name)) == 1
    assert first("gate_kx3")[0] == "conv_planar_kx3_kernel<0,0>"


def test_each_kx3_term_fails_on_its_own():
    assert first("kx3_yes")[0] == first("kx3_yes_5x3")[0] == "conv_planar_kx3_kernel<0,0>"
    for name in ("pw0", "stride2", "ph0", "kh7", "kw5", "not_full", "fmt2", "fmt0", "splitk", "mg1", "small", "ring2", "off", "window", "dual_1x1"):
        assert first(f"kx3_{name}")[0].startswith("conv_planar_kernel<"), name
    assert first("kx3_splitk")[1]["splitk"] == 3 and kernel_args("kx3_mg1")[1] == 1 and kernel_args("kx3_small")[1] == 1 and kernel_args("kx3_ring2")[4] == 2
    assert kernel_args("kx3_dual_1x1")[6] == 1 and kernel_args("kx3_dual_1x1")[1] == 2
    assert first("kx3_small_mg2")[0] == "conv_planar_kx3_kernel<0,0>"      # STM_CONV_MG=2 alone brings the small layer there


def test_each_switch_value_is_used_and_acts():
    envs = {tuple(sorted(c["env"].items())) for c in cc.CASES.values()}
    for want in (("STM_CONV_RING", "2"), ("STM_CONV_RING64", "2"), ("STM_CONV_RING64", "4"), ("STM_CONV_SPLITK", "1"), ("STM_CONV_SPLITK", "3"),
                 ("STM_CONV_SPLITK", "5"), ("STM_CONV_MG", "1"), ("STM_CONV_MG", "2"), ("STM_CONV_KX3", "0")):
        assert (want,) in envs, want
    assert kernel_args("env_ring2_t128_M76800_f1")[4] == 2 and kernel_args("env_ring2_t128_M2048_f2")[4] == 2
    assert kernel_args("env_ring642_t64_slabs8_small")[4] == 2 and kernel_args("env_ring644_t64_slabs72_large")[4] == 3
    assert kernel_args("rows_t64_f1p2_M1024_ring3")[4] == 3 and kernel_args("env_ring2_t64_slabs72_large")[4] == 2      # (without the switch)
    for tile in (64, 128):
        assert first(f"env_splitk1_t{tile}_M2048_f1")[1]["splitk"] == 1
        assert first(f"env_splitk3_t{tile}_M76800_f2")[1]["splitk"] == 3 and first(f"env_splitk5_t{tile}_M76800_f2")[1]["splitk"] == 5
    assert kernel_args("env_mg1_t128_M76800_f2")[1] == 1 and kernel_args("env_mg2_t128_M2048_f2")[1] == 2
    assert first("env_kx30_t128_M76800_f1")[0] == "conv_planar_kernel<2,2,2,1,3,0,0,0>"


def test_window_sets():
    for hw in ("7x7", "5x9", "3x3"):
        for pool in ("", "pool_"):
            for B in (4, 200):
                on, off = lines(f"windows_{pool}{hw}_B{B}"), lines(f"windows_{pool}{hw}_B{B}_kx3off")
                assert [ln.split()[0] for ln in off] == ["conv_planar_kernel<2,2,2,1,3,0,0,1>"]
                # 3x3 maps: the interior column is one pixel wide, and 257 window rows of 1 + 2 staged pixels are more than 384 rows
                assert [ln.split()[0] for ln in on] == ["conv_planar_kernel<2,2,2,1,3,0,0,1>"] + ([] if hw == "3x3" else ["conv_planar_kx3_kernel<0,1>"])
                assert sum(len(ln.split("cls=")[1].split(",")) for ln in on) == 9 == len(off[0].split("cls=")[1].split(","))
    assert [ln.split()[0] for ln in lines("windows_one")] == ["conv_planar_kx3_kernel<0,1>"]
    for name in ("windows_wide_rows", "windows_kh7"):                       # over 384 staged rows; a kernel of seven rows
        assert [ln.split()[0] for ln in lines(name)] == ["conv_planar_kernel<2,2,2,1,3,0,0,1>"]
    for name in ("gated_segments_g1", "gated_segments_g2", "gated_segments_small"):
        assert [ln.split()[0] for ln in lines(name)] == ["conv_planar_kernel<2,2,2,1,3,0,0,2>"] and lines(name)[0].count(":") == 3


def test_recorded_layer_tables_are_in_the_list():
    rows = {r for path in ("r03_layer_table_32clips.txt", "r02_layer_table_8clips.txt") for r in cc.layer_rows(path)}
    assert len(rows) >= 40 and {r[6] for r in rows} == {64, 128}
    for M, C, O, k, s, groups, tile in rows:
        for fmt in (1, 2):
            assert f"layer_{M}_{C}_{O}_k{k}s{s}g{groups}_t{tile}_f{fmt}" in GOLD


def test_every_refusal_is_hit():
    errors = {re.sub(r"\d+", "#", v["error"].split(": ", 1)[1]) for v in GOLD.values() if v["rc"]}
    codes = {v["rc"] for v in GOLD.values()}
    assert codes == {0, -1, -2, -5}
    for want in ("x_planes/packed_weight and at least one output must be non-NULL", "geometry is NULL", "bad channel / kernel / planes arguments",
                 "tile_n must be # or #", "Cout per group (#) must be a multiple of the tile width #",
                 "multi-level launches need stride # and same padding (<= # levels)", "lvl_start[#] must be #",
                 "level #: # pixels is not a whole number of #x# images", "bad geometry", "the #x# window at (#, #) leaves the #x# output image",
                 "Ho/Wo do not match the convolution arithmetic", "bad leading dimensions out_ld=# res_ld=#",
                 "window launches take no residual / second source", "x_np / out_np / res_np smaller than the pixel count",
                 "x_planes and packed_weight must be #-byte aligned", "#x# / stride # / one group / fp# plane formats only",
                 "second source # channels of #x# at stride # does not match the #x# output", "plane larger than # GiB", "too many output pixels",
                 "x_plane_stride must be a multiple of # elements", "more than # taps", "more than #^# output pixels in one launch",
                 "output format # cannot be produced by a format-# layer", "format # has # planes (planes = #)", "pooled window sets take no pixel gate",
                 "bad second-source plane geometry", "# images are not # equal segments", "the windows of a gated set share the layer's #x# kernel",
                 "window # (#x# at #, #) is not inside the #x# output", "window # reads outside the #x# input image",
                 "packed weight # is not #-byte aligned", "window sets run on the # x # ring tiles of the fp#x# format, one group unless gated",
                 "window # (#x# at #, #, kernel #x#) is not inside the #x# output", "more than #^# output pixels in one window",
                 # the window entries' own
                 "NULL argument", "# .. # windows", "fp#x# planes, stride #, #-channel tiles, win_h / win_w set", "packed weight # is NULL",
                 "fp#x# planes, stride #, one group, whole #-channel tiles, win_h / win_w set", "pooled images of at most # pixels",
                 "pool_fix must be #-byte aligned"):
        assert want in errors, want
    # each alignment and each second-source mismatch on its own
    for name, word in (("bad_x_alignment", "x_planes and packed_weight"), ("bad_w_alignment", "x_planes and packed_weight"),
                       ("bad_dual_alignment", "second-source plane geometry"), ("bad_dual_np", "second-source plane geometry"),
                       ("bad_dual_size", "does not match"), ("bad_dual_channels", "does not match"), ("bad_dual_kernel", "1x1 / stride 1"),
                       ("bad_dual_fmt0", "1x1 / stride 1"), ("bad_dual_window", "window launches take no"), ("bad_windows_weight_alignment", "packed weight 8"),
                       ("bad_gated_weight_alignment", "packed weight 2"), ("bad_pool_alignment", "pool_fix")):
        assert GOLD[name]["rc"] and word in GOLD[name]["error"], name
    # (not reachable through the entries: the gated set's "window sets run on the 256 x 128 ring tiles" -- stm_conv2d_planar_windows_f32 has refused
    # another format or tile width before -- and geom_ok's NULL / channel / planes checks, which conv2d_planar_impl makes first)
