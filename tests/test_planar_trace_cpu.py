"""The Python half of the planar launch path on the CPU: every case of tests/planar_trace.py sends across the C boundary exactly the calls recorded
in tests/golden/planar_trace.json.gz -- entry, numbers, struct fields, and for every pointer the storage it points into, that storage's size and the
offset.  The golden was written by scripts/make_planar_trace_golden.py from the commit BEFORE PlanarConv.__call__ became a sequence of steps
(scripts/planar_trace_golden_parent.md), so it is the behaviour a change of stmask_amd/planar.py has to keep, not the new code's opinion of
itself.  The coverage tests read the golden only: they say which entries, arguments and refusals the case list reaches."""
import gzip
import json
import os
import re

import pytest

from conftest import GOLDEN
from stmask_amd import _lib

if not os.path.exists(_lib.LIB_PATH):
    pytest.skip("libstmask_hip.so not built (run __graft_entry__.build())", allow_module_level=True)

import planar_trace as pt   # noqa: E402

with gzip.open(os.path.join(GOLDEN, "planar_trace.json.gz"), "rt") as _f:
    GOLD = json.load(_f)


def test_case_list_and_golden_are_the_same_list():
    assert sorted(pt.CASES) == sorted(GOLD) and sum(len(v) for v in GOLD.values()) > 2000


@pytest.mark.parametrize("name", list(pt.CASES))
def test_trace_equals_the_recorded_parent(name):
    got, want = pt.run_case(name), GOLD[name]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{name}: call {i} differs\n  now:      {a}\n  recorded: {b}"
    assert len(got) == len(want), f"{name}: {len(got)} calls, recorded {len(want)}; first extra: {(got + want)[min(len(got), len(want))]}"


def test_tracing_restores_what_it_patched():
    import torch
    from stmask_amd import ops, planar
    before = (ops.call, planar.call, ops.conv_set_pixel_gate, ops._dev, ops._stream, ops.planar_range_flag, torch.cuda.current_device,
              torch.cuda.current_stream, torch.cuda.is_current_stream_capturing, planar.TN_POOL, planar.FMT)
    pt.run_case("temporal_n335_no_pool")
    assert before == (ops.call, planar.call, ops.conv_set_pixel_gate, ops._dev, ops._stream, ops.planar_range_flag, torch.cuda.current_device,
                      torch.cuda.current_stream, torch.cuda.is_current_stream_capturing, planar.TN_POOL, planar.FMT)


def test_a_pointer_into_no_live_tensor_is_an_error():
    rec = pt.Recorder()
    with pytest.raises(pt.TraceError):
        rec.call("stm_planar_set_range_flag", 0x10)


# ---- what the case list reaches, read off the golden ---------------------------------------------------------------------------------------------
def entries(name):
    return [ln.split(" ", 1)[0] for ln in GOLD[name]]


def test_forward_passes_reach_the_entries_of_the_graph():
    dense = entries("forward_r50_fp16x2_dense")
    assert 120 <= len(dense) <= 200 and {"stm_conv2d_planar_ws_f32", "stm_conv2d_planar_dual_f32", "stm_stem_fused_f32", "stm_bottleneck_chain_f32",
                                         "stm_dcn_sample_planar_fmt_f32", "stm_head_assemble_f32"} <= set(dense)
    # (frames this small stay below the thresholds of the kx-reuse kernel and of the fused deformable convolution: one case lowers both)
    assert not {"stm_conv2d_planar_kxr_f32", "stm_deform_conv_fused_planar_f32"} & set(dense)
    assert {"stm_conv2d_planar_kxr_f32", "stm_deform_conv_fused_planar_f32"} <= set(entries("forward_r50_fp16x2_dense_kxr_fused"))
    for k in ("center", "shapes"):
        assert "stm_conv2d_planar_kxr_f32" in entries(f"forward_r50_fp16x2_sparse_{k}_kxr")
    for k in pt.SPARSE:
        e = entries(f"forward_r50_fp16x2_sparse_{k}")
        assert {"stm_head_candidates_f32", "stm_head_patch_gather", "stm_head_patch_mask", "stm_head_assemble_sparse_f32", "conv_set_pixel_gate"} <= set(e)
        assert ("stm_conv2d_planar_windows_f32" in e) == (k == "shapes")
    # four different launch sequences: the setting without a capacity and a centre flag gets the default ones, which at this size are `center`'s
    assert len({tuple(GOLD[f"forward_r50_fp16x2_sparse_{k}"]) for k in pt.SPARSE}) == 4
    assert GOLD["forward_r50_fp16x2_sparse_pos"] == GOLD["forward_r50_fp16x2_sparse_center"]
    assert any(",fmt=2," in ln for ln in GOLD["forward_r50_fp16x1_dense"]) and not any(",fmt=2," in ln for ln in dense)
    assert not any(",fmt=" in ln for ln in GOLD["forward_r50_bf16x3_dense"] if ln.startswith("stm_conv2d_planar_ws_f32"))
    for cfg in ("ada", "ali"):
        fused = [entries(f"forward_{cfg}_{s}").count("stm_deform_conv_fused_planar_f32") for s in ("default", "fused_min_tiles_1")]
        assert fused[0] < fused[1]
        assert "stm_deform_sample_planar_f32" in entries(f"forward_{cfg}_default")
        assert "stm_deform_conv_fwd_f32" in entries(f"forward_{cfg}_fcb_module") and "stm_deform_conv_fwd_f32" not in entries(f"forward_{cfg}_default")
    assert "stm_fcb_ali_offsets_f32" in entries("forward_ali_default")


def test_temporal_net_paths():
    assert entries("temporal_n8").count("stm_conv2d_planar_ws_f32") == 3
    assert entries("temporal_n335_pool")[-2:] == ["stm_conv2d_planar_windows_pool_f32", "stm_temporal_pool_fc_f32"]
    assert entries("temporal_n335_no_pool").count("stm_conv2d_planar_windows_f32") == 3 and entries("temporal_n335_pool").count("stm_conv2d_planar_windows_f32") == 2


def test_every_refusal_of_the_layer_is_hit_once():
    errors = {name: GOLD[name][-1] for name in GOLD if name.startswith("direct_error_")}
    assert len(errors) >= 25 and all(ln.startswith("raise StmError: ") for ln in errors.values()), errors
    assert len(set(re.sub(r"\d+", "#", ln) for ln in errors.values())) >= 20      # (some sites have two ways in)
    assert not any(ln.startswith("raise ") for name, lines in GOLD.items() if not name.startswith("direct_error_") for ln in lines)
    assert len(pt.UNREACHED) == 7


def test_kernel_choice_on_either_side_of_the_threshold():
    kern = lambda name: entries("direct_" + name)[-1]
    kxr, ws = "stm_conv2d_planar_kxr_f32", "stm_conv2d_planar_ws_f32"
    assert [kern(f"kxr_{o}_{side}") for o in (None, True, False) for side in ("at", "below")] == [kxr, ws, kxr, kxr, ws, ws]
    assert kern("kxr_residual") == ws and kern("kxr_grouped_at") == kxr and kern("window_one_pixel_kxr") == kxr and kern("window_one_pixel_general") == ws
    assert entries("direct_kxr_twice").count("stm_conv_pack_weights_kxr_f32") == 1
    tiles = [int(re.search(r"tile_n=(\d+)", ln).group(1)) for ln in GOLD["direct_tile_both"] if ln.startswith(ws)]
    assert tiles == [64, 128, 64] and entries("direct_tile_both").count("stm_conv_pack_weights_fmt_f32") == 2
    assert "tile_n=64" in GOLD["direct_tile_64"][-1] and "tile_n=128" in GOLD["direct_tile_128"][-1]
    # a gate: the gate call precedes the launch, and the launch gets no split-K workspace; splitk=False alone: no workspace either
    for name in ("gate", "gate_splitk_off"):
        assert entries("direct_" + name)[-2:] == ["conv_set_pixel_gate", ws] and GOLD["direct_" + name][-1].endswith(" null 0 null")
    assert GOLD["direct_splitk_off"][-1].endswith(" null 0 null") and not GOLD["direct_plain_planes"][-1].endswith(" null 0 null")


def test_rule_table_covers_the_workload():
    rows = GOLD["rule_table"]
    for cfg in (pt.R50, pt.R101):
        for clips in (1, 4, 8, 32):
            mine = [r for r in rows if r.startswith(f"rule {cfg} clips={clips} ")]
            assert len(mine) >= 40 and {"up", "tower1", "tower2", "finals.0.small", "finals.0.trk"} <= {r.split()[3] for r in mine}
    assert {re.search(r"kernel=(\d+)", r).group(1) for r in rows} == {"0", "64", "128"}
