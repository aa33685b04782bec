"""CPU-only checks of the drop-in boundary: every header of include/ and the table of stmask_amd/_lib.py that restates it say the same thing
(_lib.HEADERS lists them; EXPECTED below pins what each declares), the C-ABI library loads and exports every symbol, and the product path never
touches the oracle.  What is about one header only (what its entries refuse without a device, its defines) is in tests/test_abi_<header>.py."""
import ctypes
import os
import re

import pytest
import torch

from abi_header import assert_table_matches_header, header_raw, header_symbols, header_text, struct_field_names
from conftest import ROOT
from kernel_resources import kernel_resources
from stmask_amd import _lib, ops

# What every header declares, in the order of _lib.HEADERS: how many entries, and (but for the first header's 129) which.  The one place these live.
EXPECTED = {
    "stmask_hip.h": (129, None),
    "stmask_hip_output.h": (3, ["stm_output_stage_multi_f32", "stm_output_stage_workspace_bytes", "stm_output_struct_bytes"]),
    "stmask_hip_tracker.h": (2, ["stm_track_drop_plan", "stm_track_resolve_tf"]),
    "stmask_hip_train.h": (8, ["stm_lincomb_rows_proto_backward_f32", "stm_lincomb_rows_proto_backward_workspace_bytes", "stm_mbox_gather_f32",
                               "stm_mbox_positives", "stm_mbox_reduce_backward_f32", "stm_mbox_reduce_f32", "stm_mbox_scatter_coeff_f32",
                               "stm_mbox_workspace_bytes"]),
    "stmask_hip_eval.h": (4, ["stm_vis_match", "stm_vis_rle_check", "stm_vis_rle_decode", "stm_vis_tube_iou"]),
    "stmask_hip_t2s_feat.h": (2, ["stm_t2s_feat_backward_f32", "stm_t2s_feat_forward_f32"]),
    "stmask_hip_data.h": (5, ["stm_data_boxes_f32", "stm_data_frames_u8_f32", "stm_data_masks_u8", "stm_data_rle_starts", "stm_data_struct_bytes"]),
}
# mirror -> sizeof, where a size is part of the contract (ConvWindow is passed as an array: the size is the stride)
STRUCT_SIZES = {"ConvWindow": 32, "OutputFrame": 32, "OutputRow": 48, "OutputHeader": 16, "DataFrameDesc": 32, "DataMaskDesc": 16}
# mirror -> (header, struct) whose field names, in the header's order, are the mirror's
STRUCT_FIELDS = {"OutputFrame": ("stmask_hip_output.h", "stm_output_frame"), "OutputRow": ("stmask_hip_output.h", "stm_output_row"),
                 "OutputHeader": ("stmask_hip_output.h", "stm_output_header"), "DataFrameDesc": ("stmask_hip_data.h", "stm_data_frame_desc"),
                 "DataMaskDesc": ("stmask_hip_data.h", "stm_data_mask_desc")}


def test_headers_tables_and_expectations_are_the_same_list():
    assert list(_lib.HEADERS) == list(EXPECTED) == ["stmask_hip" + s + ".h" for s in ("", "_output", "_tracker", "_train", "_eval", "_t2s_feat", "_data")]
    assert sorted(_lib.HEADERS) == sorted(os.listdir(os.path.join(ROOT, "include")))          # a header nobody binds fails here
    tables = [_lib.SIGNATURES, _lib.OUTPUT_SIGNATURES, _lib.TRACKER_SIGNATURES, _lib.TRAIN_SIGNATURES, _lib.EVAL_SIGNATURES, _lib.T2S_FEAT_SIGNATURES,
              _lib.DATA_SIGNATURES]
    assert all(a is b for a, b in zip(_lib.HEADERS.values(), tables))                         # the module-level names are the tables lib() reads
    assert _lib.ABI_SYMBOLS == list(_lib.SIGNATURES)
    merged = _lib.all_signatures()
    assert len(merged) == sum(count for count, _ in EXPECTED.values()) and list(merged) == [n for t in tables for n in t]


@pytest.mark.parametrize("header", list(_lib.HEADERS))
def test_header_and_signature_table_agree(header):
    """Every argument of every entry point: the table lib() takes restype / argtypes from says what the header says."""
    assert_table_matches_header(header, _lib.HEADERS[header])


@pytest.mark.parametrize("header,name,wrong", [("stmask_hip_tracker.h", "stm_track_drop_plan", ("i", "ppiippi")),
                                               ("stmask_hip_tracker.h", "stm_track_drop_plan", ("i", "ppiipp")),
                                               ("dp_step.h", "stm_dp_sgd_finish_multi_f32", ("i", "ppppipppifffip")),
                                               ("dp_step.h", "stm_dp_sgd_finish_multi_f32", ("z", "ppppipppiffffp"))])
def test_a_wrong_table_entry_is_caught(header, name, wrong, monkeypatch):
    """The comparison can fail: one kind, the argument count or the return kind of one entry off, in a public and in a private table."""
    table = _lib.HEADERS.get(header) or _lib.PRIVATE_HEADERS[header]
    assert table[name] != wrong
    assert_table_matches_header(header, table)            # also binds the private entry from the table as it is
    monkeypatch.setitem(table, name, wrong)
    with pytest.raises(AssertionError, match=name):
        assert_table_matches_header(header, table)


@pytest.mark.parametrize("header", list(EXPECTED))
def test_header_declares_what_is_expected(header):
    count, names = EXPECTED[header]
    table = _lib.HEADERS[header]
    assert len(table) == len(header_symbols(header)) == count
    if names is not None:
        assert sorted(table) == header_symbols(header) == names and len(names) == count
    else:   # the first header: one prototype per line that starts with one of its return types
        assert len(re.findall(r"^[ \t]*(?:int|size_t|void|long long|const char\*)\s+stm_[a-z0-9_]+\s*\(", header_raw(header), flags=re.M)) == count


@pytest.mark.parametrize("header", list(_lib.HEADERS))
def test_no_entry_is_named_in_another_header(header):
    """Every entry belongs to one table and one header.  A newer header may mention an older entry in a comment; nothing else names another
    header's entry."""
    order = list(_lib.HEADERS)
    for other in order:
        if other == header:
            continue
        assert not set(_lib.HEADERS[header]) & set(_lib.HEADERS[other]), (header, other)
        text = header_raw(other) if order.index(other) < order.index(header) else header_text(other)
        assert not [name for name in _lib.HEADERS[header] if name in text], (header, other)


def test_abi_version_is_six_everywhere():
    assert _lib.lib().stm_version() == 6 == _lib.ABI_VERSION == int(re.search(r"#define STM_ABI_VERSION (\d+)", header_raw("stmask_hip.h")).group(1))


@pytest.mark.parametrize("header", list(_lib.HEADERS))
def test_a_library_without_an_entry_of_a_table_is_refused(header, monkeypatch):
    """lib() walks every table and lists the entries a stale library lacks: an StmError at load, not an AttributeError at the first call."""
    name = "stm_%s_not_there" % (header[len("stmask_hip_"):-2] or "first")
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.HEADERS[header], name, ("i", "p"))
    with pytest.raises(_lib.StmError) as e:
        _lib.lib()
    assert name in str(e.value) and "rebuild" in str(e.value)
    monkeypatch.undo()
    assert _lib.lib() is not None


@pytest.mark.parametrize("size_fn", list(_lib.STRUCTS))
def test_struct_layouts_of_binding_and_library_agree(size_fn):
    """A client built against another header revision passes a struct of another size: the *_struct_bytes functions let it find out
    (stm_conv_geom grew a trailing field in round 2 while the version stayed 1)."""
    mirrors = _lib.STRUCTS[size_fn]
    fn = getattr(ctypes.CDLL(_lib.LIB_PATH), size_fn)
    fn.restype = ctypes.c_size_t
    for i, mirror in enumerate(mirrors):
        assert fn(i) == ctypes.sizeof(mirror) == STRUCT_SIZES.get(mirror.__name__, ctypes.sizeof(mirror)), (size_fn, i, mirror.__name__)
        if mirror.__name__ in STRUCT_FIELDS:
            assert struct_field_names(*STRUCT_FIELDS[mirror.__name__]) == [f[0] for f in mirror._fields_], mirror.__name__
    assert fn(len(mirrors)) == 0 and fn(7) == 0


def test_every_pinned_struct_is_checked():
    checked = [m.__name__ for mirrors in _lib.STRUCTS.values() for m in mirrors]
    assert checked == ["DeformGeom", "ConvGeom", "ConvWindow", "HeadLayout", "FrameDesc", "RenderFrame", "OutputFrame", "OutputRow", "OutputHeader",
                       "DataFrameDesc", "DataMaskDesc"]
    assert set(STRUCT_SIZES) | set(STRUCT_FIELDS) <= set(checked)


def test_counts_keep_their_width():
    """stm_encode_boxes_f32 returns 0 for n == 0 before it looks at its pointers: a count cut to 32 bits would make 2**32 that (no launch happens)."""
    assert _lib.lib().stm_encode_boxes_f32(None, None, None, 2**32, None) == -2


def test_type_and_arity_errors_are_python_errors():
    with pytest.raises(ctypes.ArgumentError):
        _lib.lib().stm_encode_boxes_f32(None, None, None, ctypes.c_int(5), None)
    with pytest.raises(_lib.StmError):
        _lib.call("stm_encode_boxes_f32", None, None, None, 5)
    with pytest.raises(_lib.StmError):
        _lib.call("stm_encode_boxes_f32", None, None, None, 5, None, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_encode_boxes_f32", None, None, None, 5, None)
    assert "stm_encode_boxes_f32" in str(e.value) and "-2" in str(e.value) and "non-NULL" in str(e.value)


def test_library_loads_and_exports_every_symbol():
    _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for header in _lib.HEADERS:
        for name in header_symbols(header):
            assert hasattr(lib, name), f"{name} declared in include/{header} but not exported"
    lib.stm_version.restype = ctypes.c_int
    assert lib.stm_version() == _lib.ABI_VERSION
    assert int(re.search(r"#define STM_ABI_VERSION (\d+)", header_raw("stmask_hip.h")).group(1)) == _lib.ABI_VERSION


def test_library_targets_gfx950():
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in data


def test_argument_errors_are_reported_not_thrown():
    """Null pointers / bad sizes return STM_E* codes with a message (no compute, no GPU needed)."""
    lib = _lib.lib()
    rc = lib.stm_decode_boxes_f32(None, None, None, ctypes.c_int64(5), None)
    assert rc == -2 and b"non-NULL" in lib.stm_last_error_string()
    rc = lib.stm_cc_fast_nms_f32(None, None, None, 10, 41, None, ctypes.c_float(0.5), 4096, 1, None, None, None, None,
                                 None, None)
    assert rc in (-1, -2)
    g = _lib.DeformGeom(1, 6, 8, 8, 3, 3, 1, 1, 1, 1, 1, 1, 4, 8, 8)  # C % dg != 0
    rc = lib.stm_deform_im2col_f32(None, None, ctypes.c_int64(0), None, ctypes.c_int64(0), 0, None, ctypes.byref(g), 0,
                                   None)
    assert rc == -1 and b"deform groups" in lib.stm_last_error_string()
    g = _lib.DeformGeom(1, 8, 8, 8, 3, 3, 1, 1, 1, 1, 1, 1, 1, 9, 8)  # wrong Ho
    rc = lib.stm_deform_im2col_f32(None, None, ctypes.c_int64(0), None, ctypes.c_int64(0), 0, None, ctypes.byref(g), 0,
                                   None)
    assert rc == -1 and b"conv arithmetic" in lib.stm_last_error_string()


def test_cpu_tensors_fail_loudly():
    """No silent CPU fallback on the product path."""
    with pytest.raises(_lib.StmError):
        ops.decode(torch.zeros(4, 4), torch.zeros(4, 4))
    with pytest.raises(_lib.StmError):
        ops.corr_patch(torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8), 11)


def test_product_path_never_imports_oracle():
    pkg = os.path.join(ROOT, "stmask_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle", src, flags=re.M), f"{f} imports the oracle"
                assert "libstm_oracle" not in src, f"{f} references the oracle library"


def test_planar_conv_kernels_do_not_spill():
    """hipcc's resource report for csrc/conv_bf16x.hip: no instantiation of the planar convolution kernels may use scratch
    (a register spill in the MFMA loop costs 2x: seen once when the 128-wide body was duplicated)."""
    seen = 0
    for name, r in kernel_resources("conv_bf16x.hip").items():
        if "conv_planar_kernel" not in name and "conv_planar_kx3_kernel" not in name:
            continue
        seen += 1
        assert r.scratch == 0 and r.vgpr <= 256, (name, r.scratch, r.vgpr)
    assert seen >= 8
