"""CPU-only checks of the package-private boundary: every header of _lib.PRIVATE_HEADERS (stmask_amd/csrc/) and the table that restates it say
the same thing, the library exports the entries, nothing of the drop-in boundary names them, the struct mirrors of _lib.PRIVATE_STRUCTS have the
library's sizes and every #define that Python mirrors has the Python value.  What is about one header's entries only (what they refuse without a
device) is in the test file of the feature."""
import ctypes
import os

import pytest

import det_restate
from abi_header import assert_table_matches_header, header_define, header_raw, header_symbols
from conftest import ROOT
from stmask_amd import _lib, optim

# What every private header declares, in the order of _lib.PRIVATE_HEADERS.  The one place these live.
EXPECTED = {
    "optim.h": ["stm_grads_nonfinite_multi_f32", "stm_sgd_step_multi_f32"],
    "extra_aug.h": ["stm_aug_frames_u8_f32", "stm_aug_masks_u8", "stm_aug_source_u8", "stm_aug_struct_bytes"],
    "fold.h": ["stm_fold_rows_f32", "stm_fold_struct_bytes"],
    "dp_step.h": ["stm_dp_sgd_finish_multi_f32"],
    "det_backward.h": ["stm_deform_col2im_det_f32", "stm_det_exponent", "stm_det_workspace_bytes", "stm_roi_align_backward_det_f32",
                       "stm_upsample_bilinear_backward_f32"],
    "jpeg.h": ["stm_jpeg_decode_u8", "stm_jpeg_struct_bytes", "stm_jpeg_workspace_bytes"],
}
# private header -> (header of csrc/ that holds the #define, macro, the Python names that mirror it: all equal)
DEFINES = {
    "optim.h": [("optim.h", "STM_OPTIM_MAX_TENSORS", (optim.MAX_TENSORS,)), ("optim.h", "STM_OPTIM_CHUNK", (optim.CHUNK,))],
    "extra_aug.h": [("extra_aug.h", "STM_AUG_FRAMES_PER_LAUNCH", (_lib.AUG_FRAMES_PER_LAUNCH,))],
    "fold.h": [("fold.h", "STM_FOLD_" + m, (v,)) for m, v in (("MAX_ROWS", _lib.FOLD_MAX_ROWS), ("CHUNK", _lib.FOLD_CHUNK), ("COPY", _lib.FOLD_COPY),
                                                             ("WEIGHT", _lib.FOLD_WEIGHT), ("BIAS", _lib.FOLD_BIAS))],
    "dp_step.h": [("dp_step.h", "STM_DP_MAX_TENSORS", (_lib.DP_MAX_TENSORS, optim.MAX_TENSORS)), ("dp_step.h", "STM_DP_CHUNK", (_lib.DP_CHUNK, optim.CHUNK))],
    "det_backward.h": [("det_accum.h", "STM_DET_MIN_BITS", (_lib.DET_MIN_BITS, det_restate.MIN_BITS, 36)),
                       ("det_accum.h", "STM_DET_FINITE", (_lib.DET_FINITE, det_restate.FINITE)),
                       ("det_accum.h", "STM_DET_ZERO", (_lib.DET_ZERO, det_restate.ZERO)),
                       ("det_accum.h", "STM_DET_NONFINITE", (_lib.DET_NONFINITE, det_restate.NONFINITE))],
    "jpeg.h": [("jpeg.h", "STM_JPEG_" + m, (getattr(_lib, "JPEG_" + m),)) for m in ("MAX_DIM", "LOOK_BITS", "DECODE", "RAW", "ENOCODE", "EINDEX", "ESIZE",
                                                                                   "ETRUNCATED", "STAGE_ENTROPY", "STAGE_IDCT", "STAGE_COLOUR")],
}


def test_the_private_boundary_is_six_headers_beside_an_unchanged_public_one():
    assert list(_lib.PRIVATE_HEADERS) == list(EXPECTED) == list(DEFINES) == ["optim.h", "extra_aug.h", "fold.h", "dp_step.h", "det_backward.h", "jpeg.h"]
    tables = [_lib.PRIVATE_SIGNATURES, _lib.AUG_SIGNATURES, _lib.FOLD_SIGNATURES, _lib.DP_SIGNATURES, _lib.DET_SIGNATURES, _lib.JPEG_SIGNATURES]
    assert all(a is b for a, b in zip(_lib.PRIVATE_HEADERS.values(), tables))           # the module-level names are the tables private_fn() reads
    assert _lib.ABI_VERSION == 6 and len(_lib.HEADERS) == 7 and len(_lib.SIGNATURES) == 129
    assert not set(_lib.PRIVATE_HEADERS) & set(os.listdir(os.path.join(ROOT, "include")))
    public = [m for mirrors in _lib.STRUCTS.values() for m in mirrors]
    assert [m.__name__ for mirrors in _lib.PRIVATE_STRUCTS.values() for m in mirrors] == ["AugDesc", "FoldRow", "JpegImage", "JpegSegment", "JpegTables"]
    assert not [m for mirrors in _lib.PRIVATE_STRUCTS.values() for m in mirrors if m in public]
    assert all(sum(size_fn in t for t in tables) == 1 for size_fn in _lib.PRIVATE_STRUCTS)


@pytest.mark.parametrize("header", list(_lib.PRIVATE_HEADERS))
def test_header_and_signature_table_agree(header):
    """Every argument of every entry point: the table private_fn() takes restype / argtypes from says what the header says."""
    table = _lib.PRIVATE_HEADERS[header]
    assert sorted(table) == header_symbols(header) == EXPECTED[header]
    assert_table_matches_header(header, table)


@pytest.mark.parametrize("header", list(_lib.PRIVATE_HEADERS))
def test_library_exports_the_entries_and_nothing_else_lists_them(header):
    lib = ctypes.CDLL(_lib.LIB_PATH)
    public_text = {h: header_raw(h) for h in os.listdir(os.path.join(ROOT, "include"))}
    for name in _lib.PRIVATE_HEADERS[header]:
        assert hasattr(lib, name), f"{name} declared in csrc/{header} but not exported"
        assert name not in _lib.all_signatures()
        assert not [h for h, t in _lib.PRIVATE_HEADERS.items() if h != header and name in t], name
        assert not [h for h, text in public_text.items() if name in text], name


@pytest.mark.parametrize("header", list(_lib.PRIVATE_HEADERS))
def test_private_call_refuses_a_wrong_argument_count(header):
    for name, (_, kinds) in _lib.PRIVATE_HEADERS[header].items():
        for n in (len(kinds) - 1, len(kinds) + 1):
            with pytest.raises(_lib.StmError, match=f"{name} takes {len(kinds)} arguments, got {n}"):
                _lib.private_call(name, *[None] * n)


@pytest.mark.parametrize("size_fn", list(_lib.PRIVATE_STRUCTS))
def test_struct_mirrors_have_the_library_sizes(size_fn):
    mirrors = _lib.PRIVATE_STRUCTS[size_fn]
    fn = _lib.private_fn(size_fn)
    assert [fn(i) for i in range(len(mirrors))] == [ctypes.sizeof(m) for m in mirrors]
    assert fn(len(mirrors)) == 0 and fn(7) == 0 and fn(-1) == 0


def test_a_mirror_of_another_size_is_refused_when_its_header_is_first_bound(monkeypatch):
    """A stale library would read garbage past a shorter struct: binding any entry of the header checks the header's mirrors first."""
    monkeypatch.setattr(_lib, "_private_calls", {})
    monkeypatch.setitem(_lib.PRIVATE_STRUCTS, "stm_fold_struct_bytes", [_lib.AugDesc])
    for _ in range(2):                                   # refused again: a failed check binds nothing
        with pytest.raises(_lib.StmError, match="struct 0 of stm_fold_struct_bytes has 72 bytes, this binding's mirror AugDesc 112: rebuild"):
            _lib.private_call("stm_fold_rows_f32", None, 0, None)
    assert _lib._private_calls == {}
    monkeypatch.undo()
    _lib.private_call("stm_fold_rows_f32", None, 0, None)


@pytest.mark.parametrize("header", list(DEFINES))
def test_defines_equal_their_python_mirrors(header):
    for where, macro, mirrors in DEFINES[header]:
        assert all(header_define(where, macro) == m for m in mirrors), (where, macro, header_define(where, macro), mirrors)
