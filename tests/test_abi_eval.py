"""The fifth header of the C boundary, include/stmask_hip_eval.h (video mask AP on the device): its prototypes, _lib.EVAL_SIGNATURES and the
argtypes of the loaded library say the same thing; the four older headers, their tables and the ABI version are untouched."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from stmask_amd import _lib

HEADER = os.path.join(ROOT, "include", "stmask_hip_eval.h")
NAMES = ["stm_vis_match", "stm_vis_rle_check", "stm_vis_rle_decode", "stm_vis_tube_iou"]

_C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t, "void": None, "const char*": ctypes.c_char_p}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _header_prototypes():
    """{name: (restype, [argtypes])} of every `ret stm_name(params);` -- the parsing rule of tests/test_abi.py: a `*` or `[` in a parameter, or
    the type stm_stream_t, makes it a pointer; every other parameter is `type name` with a scalar type."""
    protos = {}
    for ret, name, params in re.findall(r"^[ \t]*([A-Za-z_][A-Za-z0-9_ ]*?\**)\s*\b(stm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header_text(), flags=re.M):
        args = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            words = p.split()
            pointer = "*" in p or "[" in p or words[0] == "stm_stream_t"
            args.append(ctypes.c_void_p if pointer else _C_TYPES[" ".join(words[:-1])])
        assert name not in protos, name
        protos[name] = (_C_TYPES[" ".join(ret.split())], args)
    return protos


def test_eval_header_and_signature_table_agree():
    protos = _header_prototypes()
    assert sorted(protos) == sorted(_lib.EVAL_SIGNATURES) == NAMES
    assert sorted(set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", _header_text()))) == sorted(protos)     # no prototype the expression missed
    assert not set(_lib.EVAL_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.OUTPUT_SIGNATURES) | set(_lib.TRACKER_SIGNATURES) |
                                            set(_lib.TRAIN_SIGNATURES))
    lib = _lib.lib()
    for name, (ret_kind, kinds) in _lib.EVAL_SIGNATURES.items():
        ret, args = protos[name]
        fn = getattr(lib, name)                                                                        # exported by the built library
        assert fn.restype == ret == _lib._KINDS[ret_kind], (name, fn.restype, ret)
        assert len(fn.argtypes) == len(args) == len(kinds), (name, len(fn.argtypes), len(args))
        for i, (got, want, kind) in enumerate(zip(fn.argtypes, args, kinds)):
            assert got == want == _lib._KINDS[kind], (name, i, got, want)


def test_header_limits_match_the_python_side():
    from stmask_amd import vis_eval
    defines = dict(re.findall(r"^#define (STM_VIS_[A-Z_]+) (\d+)", open(HEADER).read(), flags=re.M))
    assert int(defines["STM_VIS_MAX_DET"]) == vis_eval.MAX_DET == vis_eval.MAX_DETS[-1] == 100
    assert int(defines["STM_VIS_MAX_GT"]) == vis_eval.MAX_GT
    assert int(defines["STM_VIS_MAX_THREADS"]) >= len(vis_eval.IOU_THRS) * len(vis_eval.AREA_RNG) == 40
    assert (int(defines["STM_VIS_RLE_UNTERMINATED"]), int(defines["STM_VIS_RLE_RANGE"]), int(defines["STM_VIS_RLE_SUM"])) == (
        vis_eval.RLE_UNTERMINATED, vis_eval.RLE_RANGE, vis_eval.RLE_SUM)


def test_older_headers_keep_their_lists_and_version():
    assert _lib.lib().stm_version() == 6 == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES) == 128 and len(_lib.OUTPUT_SIGNATURES) == 3 and len(_lib.TRACKER_SIGNATURES) == 2
    assert len(_lib.TRAIN_SIGNATURES) == 8
    for header in ("stmask_hip.h", "stmask_hip_output.h", "stmask_hip_tracker.h", "stmask_hip_train.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert not any(name in text for name in _lib.EVAL_SIGNATURES), header


def test_call_checks_the_eval_entries_without_a_device():
    with pytest.raises(_lib.StmError):
        _lib.call("stm_vis_rle_decode", None, None)                        # argument count
    n3, n4 = [None] * 3, [None] * 4
    # sizes refused before any pointer is looked at, NULL pointers before any launch
    for n, total in ([-1, 0], [1, -1], [1, 2 ** 31]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_vis_rle_decode", *n3, n, total, *n4, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_vis_rle_decode", *n3, 2, 10, *n4, None)
    assert "NULL" in str(e.value)
    with pytest.raises(_lib.StmError):
        _lib.call("stm_vis_rle_check", *n3, -1, 0, *n3, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_vis_rle_check", *n3, 2, 10, *n3, None)
    assert "NULL" in str(e.value)
    for n_pairs, n_tracks, frames, n_masks in ([-1, 0, 0, 0], [2 ** 31, 1, 1, 1], [1, -1, 0, 0], [1, 0, -1, 0], [1, 0, 0, -1]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_vis_tube_iou", None, None, n_pairs, None, None, n_tracks, frames, *n4, n_masks, *n3, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_vis_tube_iou", None, None, 3, None, None, 2, 2, *n4, 4, *n3, None)
    assert "NULL" in str(e.value)

    def match(n_groups, max_d, max_g, n_thr, n_area):
        _lib.call("stm_vis_match", *n4, n_groups, max_d, max_g, *n4, n_thr, None, n_area, *n3, None)

    for bad in ([-1, 1, 1, 10, 4], [1, 101, 1, 10, 4], [1, 1, 1025, 10, 4], [1, -1, 1, 10, 4], [1, 1, -1, 10, 4], [1, 1, 1, 0, 4], [1, 1, 1, 10, 0],
                [1, 1, 1, 13, 5]):
        with pytest.raises(_lib.StmError):
            match(*bad)
    with pytest.raises(_lib.StmError) as e:
        match(1, 101, 1, 10, 4)
    assert "101" in str(e.value) and "100" in str(e.value)
    with pytest.raises(_lib.StmError) as e:
        match(2, 100, 1024, 10, 4)
    assert "NULL" in str(e.value)
    # nothing to do launches nothing: no device, no pointers, no error
    _lib.call("stm_vis_rle_decode", *n3, 0, 0, *n4, None)
    _lib.call("stm_vis_rle_check", *n3, 0, 0, *n3, None)
    _lib.call("stm_vis_tube_iou", None, None, 0, None, None, 0, 0, *n4, 0, *n3, None)
    match(0, 0, 0, 10, 4)
