"""The fourth header of the C boundary, include/stmask_hip_train.h (the batched mask term of the training criterion): its prototypes,
_lib.TRAIN_SIGNATURES and the argtypes of the loaded library say the same thing; the three older headers and the ABI version are untouched."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from stmask_amd import _lib

HEADER = os.path.join(ROOT, "include", "stmask_hip_train.h")
NAMES = ["stm_lincomb_rows_proto_backward_f32", "stm_lincomb_rows_proto_backward_workspace_bytes", "stm_mbox_gather_f32", "stm_mbox_positives",
         "stm_mbox_reduce_backward_f32", "stm_mbox_reduce_f32", "stm_mbox_scatter_coeff_f32", "stm_mbox_workspace_bytes"]

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


def test_train_header_and_signature_table_agree():
    protos = _header_prototypes()
    assert sorted(protos) == sorted(_lib.TRAIN_SIGNATURES) == NAMES
    assert sorted(set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", _header_text()))) == sorted(protos)     # no prototype the expression missed
    assert not set(_lib.TRAIN_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.OUTPUT_SIGNATURES) | set(_lib.TRACKER_SIGNATURES))
    lib = _lib.lib()
    for name, (ret_kind, kinds) in _lib.TRAIN_SIGNATURES.items():
        ret, args = protos[name]
        fn = getattr(lib, name)                                                                        # exported by the built library
        assert fn.restype == ret == _lib._KINDS[ret_kind], (name, fn.restype, ret)
        assert len(fn.argtypes) == len(args) == len(kinds), (name, len(fn.argtypes), len(args))
        for i, (got, want, kind) in enumerate(zip(fn.argtypes, args, kinds)):
            assert got == want == _lib._KINDS[kind], (name, i, got, want)


def test_older_headers_keep_their_lists_and_version():
    assert _lib.lib().stm_version() == 6 == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES) == 128 and len(_lib.OUTPUT_SIGNATURES) == 3 and len(_lib.TRACKER_SIGNATURES) == 2
    for header in ("stmask_hip.h", "stmask_hip_output.h", "stmask_hip_tracker.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert not any(name in text for name in _lib.TRAIN_SIGNATURES), header


def test_call_checks_the_train_entries_without_a_device():
    """Every refusal comes from the shapes, before a launch: nothing here needs a device."""
    lib = _lib.lib()
    assert lib.stm_mbox_workspace_bytes(0, 5) == 64 and lib.stm_mbox_workspace_bytes(1 << 11, (1 << 11) + 1) == 64
    assert lib.stm_mbox_workspace_bytes(2, 300) > 2 * 300 * 8
    for shape in ([0, 12, 20, 8], [65536, 12, 20, 8], [2, 0, 20, 8], [2, 12, 20, 16], [2, 1 << 15, 1 << 15, 8]):       # what the launch entry refuses
        assert lib.stm_lincomb_rows_proto_backward_workspace_bytes(*shape) == 64, shape
    assert lib.stm_lincomb_rows_proto_backward_workspace_bytes(2, 12, 20, 8) == 8 * 2 * 240 * 8 * 4 + 64              # 8 splits of [2,12,20,8] fp32
    assert lib.stm_lincomb_rows_proto_backward_workspace_bytes(3, 128, 176, 8) == 64                                   # more than 256 workgroups: no split
    with pytest.raises(_lib.StmError):
        _lib.call("stm_mbox_positives", None, None)                        # argument count
    for B, P, rows in ([0, 1, 0], [1, 0, 0], [1 << 11, (1 << 11) + 1, 0], [1, 1, -1], [1, 1, 65536]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_mbox_positives", None, None, B, P, rows, None, 0, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_mbox_positives", None, None, 2, 300, 0, None, 0, None)
    assert "NULL" in str(e.value)
    none7 = [None] * 7
    for n_rows, B, P, M in ([0, 2, 300, 8], [65536, 2, 300, 8], [4, 0, 300, 8], [4, 2, 300, 16], [4, 1 << 11, (1 << 11) + 1, 32]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_mbox_gather_f32", None, None, 0, None, None, None, 3, *none7, n_rows, B, P, M, 48, 80, None, 0, None)
        with pytest.raises(_lib.StmError):
            _lib.call("stm_mbox_scatter_coeff_f32", None, None, None, None, None, n_rows, B, P, M, None, 0, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_mbox_gather_f32", None, None, 0, None, None, None, 3, *none7, 4, 2, 300, 8, 48, 80, None, 0, None)
    assert "NULL" in str(e.value)
    for n_rows in (0, 65536):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_mbox_reduce_f32", None, None, None, None, None, n_rows, 1.0, None)
        with pytest.raises(_lib.StmError):
            _lib.call("stm_mbox_reduce_backward_f32", None, None, None, None, None, n_rows, 1.0, None)
    for h, w, m, n in ([12, 20, 16, 4], [0, 20, 8, 4], [12, 20, 8, 0], [12, 20, 8, 65536]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_lincomb_rows_proto_backward_f32", None, None, 2, None, None, None, None, None, h, w, m, n, None, 0, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_lincomb_rows_proto_backward_f32", None, None, 2, None, None, None, None, None, 12, 20, 8, 4, None, 0, None)
    assert "NULL" in str(e.value)
