"""The third header of the C boundary, include/stmask_hip_tracker.h (the tracker's decisions on the device): its prototypes,
_lib.TRACKER_SIGNATURES and the argtypes of the loaded library say the same thing; the two older headers and the ABI version are untouched."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from stmask_amd import _lib

HEADER = os.path.join(ROOT, "include", "stmask_hip_tracker.h")

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


def test_tracker_header_and_signature_table_agree():
    protos = _header_prototypes()
    assert sorted(protos) == sorted(_lib.TRACKER_SIGNATURES) == ["stm_track_drop_plan", "stm_track_resolve_tf"]
    assert sorted(set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", _header_text()))) == sorted(protos)     # no prototype the expression missed
    assert not set(_lib.TRACKER_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.OUTPUT_SIGNATURES))
    lib = _lib.lib()
    for name, (ret_kind, kinds) in _lib.TRACKER_SIGNATURES.items():
        ret, args = protos[name]
        fn = getattr(lib, name)                                                                        # exported by the built library
        assert fn.restype == ret == _lib._KINDS[ret_kind], (name, fn.restype, ret)
        assert len(fn.argtypes) == len(args) == len(kinds), (name, len(fn.argtypes), len(args))
        for i, (got, want, kind) in enumerate(zip(fn.argtypes, args, kinds)):
            assert got == want == _lib._KINDS[kind], (name, i, got, want)


def test_older_headers_keep_their_lists_and_version():
    assert _lib.lib().stm_version() == 6 == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES) == 128 and len(_lib.OUTPUT_SIGNATURES) == 3
    for header in ("stmask_hip.h", "stmask_hip_output.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert not any(name in text for name in _lib.TRACKER_SIGNATURES), header


def test_call_checks_the_tracker_entries_without_a_device():
    with pytest.raises(_lib.StmError):
        _lib.call("stm_track_resolve_tf", None, None)                      # argument count
    none = [None] * 5
    for bad in ([0, 0, 0, 0], [1025, 0, 0, 0], [1, -1, 0, 0], [1, 0, -1, 0], [1, 0, 0, -1], [1, 2 ** 31 - 1, 1, 0]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_track_resolve_tf", *none, *bad, None, None, None, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_track_resolve_tf", *none, 2, 3, 4, 0, None, None, None, None)
    assert "NULL" in str(e.value)
    for bad in ([0, 0], [1025, 0], [1, -1]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_track_drop_plan", None, None, *bad, None, None, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_track_drop_plan", None, None, 2, 3, None, None, None)
    assert "NULL" in str(e.value)
