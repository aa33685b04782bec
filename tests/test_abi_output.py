"""The second header of the C boundary, include/stmask_hip_output.h (the batched output stage): its prototypes, _lib.OUTPUT_SIGNATURES and the
argtypes of the loaded library say the same thing; its structs have the size of their ctypes mirrors; the first header's version is untouched."""
import ctypes
import os
import re

from conftest import ROOT
from stmask_amd import _lib

HEADER = os.path.join(ROOT, "include", "stmask_hip_output.h")

_C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t, "void": None, "const char*": ctypes.c_char_p}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _header_prototypes():
    """{name: (restype, [argtypes])} of every `ret stm_name(params);`: a `*` or `[` in a parameter, or the type stm_stream_t, makes it a pointer;
    every other parameter is `type name` with a scalar type (the parsing rule of tests/test_abi.py)."""
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


def test_output_header_and_signature_table_agree():
    protos = _header_prototypes()
    assert sorted(protos) == sorted(_lib.OUTPUT_SIGNATURES)
    assert len(protos) == 3 and "stm_output_stage_multi_f32" in protos
    assert sorted(set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", _header_text()))) == sorted(protos)     # no prototype the expression missed
    assert not set(_lib.OUTPUT_SIGNATURES) & set(_lib.SIGNATURES)
    lib = _lib.lib()
    for name, (ret_kind, kinds) in _lib.OUTPUT_SIGNATURES.items():
        ret, args = protos[name]
        fn = getattr(lib, name)
        assert fn.restype == ret == _lib._KINDS[ret_kind], (name, fn.restype, ret)
        assert len(fn.argtypes) == len(args) == len(kinds), (name, len(fn.argtypes), len(args))
        for i, (got, want, kind) in enumerate(zip(fn.argtypes, args, kinds)):
            assert got == want == _lib._KINDS[kind], (name, i, got, want)


def test_output_structs_have_the_size_of_their_mirrors():
    lib = _lib.lib()
    assert lib.stm_output_struct_bytes(0) == ctypes.sizeof(_lib.OutputFrame) == 32
    assert lib.stm_output_struct_bytes(1) == ctypes.sizeof(_lib.OutputRow) == 48
    assert lib.stm_output_struct_bytes(2) == ctypes.sizeof(_lib.OutputHeader) == 16
    assert lib.stm_output_struct_bytes(3) == 0
    # the fields the header names, in its order
    text = _header_text()
    for struct, mirror in (("stm_output_frame", _lib.OutputFrame), ("stm_output_row", _lib.OutputRow), ("stm_output_header", _lib.OutputHeader)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        names = [re.sub(r"\[\d+\]", "", w).strip() for decl in body.split(";") if decl.strip()
                 for w in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f[0] for f in mirror._fields_], struct
    for bit, name in ((1, "STM_ROW_KEPT"), (2, "STM_ROW_RUN_OVERFLOW"), (4, "STM_ROW_ARENA_OVERFLOW"), (8, "STM_ROW_BAD_FRAME")):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == bit
    assert (_lib.ROW_KEPT, _lib.ROW_RUN_OVERFLOW, _lib.ROW_ARENA_OVERFLOW, _lib.ROW_BAD_FRAME) == (1, 2, 4, 8)


def test_first_header_keeps_its_version():
    assert _lib.lib().stm_version() == 6 == _lib.ABI_VERSION
    assert "stm_output_stage_multi_f32" not in open(os.path.join(ROOT, "include", "stmask_hip.h")).read()


def test_call_counts_the_arguments_of_the_output_table():
    import pytest
    with pytest.raises(_lib.StmError):
        _lib.call("stm_output_stage_multi_f32", None, 1)
    # n == 0 is STM_OK before any pointer is looked at; n < 0 and NULL pointers are refused without a device
    args = [None, 0, 4, 4, None, None, None, 0, None, 0, None, None, None, 0, 0.0, 0.5, 16, None, 0, None, 0, None]
    _lib.call("stm_output_stage_multi_f32", *args)
    args[1] = -1
    with pytest.raises(_lib.StmError):
        _lib.call("stm_output_stage_multi_f32", *args)
    args[1] = 2
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_output_stage_multi_f32", *args)
    assert "non-NULL" in str(e.value)
