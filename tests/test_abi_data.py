"""The seventh header of the C boundary, include/stmask_hip_data.h (training batches on the device): its prototypes, _lib.DATA_SIGNATURES and the
argtypes of the loaded library say the same thing; the six older headers, their tables and the ABI version are untouched."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from stmask_amd import _lib

HEADER = os.path.join(ROOT, "include", "stmask_hip_data.h")
NAMES = ["stm_data_boxes_f32", "stm_data_frames_u8_f32", "stm_data_masks_u8", "stm_data_rle_starts", "stm_data_struct_bytes"]

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


def test_data_header_and_signature_table_agree():
    protos = _header_prototypes()
    assert sorted(protos) == sorted(_lib.DATA_SIGNATURES) == NAMES
    assert sorted(set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", _header_text()))) == sorted(protos)     # no prototype the expression missed
    assert not set(_lib.DATA_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.OUTPUT_SIGNATURES) | set(_lib.TRACKER_SIGNATURES) |
                                            set(_lib.TRAIN_SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.T2S_FEAT_SIGNATURES))
    lib = _lib.lib()
    for name, (ret_kind, kinds) in _lib.DATA_SIGNATURES.items():
        ret, args = protos[name]
        fn = getattr(lib, name)                                                                        # exported by the built library
        assert fn.restype == ret == _lib._KINDS[ret_kind], (name, fn.restype, ret)
        assert len(fn.argtypes) == len(args) == len(kinds), (name, len(fn.argtypes), len(args))
        for i, (got, want, kind) in enumerate(zip(fn.argtypes, args, kinds)):
            assert got == want == _lib._KINDS[kind], (name, i, got, want)



def test_the_structs_have_the_sizes_the_library_was_compiled_with():
    lib = _lib.lib()
    assert lib.stm_data_struct_bytes(0) == ctypes.sizeof(_lib.DataFrameDesc) == 32
    assert lib.stm_data_struct_bytes(1) == ctypes.sizeof(_lib.DataMaskDesc) == 16
    assert lib.stm_data_struct_bytes(2) == 0
    text = open(HEADER).read()
    for struct, cls in (("stm_data_frame_desc", _lib.DataFrameDesc), ("stm_data_mask_desc", _lib.DataMaskDesc)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        # "type a, b;" declarations -> field names in order
        names = [n for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(const\s+)?\w+\*?\s+", "", decl.strip()).replace(" ", "").split(",")]
        assert names == [f[0] for f in cls._fields_], (struct, names)


def test_older_headers_keep_their_lists_and_version():
    assert _lib.lib().stm_version() == 6 == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES) == 128 and len(_lib.OUTPUT_SIGNATURES) == 3 and len(_lib.TRACKER_SIGNATURES) == 2
    assert len(_lib.TRAIN_SIGNATURES) == 8 and len(_lib.EVAL_SIGNATURES) == 4 and len(_lib.T2S_FEAT_SIGNATURES) == 2
    for header in ("stmask_hip.h", "stmask_hip_output.h", "stmask_hip_tracker.h", "stmask_hip_train.h", "stmask_hip_eval.h", "stmask_hip_t2s_feat.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert not any(name in text for name in _lib.DATA_SIGNATURES), header
    assert len(re.findall(r"^[ \t]*(?:int|size_t|void|long long|const char\*)\s+stm_[a-z0-9_]+\s*\(", open(os.path.join(ROOT, "include", "stmask_hip.h")).read(),
                          flags=re.M)) == 128


def test_a_library_without_a_data_entry_is_refused(monkeypatch):
    """lib() walks every table, DATA_SIGNATURES included: a name the library does not export is an StmError, not a late AttributeError."""
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.DATA_SIGNATURES, "stm_data_not_there", ("i", "p"))
    with pytest.raises(_lib.StmError) as e:
        _lib.lib()
    assert "stm_data_not_there" in str(e.value)
    monkeypatch.undo()
    _lib.lib()


def test_call_checks_the_data_entries_without_a_device():
    with pytest.raises(_lib.StmError):
        _lib.call("stm_data_masks_u8", None, None)                         # argument count
    n3, n4, n5 = [None] * 3, [None] * 4, [None] * 5
    # sizes refused before any pointer is looked at, NULL pointers before any launch
    for n, h, w, Hp, Wp in ([-1, 24, 40, 32, 64], [1, 0, 40, 32, 64], [1, 24, 40, 16, 64], [1, 24, 40, 32, 32]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_data_frames_u8_f32", None, n, None, h, w, Hp, Wp, None, None, 1, None)
        with pytest.raises(_lib.StmError):
            _lib.call("stm_data_masks_u8", *n3, 1, None, n, 0, None, h, w, Hp, Wp, None)
        with pytest.raises(_lib.StmError):
            _lib.call("stm_data_boxes_f32", None, None, n, None, h, w, Hp, Wp, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_data_masks_u8", *n3, 1, None, 1, 0, None, 24, 40, 32, 42, None)
    assert "multiple of 4" in str(e.value)
    for name, args in (("stm_data_frames_u8_f32", (None, 2, None, 24, 40, 32, 64, None, None, 1, None)),
                       ("stm_data_rle_starts", (*n5, 2, 10, *n4, None)),
                       ("stm_data_masks_u8", (*n3, 2, None, 2, 10, None, 24, 40, 32, 64, None)),
                       ("stm_data_boxes_f32", (None, None, 2, None, 24, 40, 32, 64, None))):
        with pytest.raises(_lib.StmError) as e:
            _lib.call(name, *args)
        assert "NULL" in str(e.value), name
    with pytest.raises(_lib.StmError):
        _lib.call("stm_data_rle_starts", *n5, -1, 0, *n4, None)
    with pytest.raises(_lib.StmError):
        _lib.call("stm_data_rle_starts", *n5, 1, -1, *n4, None)
    # a frame descriptor with a row stride below 3 * W0 is refused on the host
    d = (_lib.DataFrameDesc * 1)()
    d[0].ptr, d[0].H0, d[0].W0, d[0].row_stride_bytes = 4096, 4, 4, 11
    m3 = (ctypes.c_double * 3)(1, 1, 1)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_data_frames_u8_f32", d, 1, ctypes.c_void_p(4096), 24, 40, 32, 64, m3, m3, 1, None)
    assert "row stride" in str(e.value)
    # nothing to do launches nothing: no device, no pointers, no error
    _lib.call("stm_data_frames_u8_f32", None, 0, None, 24, 40, 32, 64, None, None, 1, None)
    _lib.call("stm_data_rle_starts", *n5, 0, 0, *n4, None)
    _lib.call("stm_data_masks_u8", *n3, 1, None, 0, 0, None, 24, 40, 32, 64, None)
    _lib.call("stm_data_boxes_f32", None, None, 0, None, 24, 40, 32, 64, None)
