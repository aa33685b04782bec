"""The sixth header of the C boundary, include/stmask_hip_t2s_feat.h (T2S_concat_feat and its adjoint): its prototypes, _lib.T2S_FEAT_SIGNATURES
and the argtypes of the loaded library say the same thing; the five older headers, their tables and the ABI version are untouched; what the entry
points and their wrappers refuse is refused from the shapes, without a device."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from stmask_amd import _lib, layers, ops

HEADER = os.path.join(ROOT, "include", "stmask_hip_t2s_feat.h")
NAMES = ["stm_t2s_feat_backward_f32", "stm_t2s_feat_forward_f32"]

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


def test_t2s_feat_header_and_signature_table_agree():
    protos = _header_prototypes()
    assert sorted(protos) == sorted(_lib.T2S_FEAT_SIGNATURES) == NAMES
    assert sorted(set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", _header_text()))) == sorted(protos)     # no prototype the expression missed
    assert not set(_lib.T2S_FEAT_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.OUTPUT_SIGNATURES) | set(_lib.TRACKER_SIGNATURES) |
                                                set(_lib.TRAIN_SIGNATURES) | set(_lib.EVAL_SIGNATURES))
    lib = _lib.lib()
    for name, (ret_kind, kinds) in _lib.T2S_FEAT_SIGNATURES.items():
        ret, args = protos[name]
        fn = getattr(lib, name)                                                                        # exported by the built library
        assert fn.restype == ret == _lib._KINDS[ret_kind], (name, fn.restype, ret)
        assert len(fn.argtypes) == len(args) == len(kinds), (name, len(fn.argtypes), len(args))
        for i, (got, want, kind) in enumerate(zip(fn.argtypes, args, kinds)):
            assert got == want == _lib._KINDS[kind], (name, i, got, want)


def test_older_headers_keep_their_lists_and_version():
    assert _lib.lib().stm_version() == 6 == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES) == 128 and len(_lib.OUTPUT_SIGNATURES) == 3 and len(_lib.TRACKER_SIGNATURES) == 2
    assert len(_lib.TRAIN_SIGNATURES) == 8 and len(_lib.EVAL_SIGNATURES) == 4
    for header in ("stmask_hip.h", "stmask_hip_output.h", "stmask_hip_tracker.h", "stmask_hip_train.h", "stmask_hip_eval.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert not any(name in text for name in _lib.T2S_FEAT_SIGNATURES), header


def test_binding_refuses_a_library_without_the_new_entries(monkeypatch):
    """lib() lists the entries a stale library lacks instead of failing at the first call."""
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "T2S_FEAT_SIGNATURES", {**_lib.T2S_FEAT_SIGNATURES, "stm_t2s_feat_not_there": ("i", "p")})
    with pytest.raises(_lib.StmError) as e:
        _lib.lib()
    assert "stm_t2s_feat_not_there" in str(e.value) and "rebuild" in str(e.value)
    monkeypatch.undo()
    assert _lib.lib() is not None


def test_entry_points_refuse_from_the_shapes_without_a_device():
    fwd = lambda *dims: _lib.call("stm_t2s_feat_forward_f32", None, None, None, *dims, None)                        # noqa: E731
    bwd = lambda *dims: _lib.call("stm_t2s_feat_backward_f32", None, None, None, None, None, None, *dims, None)     # noqa: E731
    with pytest.raises(_lib.StmError):
        _lib.call("stm_t2s_feat_forward_f32", None, None)                                  # argument count
    #            bs  C  Cu  H  W  P
    for bad in ([0, 8, 4, 3, 4, 3], [1, 0, 4, 3, 4, 3], [1, 8, 0, 3, 4, 3], [1, 8, 4, 0, 4, 3], [1, 8, 4, 3, 0, 3], [1, 8, 4, 3, 4, 4], [1, 8, 4, 3, 4, 0],
                [1, 8, 4, 3, 4, -3], [1, 8, 4, 4096, 4096, 13], [1, 128, 4, 4096, 4096, 3], [1, 8, 128, 4096, 4096, 3]):
        for f in (fwd, bwd):
            with pytest.raises(_lib.StmError):
                f(*bad)
    for f in (fwd, bwd):
        with pytest.raises(_lib.StmError) as e:
            f(1, 8, 4, 3, 4, 3)                                                            # sizes fine: NULL pointers, before any launch
        assert "NULL" in str(e.value)


def test_wrappers_refuse_from_the_shapes_without_a_device():
    fpn, t2s = torch.zeros(4, 8, 3, 4), torch.zeros(4, 4, 3, 4)
    meta = lambda *shape: torch.empty(*shape, device="meta")                               # noqa: E731  (sizes only: nothing is allocated)
    bad = [(fpn[:3], t2s[:3], 3),                                                          # an odd image count
           (fpn, torch.zeros(4, 4, 3, 5), 3), (fpn, torch.zeros(4, 4, 2, 4), 3), (fpn, torch.zeros(2, 4, 3, 4), 3),
           (fpn, t2s.double(), 3), (fpn.half(), t2s.half(), 3),
           (fpn, t2s, 4), (fpn, t2s, 0), (fpn, t2s, -1),
           (fpn.transpose(2, 3).contiguous().transpose(2, 3), t2s, 3), (fpn, torch.zeros(4, 8, 3, 4)[:, ::2], 3),      # not contiguous
           (meta(2, 8, 4096, 4096), meta(2, 4, 4096, 4096), 13), (meta(2, 128, 4096, 4096), meta(2, 4, 4096, 4096), 3)]
    for f, t, P in bad:
        with pytest.raises(_lib.StmError):
            ops.t2s_check_shapes("t2s_concat_feat", f, t, P)
        if not f.is_meta:
            with pytest.raises(_lib.StmError):
                layers.t2s_concat_feat(f, t, patch_size=P, fused=True)
    if torch.cuda.is_available():
        with pytest.raises(_lib.StmError):
            ops.t2s_check_shapes("t2s_concat_feat", fpn.cuda(), t2s, 3)                    # two devices
    # shapes that are fine reach the device check: the product path has no CPU fallback
    with pytest.raises(_lib.StmError) as e:
        layers.t2s_concat_feat(fpn, t2s, patch_size=3, fused=True)
    assert "CPU" in str(e.value)
