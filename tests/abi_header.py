"""What tests/test_abi*.py read out of a header of include/ or a package-private one of stmask_amd/csrc/: its prototypes as ctypes types, its struct fields, and the comparison of a header
with the table of stmask_amd/_lib.py that restates it."""
import ctypes
import itertools
import os
import re

from conftest import ROOT
from stmask_amd import _lib

C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double,
           "size_t": ctypes.c_size_t, "void": None, "const char*": ctypes.c_char_p}


def header_path(header):
    """include/<header>, or stmask_amd/csrc/<header> for a package-private or internal one."""
    public = os.path.join(ROOT, "include", header)
    return public if os.path.exists(public) else os.path.join(ROOT, "stmask_amd", "csrc", header)


def header_raw(header):
    return open(header_path(header)).read()


def header_text(header):
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", "", header_raw(header), flags=re.S)


def header_symbols(header):
    return sorted(set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", header_text(header))))


def header_prototypes(header):
    """{name: (restype, [argtypes])} of every `ret stm_name(params);` of the header.  A `*` or `[` anywhere in a parameter, or the type
    stm_stream_t, makes it a pointer; every other parameter is `type name` with type one of the six scalar kinds."""
    protos = {}
    for ret, name, params in re.findall(r"^[ \t]*([A-Za-z_][A-Za-z0-9_ ]*?\**)\s*\b(stm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header_text(header), flags=re.M):
        args = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            words = p.split()
            pointer = "*" in p or "[" in p or words[0] == "stm_stream_t"
            args.append(ctypes.c_void_p if pointer else C_TYPES[" ".join(words[:-1])])
        assert name not in protos, name
        protos[name] = (C_TYPES[" ".join(ret.split())], args)
    return protos


def struct_field_names(header, struct):
    """The field names of `typedef struct NAME {...} NAME;` in the header's order: `type a, b;`, `type a[4];` and `const type* a;` declarations."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header_text(header), flags=re.S).group(1)
    return [re.sub(r"\[\d+\]", "", n).strip() for decl in body.split(";") if decl.strip()
            for n in re.sub(r"^(const\s+)?\w+\*?\s+", "", decl.strip()).split(",")]


def header_define(header, name):
    """The integer a `#define name ...` of the header stands for; a value that is another macro is looked up in the header and the csrc/ headers
    it includes."""
    text = header_raw(header)
    value = re.search(r"^#define %s (\w+)\s*(?:/[/*].*)?$" % name, text, flags=re.M).group(1)
    if re.fullmatch(r"\d+", value):
        return int(value)
    found = [h for h in [header] + re.findall(r'^#include "(\w+\.h)"', text, flags=re.M) if re.search(r"^#define %s " % value, header_raw(h), flags=re.M)]
    assert len(found) == 1, (header, name, value, found)
    return header_define(found[0], value)


def assert_table_matches_header(header, table):
    """Every argument of every entry point: the header, the table and the loaded library (whose restype / argtypes lib() or, for a
    package-private header, private_fn() took from the table) say the same thing."""
    protos = header_prototypes(header)
    assert sorted(protos) == sorted(table)
    assert header_symbols(header) == sorted(protos)                 # a prototype the expression misses fails here instead of skipping a function
    lib = _lib.lib()
    for name, (ret_kind, kinds) in table.items():
        ret, args = protos[name]
        fn = getattr(lib, name) if header in _lib.HEADERS else _lib.private_fn(name)      # exported by the built library
        assert fn.restype == ret == _lib._KINDS[ret_kind], (name, fn.restype, ret)
        # "-": one of the three ends before the others, so that an argument too few or too many is named by its index too
        for i, (got, want, kind) in enumerate(itertools.zip_longest(fn.argtypes, args, kinds, fillvalue="-")):
            assert got == want == _lib._KINDS.get(kind, "-"), (name, i, got, want, kind)
        assert len(fn.argtypes) == len(args) == len(kinds), (name, len(fn.argtypes), len(args), len(kinds))
