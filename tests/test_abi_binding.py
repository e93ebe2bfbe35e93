"""CPU: the Python binding says what the headers say.  The records of include/hhgt.h are described once more as ctypes
structures (_lib.py), from which device.py derives its numpy records, and every function the package calls has its
prototype in _lib.PROTOTYPES: both are held against the header text here, field by field and parameter by parameter.
Needs no libhhgt.so."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from haplohyped_varawareml_amd import _lib, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RECORDS = {"hhgt_layout": _lib.Layout, "hhgt_encode_stats": _lib.EncodeStats, "hhgt_encode_result": _lib.EncodeResultRec,
           "hhgt_block_sel": _lib.BlockSel, "hhgt_count_sel": _lib.CountSel, "hhgt_sample_sel": _lib.SampleSel,
           "hhgt_plane_sel": _lib.PlaneSel, "hhgt_window": _lib.Window}
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "uint8_t": C.c_uint8, "char": C.c_char, "double": C.c_double, "float": C.c_float}


def _header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


HHGT_H = _header("hhgt.h")
MACROS = {m: int(v) for m, v in re.findall(r"^#define\s+(HHGT_\w+)\s+(\d+)\s*$", HHGT_H, flags=re.M)}


def header_fields(record):
    """[(name, ctypes type)] of `typedef struct { ... } record;` in include/hhgt.h"""
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*%s\s*;" % record, HHGT_H).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        base = SCALARS[ctype] if ctype in SCALARS else RECORDS[ctype]
        for item in names.split(","):
            name, dims = re.fullmatch(r"\s*(\w+)\s*((?:\[\w+\])*)\s*", item).groups()
            t = base
            for d in reversed(re.findall(r"\[(\w+)\]", dims)):      # char a[16][32]: 16 arrays of 32
                t = t * (MACROS[d] if d in MACROS else int(d))
            fields.append((name, t))
    return fields


@pytest.mark.parametrize("record", sorted(RECORDS))
def test_structure_is_the_header_record(record):
    want = header_fields(record)
    assert len(want) >= 5
    assert [(n, t) for n, t in RECORDS[record]._fields_] == want


def _param_class(ctype):
    """'ptr', or the scalar type itself (ctypes knows int and int32_t as one type, as the ABI does)"""
    if ctype is None:
        return "void"
    if ctype in (C.c_void_p, C.c_char_p) or issubclass(ctype, C._Pointer):
        return "ptr"
    return ctype


def header_prototypes():
    """{name: (class of the return value, [class of each parameter])} of the functions of hhgt.h, hhgt_synth.h and hhgt_reader.h"""
    protos = {}
    for src in (HHGT_H, _header("hhgt_synth.h"), _header("hhgt_reader.h")):
        for ret, name, params in re.findall(r"^((?:const\s+)?\w+\s*\**)\s*(hhgt_\w+)\s*\(([^()]*)\)\s*;", src, flags=re.M):
            def cls(decl, with_name):
                decl = re.sub(r"\bconst\b", " ", decl).strip()
                if "*" in decl:
                    return "ptr"
                words = decl.split()
                assert len(words) == (2 if with_name else 1), decl
                return "void" if words[0] == "void" else SCALARS[words[0]]
            plist = [] if params.strip() == "void" else [cls(p, True) for p in params.split(",")]
            assert name not in protos
            protos[name] = (cls(ret, False), plist)
    return protos


def test_prototype_table_is_the_headers():
    declared = header_prototypes()
    assert len(declared) >= 58 and "hhgt_synth_render_mixed" in declared and "hhgt_reserve" in declared
    assert "hhgt_reader_acquire" in declared and "hhgt_crc32" in declared
    assert len(_lib.PROTOTYPES) >= 58 and "hhgt_reader_acquire" in _lib.PROTOTYPES
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        assert name in declared, f"{name} is in no header"
        ret, params = declared[name]
        assert _param_class(restype) == ret, name
        assert len(argtypes) == len(params), name
        for i, (a, p) in enumerate(zip(argtypes, params)):
            assert _param_class(a) == p, f"{name}: parameter {i}"


def test_package_binds_no_prototype_elsewhere():
    """the renderers' prototypes used to be bound on first use in device.py, the reader's in reader.py and sharding.py"""
    from haplohyped_varawareml_amd import reader, sharding
    for module in (device, reader, sharding):
        src = open(module.__file__).read()
        assert "argtypes" not in src and "restype" not in src, module.__name__


@pytest.mark.parametrize("dtype,struct,size", [(device.SEL_DTYPE, _lib.BlockSel, 40), (device.COUNT_SEL_DTYPE, _lib.CountSel, 48),
                                               (device.SAMPLE_SEL_DTYPE, _lib.SampleSel, 56),
                                               (device.PLANE_SEL_DTYPE, _lib.PlaneSel, 64)])
def test_numpy_records_are_the_structures(dtype, struct, size):
    assert dtype == np.dtype(struct) and dtype.itemsize == C.sizeof(struct) == size
    assert list(dtype.names) == [n for n, _ in struct._fields_]
    for name, ctype in struct._fields_:
        assert dtype.fields[name][0] == np.dtype(ctype) and dtype.fields[name][1] == getattr(struct, name).offset
