"""plan_gather (the selections of hhgt_gather_calls: the row planner's cuts plus each block's output column) against a
brute-force enumeration, call_class_values / cast_class_values against hand-computed values in numpy and torch, and the
binding of hhgt_gather_calls against the header.  No device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd.store_plan import (GATHER_PLAN_DTYPE, MAX_FEATURE_BYTES, ROW_PLAN_DTYPE, mask_words_per_block,
                                                  plan_gather, plan_sample_counts)
from haplohyped_varawareml_amd.store_stats import call_class_values, cast_class_values, standardized_dosages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_force(samples, n_samples, sc, vc, bs, v_lo, v_hi, keep, col0):
    """every (chunk column, chunk row, block) the query touches, with what plan_gather must say about it; keep: bool over
    [v_lo, v_hi)"""
    vb, wpb = bs // 2, mask_words_per_block(bs)
    rows, col = [], col0
    samples = sorted(set(int(s) for s in samples))
    for B in range(v_lo // vb, (v_hi - 1) // vb + 1 if v_hi > v_lo else 0):
        a, b = max(v_lo, B * vb), min(v_hi, (B + 1) * vb)
        n = int(keep[a - v_lo:b - v_lo].sum())
        if n:
            for scol in sorted(set(s // sc for s in samples)):
                mask = sum(1 << (s % sc) for s in samples if s // sc == scol)
                rows.append((B * vb // vc, scol, (B * vb % vc) // vb, mask, a - B * vb, b - B * vb, scol * sc, B * wpb, col))
        col += n
    return sorted(rows), col


@pytest.mark.parametrize("sc,vc,bs", [(64, 8192, 8192), (40, 4096, 8192), (20, 96, 64)])
def test_plan_gather_matches_brute_force(sc, vc, bs):
    rng = np.random.default_rng(sc + bs)
    vb = bs // 2
    n_samples, n_variants = 3 * sc + 7, 7 * vb // 2 + 13
    cases = [(0, n_variants), (vb + 3, 2 * vb - 1), (vb - 1, vb + 1), (7, 7), (2 * vb, 3 * vb), (5, n_variants - 2)]
    for v_lo, v_hi in cases:
        for density in (0.0, 0.03, 1.0):
            keep = rng.random(v_hi - v_lo) < density
            if density == 0.03 and v_hi - v_lo > 2 * vb:
                keep[vb - v_lo % vb:2 * vb - v_lo % vb] = False               # a whole block without a gathered variant
            samples = rng.choice(n_samples, 30, replace=True)
            blocks = np.arange(v_lo, v_hi) // vb - v_lo // vb
            counts = np.bincount(blocks[keep], minlength=(blocks[-1] + 1 if len(blocks) else 0))
            for col0 in (0, 11):
                plan = plan_gather(samples, n_samples, sc, vc, n_variants, v_lo, v_hi, counts, blocksize=bs, col0=col0)
                assert plan.dtype == GATHER_PLAN_DTYPE
                want, end = brute_force(samples, n_samples, sc, vc, bs, v_lo, v_hi, keep, col0)
                got = sorted((int(p["vcol"]), int(p["scol"]), int(p["part"]), int(p["row_mask"]), int(p["lo"]), int(p["hi"]),
                              int(p["out_row"]), int(p["mask_word"]), int(p["out_col"])) for p in plan)
                assert got == want, (v_lo, v_hi, density, col0)
                assert end == col0 + int(keep.sum())
                # the row planner's cuts, minus the blocks that gather nothing, in the row planner's order
                rows = plan_sample_counts(samples, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize=bs)
                B = rows["vcol"] * (vc // vb) + rows["part"] - v_lo // vb
                kept = rows[counts[B] > 0] if len(rows) else rows
                for f in ROW_PLAN_DTYPE.names:
                    assert np.array_equal(plan[f], kept[f]), f
    assert GATHER_PLAN_DTYPE.names == ROW_PLAN_DTYPE.names + ("out_col",)
    assert ROW_PLAN_DTYPE.names == ("vcol", "scol", "part", "row_mask", "lo", "hi", "out_row", "mask_word", "out_word")
    assert MAX_FEATURE_BYTES == 4 << 30


def test_plan_gather_refuses_wrong_counts():
    args = ([0, 1], 100, 64, 8192, 20000, 100, 9000)
    with pytest.raises(ValueError):
        plan_gather(*args, [5, 5])                           # three blocks are touched
    with pytest.raises(ValueError):
        plan_gather(*args, [5, 5, 809])                      # the last block holds 808 variants of the range
    with pytest.raises(ValueError):
        plan_gather(*args, [3997, 5, 5])                     # the first one 3996
    assert len(plan_gather(*args, [3996, 0, 808])) == 2
    assert len(plan_gather([], 100, 64, 8192, 20000, 100, 9000, [1, 1, 1])) == 0
    assert len(plan_gather([3], 100, 64, 8192, 20000, 7, 7, [])) == 0


#                    AN  AC HET HOM
COUNTS = np.array([[10,  3,  1,  1],       # p = 0.3
                   [0,   0,  0,  0],       # nobody called
                   [8,   0,  0,  0],       # monomorphic REF
                   [6,   6,  0,  3],       # monomorphic ALT
                   [4,   2,  2,  0]],      # p = 0.5
                  dtype=np.int32)


def expected_values(coding, impute):
    nan = float("nan")
    miss = [nan] * 5
    if coding == "dosage":
        last = miss if impute == "missing" else [2 * 0.3, 0.0, 0.0, 2.0, 1.0]
        used = [True] * 5 if impute == "missing" else [True, False, True, True, True]
        return np.array([[0.0] * 5, [1.0] * 5, [2.0] * 5, last]), np.array(used)
    z = np.zeros((3, 5))
    for v, p in ((0, 0.3), (4, 0.5)):
        for d in range(3):
            z[d, v] = np.float32((d - 2 * p) / np.sqrt(2 * p * (1 - p)))
    return np.vstack([z, [miss if impute == "missing" else [0.0] * 5]]), np.array([True, False, False, False, True])


@pytest.mark.parametrize("coding", ["dosage", "standardized"])
@pytest.mark.parametrize("impute", ["mean", "missing"])
def test_call_class_values_by_hand(coding, impute):
    want, used = expected_values(coding, impute)
    v, u = call_class_values(COUNTS, coding, impute)
    assert v.dtype == np.float64 and v.shape == (4, 5) and u.dtype == bool
    assert np.array_equal(u, used)
    assert np.array_equal(v[:, used], want[:, used], equal_nan=True)
    tv, tu = call_class_values(torch.from_numpy(COUNTS), coding, impute)
    assert tv.dtype == torch.float64 and tu.dtype == torch.bool
    assert np.array_equal(tv.numpy().view(np.int64), v.view(np.int64)) and np.array_equal(tu.numpy(), u)      # the same bits
    if coding == "standardized":
        z, zu = standardized_dosages(COUNTS)
        assert np.array_equal(v[:3], z.astype(np.float64)) and np.array_equal(u, zu)


def test_call_class_values_dtype_and_arguments():
    for dtype in (torch.int8, np.int8, "int8", torch.int32):
        for coding in ("dosage", "standardized"):
            with pytest.raises(ValueError):
                call_class_values(COUNTS, coding, "mean", dtype)
        call_class_values(COUNTS, "dosage", "missing", dtype)
    for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64, np.float32, None):
        call_class_values(COUNTS, "dosage", "mean", dtype)
    for coding, impute in (("haplotypes", "mean"), ("dosage", "none"), ("additive", "missing")):
        with pytest.raises(ValueError):
            call_class_values(COUNTS, coding, impute)
    with pytest.raises(ValueError):
        call_class_values(COUNTS[:, :3], "dosage", "mean")
    # "missing" needs no counts: a table of zeros gives the same values
    a = call_class_values(COUNTS, "dosage", "missing")[0]
    b = call_class_values(np.zeros_like(COUNTS), "dosage", "missing")[0]
    assert np.array_equal(a, b, equal_nan=True)


def test_cast_applies_the_missing_marker():
    v = call_class_values(torch.from_numpy(COUNTS), "dosage", "missing")[0]
    i8 = cast_class_values(v, torch.int8)
    assert i8.dtype == torch.int8 and i8.tolist() == [[0] * 5, [1] * 5, [2] * 5, [-1] * 5]
    for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        f = cast_class_values(v, dtype)
        assert f.dtype == dtype and torch.isnan(f[3]).all() and torch.equal(f[:3], v[:3].to(dtype))
    m = call_class_values(torch.from_numpy(COUNTS), "dosage", "mean")[0]
    assert torch.equal(cast_class_values(m, torch.float16), m.to(torch.float16))


def header_prototype(name):
    src = open(os.path.join(ROOT, "include", "hhgt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    args = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src).group(1)
    return [" ".join(a.split()) for a in args.split(",")]


def test_lib_declares_hhgt_gather_calls_as_the_header_does():
    from haplohyped_varawareml_amd import _lib, build
    build.build()
    L = _lib.load()
    args = header_prototype("hhgt_gather_calls")
    assert args == ["hhgt_ctx *ctx", "const hhgt_gather_sel *d_sel", "uint32_t n_sel", "uint32_t sc", "uint32_t vc", "int typesize",
                    "int blocksize", "const uint32_t *d_vmask", "uint64_t vmask_words", "const uint32_t *d_row_map",
                    "uint64_t n_map", "const void *d_values", "int elem_bytes", "void *d_out", "uint64_t n_rows",
                    "uint64_t n_cols", "uint64_t row_stride", "uint64_t *n_bad", "void *stream"]
    scalar = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int}
    want = [ctypes.POINTER(ctypes.c_uint64) if a == "uint64_t *n_bad" else ctypes.c_void_p if "*" in a else scalar[a.split()[0]]
            for a in args]
    assert list(L.hhgt_gather_calls.argtypes) == want and L.hhgt_gather_calls.restype == ctypes.c_int
    # the same leading arguments as its sibling, and the selection record field for field
    assert header_prototype("hhgt_genotype_planes")[2:9] == args[2:9]
    src = open(os.path.join(ROOT, "include", "hhgt.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} hhgt_gather_sel;", re.sub(r"/\*.*?\*/", "", src, flags=re.S)).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in _lib.GatherSel._fields_]
    assert fields == ["src_ptr", "src_bytes", "row_mask", "out_row", "mask_word", "out_col", "part", "lo", "hi", "reserved"]
    assert ctypes.sizeof(_lib.GatherSel) == 64
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1))                    # noqa: E731
    assert define("HHGT_N_STAGES") == _lib.N_STAGES == len(_lib.STAGE_NAMES) == 16          # no stage of its own
