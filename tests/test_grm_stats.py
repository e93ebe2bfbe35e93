"""CPU: the statistics behind the genetic relationship matrix — store.standardized_dosages and grm_from_sums on numpy and on
CPU torch tensors (the same bits) and against a direct float64 restatement on a random genotype matrix with missing,
half-missing and allele-2 calls; the row sums of S on complete data; top_eigenpairs' order, sign rule and refusals; the
ctypes declaration of hhgt_grm and GRM_SPAN against include/hhgt.h."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd.store import (AC, AN, GRM_SPAN, grm_from_sums, standardized_dosages, top_eigenpairs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bound on an entry of S relative to T = sum |x_i x_j|: a chain of 32 * GRM_SPAN fused multiply-adds in float32
# (gamma_K ~ K 2^-24) and the two float32 roundings of z in every product; the float64 additions on top are 2^-29 of that
S_BOUND = (32 * GRM_SPAN + 4) * 2.0 ** -24


def np_counts(g):
    """int8 [S, V, 2] -> int64 [V, 4]: AN, AC (the other two columns are not read here)"""
    out = np.zeros((g.shape[1], 4), np.int64)
    out[:, AN] = (g >= 0).sum((0, 2))
    out[:, AC] = (g == 1).sum((0, 2))
    return out


def np_z(counts):
    """the contract, restated variant by variant -> (z float64 [3, V], not rounded; used bool [V])"""
    z, used = np.zeros((3, len(counts))), np.zeros(len(counts), bool)
    for v, (an, ac) in enumerate(zip(counts[:, AN].tolist(), counts[:, AC].tolist())):
        if an > 0 and 0 < ac < an:
            p = np.float64(ac) / np.float64(an)
            used[v] = True
            z[:, v] = [(d - 2.0 * p) / np.sqrt(2.0 * p * (1.0 - p)) for d in (0.0, 1.0, 2.0)]
    return z, used


def np_grm_sums(g, z, take):
    """int8 [n, V, 2], z float64 [3, V], take bool [V] -> (S, T, N): float64 sums of x_i x_j and of |x_i x_j|, int64 number
    of taken variants at which both calls are complete; x = z[dosage] of a complete call (both alleles 0 or 1) at a taken
    variant, else 0"""
    a, b = g[..., 0].astype(np.int64), g[..., 1].astype(np.int64)
    m = (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1) & take[None, :]
    x = np.where(m, z[np.where(m, a + b, 0), np.arange(g.shape[1])[None, :]], 0.0)
    mi = m.astype(np.int64)
    return x @ x.T, np.abs(x) @ np.abs(x).T, mi @ mi.T


def random_genotypes(rng, S, V):
    """every frequency from rare to common, 3 % missing alleles (so whole and half-missing calls), 1 % allele 2, then a
    monomorphic variant of each kind and one nobody is called at"""
    p = rng.random(V) * 0.9 + 0.02
    g = (rng.random((S, V, 2)) < p[None, :, None]).astype(np.int8)
    g[rng.random((S, V, 2)) < 0.03] = -9
    g[rng.random((S, V, 2)) < 0.01] = 2
    g[:, 0], g[:, 1], g[:, 2] = 0, 1, -9
    g[3, 1, 0] = -9
    return g


def test_numpy_and_torch_give_the_same_bits():
    rng = np.random.default_rng(1)
    c = np_counts(random_genotypes(rng, 40, 300)).astype(np.int32)
    z, used = standardized_dosages(c)
    zt, ut = standardized_dosages(torch.from_numpy(c))
    assert z.dtype == np.float32 and z.shape == (3, 300) and used.dtype == bool and used.shape == (300,)
    assert zt.dtype == torch.float32 and ut.dtype == torch.bool
    assert np.array_equal(z.view(np.uint32), zt.numpy().view(np.uint32)) and np.array_equal(used, ut.numpy())
    S = rng.standard_normal((7, 7)) * 1000
    N = rng.integers(0, 3, (7, 7)).astype(np.int32) * 500
    assert (N == 0).any()
    a, b = grm_from_sums(S, N), grm_from_sums(torch.from_numpy(S), torch.from_numpy(N))
    assert a.dtype == np.float64 and b.dtype == torch.float64
    assert np.array_equal(np.isnan(a), N == 0) and np.array_equal(a.view(np.uint64), b.numpy().view(np.uint64))


def test_against_direct_restatement():
    rng = np.random.default_rng(2)
    g = random_genotypes(rng, 40, 300)
    counts = np_counts(g)
    z, used = standardized_dosages(counts)
    want, want_used = np_z(counts)
    assert np.array_equal(used, want_used) and not used[:3].any() and used.sum() > 250
    assert not z[:, ~used].any() and not np.signbit(z[:, ~used]).any()
    assert np.array_equal(z, want.astype(np.float32))                    # float64, rounded once
    assert (z[0, used] < 0).all() and (z[2, used] > 0).all()
    # the matrix, pair by pair, from z as rounded (both sides float64)
    z64 = z.astype(np.float64)
    S, _, N = np_grm_sums(g, z64, used)
    got = grm_from_sums(S, N)
    for i in range(0, 40, 7):
        for j in range(40):
            tot, n = 0.0, 0
            for v in np.nonzero(used)[0]:
                ci, cj = g[i, v], g[j, v]
                if set(ci.tolist()) <= {0, 1} and set(cj.tolist()) <= {0, 1}:
                    tot += z64[int(ci.sum()), v] * z64[int(cj.sum()), v]
                    n += 1
            assert n == N[i, j] and n > 0
            assert abs(got[i, j] - tot / n) <= 1e-12 * abs(tot / n), (i, j)
    assert np.array_equal(got, got.T)


def test_row_sums_vanish_on_complete_data():
    rng = np.random.default_rng(3)
    p = rng.random(300) * 0.9 + 0.05
    g = (rng.random((40, 300, 2)) < p[None, :, None]).astype(np.int8)
    z, used = standardized_dosages(np_counts(g))
    S, T, N = np_grm_sums(g, z.astype(np.float64), used)
    assert (N == used.sum()).all()
    assert (np.abs(S.sum(1)) <= S_BOUND * T.sum(1)).all()
    assert np.abs(S).max() > 100 * np.abs(S.sum(1)).max()               # (the entries themselves are not small)


def test_top_eigenpairs():
    rng = np.random.default_rng(4)
    a = rng.standard_normal((12, 30))
    g = a @ a.T / 30
    w, v = np.linalg.eigh(g)
    vals, vecs = top_eigenpairs(g, 5)
    assert vals.dtype == np.float64 and vecs.shape == (12, 5)
    assert np.array_equal(vals, w[::-1][:5])
    for c in range(5):
        col = v[:, 11 - c]
        lead = int(np.argmax(np.abs(col)))
        assert np.array_equal(vecs[:, c], col if col[lead] > 0 else -col) and vecs[lead, c] > 0
    assert np.abs(vecs.T @ vecs - np.eye(5)).max() < 1e-12
    # a tie in magnitude: the first such component decides
    _, t = top_eigenpairs(np.array([[2.0, -1.0], [-1.0, 2.0]]), 1)
    assert t[0, 0] > 0 and t[1, 0] < 0
    assert top_eigenpairs(g, 12)[1].shape == (12, 12)
    for k in (0, 13, -1):
        with pytest.raises(ValueError):
            top_eigenpairs(g, k)
    g[2, 5] = g[5, 2] = np.nan
    with pytest.raises(ValueError, match="1 pair"):
        top_eigenpairs(g, 3)


def header_prototype(name):
    src = open(os.path.join(ROOT, "include", "hhgt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    args = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src).group(1)
    return [" ".join(a.split()) for a in args.split(",")]


def test_lib_declares_hhgt_grm_as_the_header_does():
    from haplohyped_varawareml_amd import _lib, build
    build.build()
    L = _lib.load()
    args = header_prototype("hhgt_grm")
    assert args == ["hhgt_ctx *ctx", "const uint32_t *d_planes", "uint64_t n_rows", "uint64_t row_words", "uint64_t w_lo",
                    "uint64_t w_hi", "const float *d_z", "double *d_table", "void *stream"]
    want = [ctypes.c_void_p if "*" in a else {"uint64_t": ctypes.c_uint64}[a.split()[0]] for a in args]
    assert list(L.hhgt_grm.argtypes) == want
    assert header_prototype("hhgt_pair_counts")[:6] == args[:6]          # the same plane arguments as its neighbour
    src = open(os.path.join(ROOT, "include", "hhgt.h")).read()
    assert int(re.search(r"#define\s+HHGT_GRM_SPAN\s+(\d+)", src).group(1)) == GRM_SPAN == 128
    assert _lib.STAGE_NAMES[int(re.search(r"#define\s+HHGT_STAGE_GRM\s+(\d+)", src).group(1))] == "grm"
    assert int(re.search(r"#define\s+HHGT_N_STAGES\s+(\d+)", src).group(1)) == _lib.N_STAGES == len(_lib.STAGE_NAMES)
