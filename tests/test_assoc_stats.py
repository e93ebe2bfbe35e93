"""The association scan's host side (store_stats): the design, the statistics from the sums against an independent
per-variant numpy.linalg.lstsq, the p-value's continued fraction, and the C declaration.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd.store import (ASSOC_ALT, ASSOC_BETA, ASSOC_COMPLETE, ASSOC_HET, ASSOC_P, ASSOC_SE, ASSOC_T,
                                             assoc_design, assoc_from_sums, student_t_two_sided)
from tests.test_grm_stats import ROOT, header_prototype

# relative tolerance of BETA, SE, T (and P) against the lstsq reference: 1000 x the largest relative difference measured on
# the CPU over the cases of test_statistics_match_lstsq, 1.73e-11 (numpy sums; the four cases give 1.73e-11, 3.91e-12,
# 8.64e-13, 2.81e-12).  The device differs from these numpy sums in summation order only, which hhgt_assoc_sums bounds.
STAT_RTOL = 1.73e-8


# ---- the reference: plain numpy on the genotypes ---------------------------------------------------------------------------
def np_classes(G):
    """genotypes int8 [S, V, 2] -> (het, complete, alt), bool [V, S] each, in the kernel's plane order"""
    ok = ((G == 0) | (G == 1)).all(axis=2)
    het, alt = ok & (G[..., 0] != G[..., 1]), ok & (G[..., 0] == 1) & (G[..., 1] == 1)
    return het.T, ok.T, alt.T


def np_sums(G, W):
    """-> float64 [V, 3, C]: bits @ W per plane"""
    return np.stack([c.astype(np.float64) @ W for c in np_classes(G)], axis=1)


def np_lstsq_scan(G, y, cov=None, dependent=()):
    """the contract by another route: per variant, numpy.linalg.lstsq of every phenotype on [1 | covariates | dosage], a
    call that is not complete imputed to the mean dosage of the complete ones -> (stats float64 [V, P, 4], calls int64
    [V, 3]); P from student_t_two_sided.  NaN for a variant without a complete call, with fewer than two genotype classes,
    or named in `dependent` (the caller knows its dosage is a combination of the covariates)."""
    het, ok, alt = np_classes(G)
    Y = np.asarray(y, np.float64).reshape(len(y), -1)
    n, V = G.shape[0], G.shape[1]
    X0 = np.ones((n, 1)) if cov is None else np.concatenate([np.ones((n, 1)), cov], axis=1)
    df = n - X0.shape[1] - 1
    stats = np.full((V, Y.shape[1], 4), np.nan)
    calls = np.stack([ok.sum(1), het.sum(1), alt.sum(1)], axis=1).astype(np.int64)
    for v in range(V):
        m, h, a = (int(x) for x in calls[v])
        if m == 0 or (m - h - a > 0) + (h > 0) + (a > 0) < 2 or v in dependent:
            continue
        g = np.where(ok[v], het[v] + 2.0 * alt[v], (h + 2.0 * a) / m)
        X = np.concatenate([X0, g[:, None]], axis=1)
        coef, _, rank, _ = np.linalg.lstsq(X, Y, rcond=None)
        assert rank == X.shape[1]
        res = Y - X @ coef
        se = np.sqrt((res * res).sum(0) / df * np.linalg.inv(X.T @ X)[-1, -1])
        stats[v, :, ASSOC_BETA], stats[v, :, ASSOC_SE], stats[v, :, ASSOC_T] = coef[-1], se, coef[-1] / se
    stats[..., ASSOC_P] = student_t_two_sided(stats[..., ASSOC_T], df)
    return stats, calls


def rel_diff(got, want):
    """the largest relative difference of BETA, SE, T, and of P where P > 1e-300; the NaN patterns must agree"""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    ok[..., ASSOC_P] &= np.nan_to_num(want[..., ASSOC_P]) > 1e-300
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.abs(got - want)[ok] / np.abs(want)[ok], initial=0.0))


def synthetic(seed, n=200, V=300, q0=2, P=1, missing=0.02):
    """-> (G int8 [n, V, 2], y [n, P], cov [n, q0] or None, dependent): variant 0 monomorphic, variant 1 all missing, and
    with covariates the last one is the dosage of variant 2 (which has no missing allele)"""
    rng = np.random.default_rng(seed)
    G = (rng.random((n, V, 2)) < rng.uniform(0.05, 0.95, V)[None, :, None]).astype(np.int8)
    G[rng.random((n, V, 2)) < missing] = -9
    G[:, 0], G[:, 1] = 0, -9
    G[:, 2] = (rng.random((n, 2)) < 0.4).astype(np.int8)
    cov = rng.normal(size=(n, q0)) if q0 else None
    dependent = ()
    if q0:
        cov[:, -1] = G[:, 2].sum(1)
        dependent = (2,)
    y = rng.normal(size=(n, P)) + 0.5 * G[:, 5].clip(0).sum(1)[:, None] + (cov[:, :1] if q0 else 0.0)
    return G, y, cov, dependent


# ---- assoc_design -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q0, P", [(0, 1), (3, 2), (10, 1)])
def test_design_is_orthonormal(q0, P):
    rng = np.random.default_rng(q0)
    n = 150
    y = rng.normal(size=(n, P)) * 10 + 3
    cov = rng.normal(size=(n, q0)) + 5 if q0 else None
    W, q, yy = assoc_design(y if P > 1 else y[:, 0], cov)
    assert W.dtype == np.float64 and W.shape == (n, 1 + q + P) and q == 1 + q0 and yy.shape == (P,)
    Q, Yr = W[:, 1:1 + q], W[:, 1 + q:]
    assert np.array_equal(W[:, 0], np.ones(n))
    assert np.abs(Q.T @ Q - np.eye(q)).max() < 1e-12
    assert np.abs(Q.T @ Yr).max() < 1e-12 * np.linalg.norm(y)
    assert np.allclose(yy, (Yr * Yr).sum(0), rtol=1e-15)
    # Q spans [1 | covariates]: the residual of y is that of lstsq
    X = np.ones((n, 1)) if cov is None else np.concatenate([np.ones((n, 1)), cov], axis=1)
    res = y - X @ np.linalg.lstsq(X, y, rcond=None)[0]
    assert np.abs(Yr - res).max() < 1e-10
    Wt = assoc_design(torch.from_numpy(y), None if cov is None else torch.from_numpy(cov))[0]
    assert np.array_equal(Wt, assoc_design(y, cov)[0])


def test_design_refuses():
    rng = np.random.default_rng(0)
    y, cov = rng.normal(size=20), rng.normal(size=(20, 3))
    assoc_design(y, cov)
    bad = y.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        assoc_design(bad, cov)
    bad = cov.copy()
    bad[0, 0] = np.inf
    with pytest.raises(ValueError, match="finite"):
        assoc_design(y, bad)
    with pytest.raises(ValueError, match="rows"):
        assoc_design(y, cov[:19])
    with pytest.raises(ValueError, match="rank"):
        assoc_design(y, np.concatenate([cov, cov[:, :1] * 2 - cov[:, 1:2]], axis=1))
    with pytest.raises(ValueError, match="rank"):
        assoc_design(y, np.full((20, 1), 3.0))                       # a constant column beside the intercept
    with pytest.raises(ValueError, match="degree"):
        assoc_design(y[:5], cov[:5])                                   # n - q - 1 = 5 - 4 - 1
    assoc_design(y[:6], cov[:6])
    with pytest.raises(ValueError, match="64"):
        assoc_design(rng.normal(size=(100, 3)), rng.normal(size=(100, 60)))     # 1 + 61 + 3
    assoc_design(rng.normal(size=(100, 2)), rng.normal(size=(100, 60)))


# ---- assoc_from_sums ------------------------------------------------------------------------------------------------------------
CASES = [(0, 1), (1, 2), (2, 1), (3, 2)]


@pytest.mark.parametrize("q0, P", CASES)
def test_statistics_match_lstsq(q0, P):
    G, y, cov, dependent = synthetic(10 + q0, q0=q0, P=P)
    W, q, yy = assoc_design(y, cov)
    T = np_sums(G, W)
    stats, calls = assoc_from_sums(T, W.sum(axis=0), q, yy)
    want, want_calls = np_lstsq_scan(G, y, cov, dependent)
    assert stats.dtype == np.float64 and stats.shape == (G.shape[1], P, 4) and calls.dtype == np.int64
    assert np.array_equal(calls, want_calls)
    for v in (0, 1) + tuple(dependent):                                # monomorphic, all missing, explained by the covariates
        assert np.isnan(stats[v]).all()
    assert np.isnan(stats).any(axis=(1, 2)).sum() == 2 + len(dependent)
    d = rel_diff(stats, want)
    print(f"assoc_from_sums q0={q0} P={P}: largest relative difference {d:.3g}")
    assert d <= STAT_RTOL
    assert np.nanmin(stats[..., ASSOC_P]) < 1e-3 and (np.nan_to_num(stats[..., ASSOC_SE]) >= 0).all()
    # torch answers in kind, with the same numbers
    ts, tc = assoc_from_sums(torch.from_numpy(T), torch.from_numpy(W.sum(axis=0)), q, torch.from_numpy(yy))
    assert ts.dtype == torch.float64 and tc.dtype == torch.int64 and np.array_equal(tc.numpy(), calls)
    assert rel_diff(ts.numpy(), stats) < 1e-12


# ---- student_t_two_sided ----------------------------------------------------------------------------------------------------------
T_GRID = np.array([0.0, 1e-3, 0.1, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 12.0, 20.0, 37.5])


def test_p_value_closed_forms():
    t = T_GRID
    # (the closed forms lose digits to cancellation as p gets small: compared where they are good to 1e-12)
    p1, p2 = student_t_two_sided(t, 1), student_t_two_sided(t, 2)
    assert np.abs(p1 - (1 - 2 / np.pi * np.arctan(t))).max() < 1e-14
    assert np.abs(p2 - (1 - t / np.sqrt(2 + t * t))).max() < 1e-14
    big = np.array([1e3, 1e5, 1e8])                                    # the tails, by their own series: relative accuracy
    assert np.abs(student_t_two_sided(big, 1) / (2 / np.pi * (1 / big - 1 / (3 * big ** 3))) - 1).max() < 1e-12
    assert np.abs(student_t_two_sided(big, 2) / (1 / big ** 2 - 1.5 / big ** 4) - 1).max() < 1e-9
    for df in (1, 2, 7, 2492, 1e6):
        p = student_t_two_sided(np.concatenate([-t[::-1], t]), df)
        assert p[len(t)] == 1.0 and np.array_equal(p[:len(t)], p[len(t):][::-1])       # t = 0; even in t
        assert (np.diff(p[len(t):]) < 0).all() and (p > 0).all() and (p <= 1).all()     # monotone in |t|
    assert student_t_two_sided(np.array([np.inf, -np.inf]), 5).tolist() == [0.0, 0.0]
    assert np.isnan(student_t_two_sided(np.array([np.nan]), 5)).all()
    # df = 1e6 against the normal tail: the two differ, to first order, by 2 phi(t) (t^3 + t) / (4 df) — 2.4e-5 of the
    # tail at t = 3, less below —, and the fraction itself is good to 1e-10 there
    small = np.array([0.25, 0.5, 1.0, 2.0, 3.0])
    normal = np.array([math.erfc(x / math.sqrt(2)) for x in small])
    p = student_t_two_sided(small, 1e6)
    assert np.abs(p / normal - 1).max() < 1e-4
    first = 2 * np.exp(-small ** 2 / 2) / math.sqrt(2 * math.pi) * (small ** 3 + small) / 4e6
    assert np.abs(p / (normal + first) - 1).max() < 1e-8


def test_p_value_numpy_and_torch_agree():
    for df in (1, 2, 5, 30, 197, 2492):
        a = student_t_two_sided(T_GRID.reshape(1, -1), df)
        b = student_t_two_sided(torch.from_numpy(T_GRID).reshape(1, -1), df)
        assert b.dtype == torch.float64 and tuple(b.shape) == a.shape
        assert np.abs(b.numpy() / a - 1).max() < 1e-12, df


def test_p_value_against_scipy():
    special = pytest.importorskip("scipy.special")
    t = T_GRID[2:]                                                     # (below, x = df / (df + t^2) rounds to 1 in float64)
    for df in (1, 3, 30, 197, 2492):
        want = special.betainc(df / 2, 0.5, df / (df + t * t))
        assert np.abs(student_t_two_sided(t, df) / want - 1).max() < 1e-10, df


# ---- the declaration ------------------------------------------------------------------------------------------------------------
def test_lib_declares_hhgt_assoc_sums_as_the_header_does():
    from haplohyped_varawareml_amd import _lib, build
    build.build()
    L = _lib.load()
    args = header_prototype("hhgt_assoc_sums")
    assert args == ["hhgt_ctx *ctx", "const uint32_t *d_vplanes", "uint64_t n_var", "uint64_t sw", "const double *d_w",
                    "uint32_t n_cols", "double *d_sums", "void *stream"]
    want = [ctypes.c_void_p if "*" in a else {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}[a.split()[0]]
            for a in args]
    assert list(L.hhgt_assoc_sums.argtypes) == want and L.hhgt_assoc_sums.restype == ctypes.c_int
    src = open(os.path.join(ROOT, "include", "hhgt.h")).read()
    stage = int(re.search(r"#define\s+HHGT_STAGE_ASSOC\s+(\d+)", src).group(1))
    assert stage == 15 and _lib.STAGE_NAMES[stage] == "assoc"
    assert int(re.search(r"#define\s+HHGT_N_STAGES\s+(\d+)", src).group(1)) == _lib.N_STAGES == len(_lib.STAGE_NAMES) == 16
    assert (ASSOC_HET, ASSOC_COMPLETE, ASSOC_ALT) == (0, 1, 2) and (ASSOC_BETA, ASSOC_SE, ASSOC_T, ASSOC_P) == (0, 1, 2, 3)
