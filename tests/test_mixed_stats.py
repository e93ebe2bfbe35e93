"""The mixed-model scan's host side (store_stats): the null model against a brute-force dense likelihood, the statistics
from the sums and quadratic forms against an independent whitened least-squares fit, the coefficients, leave-one-group-out
sums, and the C declaration.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd.store import (MIXED_BETA, MIXED_P, MIXED_SE, MIXED_Z, loco_sums, mixed_coefficients,
                                             mixed_from_forms, mixed_null, mixed_reference, normal_two_sided)
from tests.test_assoc_stats import np_classes, np_sums, rel_diff
from tests.test_grm_stats import ROOT, header_prototype

# relative tolerance of BETA, SE, Z (and P) against the whitened lstsq reference: 1000 x the largest relative difference
# measured on the CPU over the cases of test_statistics_match_whitened_lstsq, 1.86e-12 (numpy sums; the four cases
# (n, q0) = (200, 0), (200, 3), (500, 0), (500, 3) give 1.58e-12, 1.86e-12, 1.52e-13, 1.99e-13).  The device differs from these numpy sums in
# summation order only, which hhgt_assoc_sums and hhgt_quad_forms bound.
MIXED_RTOL = 1.86e-9


# ---- a cohort with relatedness: families of siblings, so that K has structure and h2 lies inside (0, 1) -----------------------
def cohort(seed, n, q0, V=120, missing=0.05, h2=0.5):
    """-> (G int8 [n, V, 2], K [n, n] from 2000 other variants, y [n], cov [n, q0] or None): variant 0 monomorphic, variant 1
    all missing, and with covariates the last one is the dosage of variant 2 (which has no missing allele)"""
    rng = np.random.default_rng(seed)
    fam = np.arange(n) // 4

    def draw(m):
        f = rng.uniform(0.1, 0.9, m)
        parents = rng.random((fam.max() + 1, 2, m, 2)) < f[None, None, :, None]           # two parents per family
        pick = rng.integers(0, 2, (n, 2, m))
        pat = np.take_along_axis(parents[fam, 0], pick[:, 0, :, None], axis=2)[..., 0]
        mat = np.take_along_axis(parents[fam, 1], pick[:, 1, :, None], axis=2)[..., 0]
        return np.stack([pat, mat], axis=2).astype(np.int8), f
    Gk, f = draw(2000)
    Z = (Gk.sum(2) - 2.0 * f) / np.sqrt(2.0 * f * (1.0 - f))
    K = Z @ Z.T / Z.shape[1]
    G, _ = draw(V)
    G[rng.random((n, V, 2)) < missing] = -9
    G[:, 0], G[:, 1] = 0, -9
    G[:, 2] = np.where(G[:, 2] < 0, 0, G[:, 2])
    cov = rng.normal(size=(n, q0)) if q0 else None
    if q0:
        cov[:, -1] = G[:, 2].sum(1)
    u = np.linalg.cholesky(K + 1e-6 * np.eye(n)) @ rng.normal(size=n)
    y = math.sqrt(h2) * u + math.sqrt(1.0 - h2) * rng.normal(size=n) + 0.3 * G[:, 5].clip(0).sum(1) + (cov[:, 0] if q0 else 0.0)
    return G, K, y, cov


def design(n, cov):
    return np.ones((n, 1)) if cov is None else np.concatenate([np.ones((n, 1)), cov], axis=1)


def np_forms(G, null):
    """numpy sums T [V, 3, 2] of W = [1 | My] and q = x^T M x with x from mixed_coefficients(T)"""
    T = np_sums(G, np.stack([np.ones(G.shape[0]), null["My"]], axis=1))
    het, ok, alt = (c.T.astype(np.float64) for c in np_classes(G))
    coef = mixed_coefficients(T)
    x = coef[None, :, 0] * het + coef[None, :, 1] * ok + coef[None, :, 2] * alt
    return T, ((null["M"] @ x) * x).sum(0)


def whitened_lstsq_scan(G, K, y, cov, null, dependent=()):
    """the contract by another route: V = sigma2 (h2 K + (1 - h2) I) from the null's two numbers, L its Cholesky factor, and
    per variant numpy.linalg.lstsq of L^-1 y on L^-1 [X | g], g the mean-imputed dosage -> stats [V, 4]: the coefficient
    of g, sqrt of the last diagonal entry of (A^T A)^-1, their ratio, normal_two_sided of it"""
    het, ok, alt = np_classes(G)
    n, nv = G.shape[0], G.shape[1]
    L = np.linalg.cholesky(null["sigma2"] * (null["h2"] * K + (1.0 - null["h2"]) * np.eye(n)))
    X0, yw = design(n, cov), np.linalg.solve(L, y)
    stats = np.full((nv, 4), np.nan)
    for v in range(nv):
        m, h, a = int(ok[v].sum()), int(het[v].sum()), int(alt[v].sum())
        if m == 0 or (m - h - a > 0) + (h > 0) + (a > 0) < 2 or v in dependent:
            continue
        g = np.where(ok[v], het[v] + 2.0 * alt[v], (h + 2.0 * a) / m)
        A = np.linalg.solve(L, np.concatenate([X0, g[:, None]], axis=1))
        coef, _, rank, _ = np.linalg.lstsq(A, yw, rcond=None)
        assert rank == A.shape[1]
        se = math.sqrt(np.linalg.inv(A.T @ A)[-1, -1])
        stats[v, MIXED_BETA], stats[v, MIXED_SE], stats[v, MIXED_Z] = coef[-1], se, coef[-1] / se
    stats[:, MIXED_P] = normal_two_sided(stats[:, MIXED_Z])
    return stats


# ---- mixed_null -----------------------------------------------------------------------------------------------------------------
def brute_force(K, y, X, h2):
    """the REML log-likelihood profiled over sigma2, dense: explicit inverse and slogdet -> (value, sigma2)"""
    n, q = X.shape
    Vi = np.linalg.inv(h2 * K + (1.0 - h2) * np.eye(n))
    XVX = X.T @ Vi @ X
    P = Vi - Vi @ X @ np.linalg.solve(XVX, X.T @ Vi)
    s2 = float(y @ P @ y) / (n - q)
    return -0.5 * ((n - q) * math.log(s2) - np.linalg.slogdet(Vi)[1] + np.linalg.slogdet(XVX)[1]), s2


@pytest.mark.parametrize("seed, q0, h2", [(1, 0, 0.5), (2, 3, 0.7), (3, 1, 0.0)])
def test_null_model_is_the_brute_force_optimum(seed, q0, h2):
    G, K, y, cov = cohort(seed, 120, q0, h2=h2)
    null = mixed_null(K, y, cov)
    X = design(len(y), cov)
    values = [brute_force(K, y, X, k / 1000.0)[0] for k in range(991)]
    best = int(np.argmax(values)) / 1000.0
    print(f"h2 = {null['h2']:.6f} (brute force on k / 1000: {best}), sigma2 = {null['sigma2']:.6f}")
    assert abs(null["h2"] - best) <= 1e-3 + 1e-12 and 0.0 <= null["h2"] <= 0.99 and null["q"] == 1 + q0
    assert null["sigma2"] == pytest.approx(brute_force(K, y, X, null["h2"])[1], rel=1e-9)
    M = null["M"]
    assert np.array_equal(M, M.T)
    assert np.abs(M @ X).max() <= 1e-9 * np.abs(M).max()
    assert np.array_equal(null["My"], M @ y)
    again = mixed_null(torch.from_numpy(K), torch.from_numpy(y), None if cov is None else torch.from_numpy(cov))
    assert again["h2"] == null["h2"] and again["sigma2"] == null["sigma2"] and np.array_equal(again["M"], M)


def test_null_model_of_the_identity_is_ordinary_least_squares():
    rng = np.random.default_rng(4)
    n, q0 = 90, 2
    cov, y = rng.normal(size=(n, q0)), rng.normal(size=n)
    null = mixed_null(np.eye(n), y, cov)
    X = design(n, cov)
    Q = np.linalg.qr(X)[0]
    res = y - Q @ (Q.T @ y)
    assert null["sigma2"] == pytest.approx(float(res @ res) / (n - 1 - q0), rel=1e-12)
    assert np.abs(null["M"] - (np.eye(n) - Q @ Q.T) / null["sigma2"]).max() <= 1e-12 / null["sigma2"]


def test_null_model_refuses():
    rng = np.random.default_rng(5)
    n = 30
    K, y = np.eye(n), rng.normal(size=n)
    for bad in (K[:-1], K[:, :-1], np.eye(n + 1), np.where(np.eye(n) > 0, 1.0, np.nan), K + np.triu(np.full((n, n), 1e-6), 1)):
        with pytest.raises(ValueError, match="mixed_null"):
            mixed_null(bad, y)
    Kinf = K.copy()
    Kinf[2, 3] = Kinf[3, 2] = np.inf
    with pytest.raises(ValueError, match="finite"):
        mixed_null(Kinf, y)
    with pytest.raises(ValueError):
        mixed_null(K, np.stack([y, y], axis=1))
    with pytest.raises(ValueError, match="finite"):
        mixed_null(K, np.where(np.arange(n) == 3, np.nan, y))
    with pytest.raises(ValueError, match="rank"):
        mixed_null(K, y, np.ones((n, 1)))
    with pytest.raises(ValueError):
        mixed_null(K, y, rng.normal(size=(n - 1, 2)))
    with pytest.raises(ValueError, match="freedom"):
        mixed_null(np.eye(4), y[:4], rng.normal(size=(4, 2)))


# ---- mixed_from_forms -----------------------------------------------------------------------------------------------------------
CASES = [(200, 0), (200, 3), (500, 0), (500, 3)]


@pytest.mark.parametrize("n, q0", CASES)
def test_statistics_match_whitened_lstsq(n, q0):
    G, K, y, cov = cohort(10 * n + q0, n, q0)
    null = mixed_null(K, y, cov)
    T, q = np_forms(G, null)
    stats, calls = mixed_from_forms(T, q, np.trace(null["M"]) / n)
    want = whitened_lstsq_scan(G, K, y, cov, null, dependent=(2,) if q0 else ())
    assert stats.shape == (G.shape[1], 4) and stats.dtype == np.float64
    d = rel_diff(stats, want)
    print(f"mixed statistics, n = {n}, q0 = {q0}: largest relative difference {d:.3g}, h2 = {null['h2']:.4f}")
    assert d <= MIXED_RTOL
    # not tested: the monomorphic variant, the one without a call, and with covariates the one inside their span
    assert np.isnan(stats[0]).all() and np.isnan(stats[1]).all() and np.isnan(stats[2]).all() == bool(q0)
    assert int(np.isnan(stats[:, 0]).sum()) == (3 if q0 else 2)
    het, ok, alt = np_classes(G)
    assert calls.dtype == np.int64 and np.array_equal(calls, np.stack([ok.sum(1), het.sum(1), alt.sum(1)], axis=1))
    # the dense reference says the same, and torch answers in kind
    ref = mixed_reference(het.T + 2 * alt.T, ok.T, null["M"], y)
    assert np.array_equal(ref["calls"], calls) and rel_diff(ref["stats"], want) <= MIXED_RTOL
    tested = ~np.isnan(stats[:, MIXED_BETA])
    assert np.abs(ref["q"] - q).max() <= 1e-12 * np.abs(q).max()
    assert np.allclose(ref["U"][tested], (stats[:, MIXED_BETA] * q)[tested], rtol=1e-9, atol=0.0)
    ts, tc = mixed_from_forms(torch.from_numpy(T), torch.from_numpy(q), np.trace(null["M"]) / n)
    assert ts.dtype == torch.float64 and tc.dtype == torch.int64 and np.array_equal(tc.numpy(), calls)
    assert rel_diff(ts.numpy(), stats) <= 1e-12
    assert np.array_equal(mixed_coefficients(torch.from_numpy(T)).numpy(), mixed_coefficients(T))


def test_coefficients():
    T = np.zeros((3, 3, 2))
    T[0, :, 0] = (2, 8, 1)                       # 2 HET, 8 complete, 1 HOM_ALT: mean 1/2
    T[2, :, 0] = (0, 5, 5)
    assert np.array_equal(mixed_coefficients(T), [[1.0, -0.5, 2.0], [0.0, 0.0, 0.0], [1.0, -2.0, 2.0]])
    with pytest.raises(ValueError):
        mixed_from_forms(T[:, :, :1], np.zeros(3), 1.0)
    with pytest.raises(ValueError):
        mixed_from_forms(T, np.zeros(4), 1.0)


def test_loco_sums():
    S = {g: np.full((2, 2), float(k)) for k, g in enumerate(("chr_1", "chr_2", "chr_3"), 1)}
    N = {g: np.full((2, 2), 10 * k, dtype=np.int32) for k, g in enumerate(("chr_1", "chr_2", "chr_3"), 1)}
    s, n = loco_sums(S, N, "chr_2")
    assert np.array_equal(s, np.full((2, 2), 4.0)) and np.array_equal(n, np.full((2, 2), 40)) and n.dtype == np.int32
    ts, tn = loco_sums({g: torch.from_numpy(x) for g, x in S.items()}, {g: torch.from_numpy(x) for g, x in N.items()}, "chr_1")
    assert torch.equal(ts, torch.full((2, 2), 5.0, dtype=torch.float64)) and torch.equal(tn, torch.full((2, 2), 50, dtype=torch.int32))
    with pytest.raises(ValueError, match="only group"):
        loco_sums({"chr_1": S["chr_1"]}, {"chr_1": N["chr_1"]}, "chr_1")
    with pytest.raises(ValueError):
        loco_sums(S, N, "chr_9")


# ---- the C declaration ----------------------------------------------------------------------------------------------------------
def test_lib_declares_hhgt_quad_forms_as_the_header_does():
    from haplohyped_varawareml_amd import _lib, build
    build.build()
    L = _lib.load()
    args = header_prototype("hhgt_quad_forms")
    assert args == ["hhgt_ctx *ctx", "const uint32_t *d_vplanes", "uint64_t n_var", "uint64_t sw", "const double *d_coef",
                    "const double *d_a", "double *d_q", "void *stream"]
    want = [ctypes.c_void_p if "*" in a else {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}[a.split()[0]]
            for a in args]
    assert L.hhgt_quad_forms.argtypes == want == _lib.PROTOTYPES["hhgt_quad_forms"][1]
    assert L.hhgt_quad_forms.restype == ctypes.c_int and "quad.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "include", "hhgt.h")).read()
    assert int(re.search(r"#define\s+HHGT_N_STAGES\s+(\d+)", src).group(1)) == _lib.N_STAGES == len(_lib.STAGE_NAMES) == 16
    assert int(re.search(r"#define\s+HHGT_QUAD_MAX_WORDS\s+(\d+)", src).group(1)) == 1024
    assert (MIXED_BETA, MIXED_SE, MIXED_Z, MIXED_P) == (0, 1, 2, 3)
