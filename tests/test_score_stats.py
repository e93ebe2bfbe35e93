"""CPU: the formulas behind polygenic scores and the projection onto principal components (store_stats) — against plain
numpy on the genotypes, a sum of class bits standing in for hhgt_score_sums and tests.test_assoc_stats.np_sums for
hhgt_assoc_sums —, numpy against torch, the refusals, and the C declaration."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd.store import (AC, AN, SCORE_MAX_COLS, SCORE_SLICE, SCORE_SPAN, loadings_from_sums,
                                             projection_class_weights, score_class_weights, standardized_dosages,
                                             top_eigenpairs)
from tests.test_assoc_stats import np_classes, np_sums
from tests.test_grm_stats import ROOT, header_prototype, np_counts


# ---- the stand-in for the kernel: plain numpy on the genotypes -----------------------------------------------------------------
def np_score_sums(G, Wd):
    """genotypes int8 [n, V, 2], class weights float64 [3, V, K] -> float64 [n, K]: per sample, the sum over its complete
    calls of the weight of the call's dosage class (0 HOM_REF, 1 HET, 2 HOM_ALT) — what hhgt_score_sums adds"""
    het, ok, alt = (c.T.astype(np.float64) for c in np_classes(G))
    return (ok - het - alt) @ Wd[0] + het @ Wd[1] + alt @ Wd[2]


def np_dense_score(G, beta, counts, impute):
    """the contract by another route: the dosage matrix, a call that is not complete replaced by 2p (mean) or 0 (none), a
    variant without a called allele among the frequency samples left out (mean), times beta"""
    het, ok, alt = (c.T for c in np_classes(G))
    dosage = het + 2.0 * alt
    if impute == "none":
        return np.where(ok, dosage, 0.0) @ beta
    an, ac = counts[:, AN].astype(np.float64), counts[:, AC].astype(np.float64)
    used = an > 0
    two_p = np.where(used, 2.0 * ac / np.maximum(an, 1.0), 0.0)
    return (np.where(ok, dosage, two_p[None, :]) * used[None, :]) @ beta


def quarter_cohort(seed=0, n=8, V=300, K=3):
    """eight samples; at a variant all eight or four of them are called (the others miss both alleles: AN = 16 or 8) and
    carry AC in {0, AN/4, AN/2, 3AN/4, AN} ALT alleles, so p = AC / AN is in quarters; betas in quarters; variant 1
    nobody is called at"""
    rng = np.random.default_rng(seed)
    G = np.zeros((n, V, 2), np.int8)
    for v in range(V):
        called = 8 if v % 3 else 4                              # AN = 16 or 8
        alt_alleles = int(rng.integers(0, 5)) * called // 2     # AC = 0, AN/4, AN/2, 3AN/4, AN
        alleles = np.zeros(2 * called, np.int8)
        alleles[:alt_alleles] = 1
        rows = rng.permutation(n)
        G[rows[:called], v] = rng.permutation(alleles).reshape(called, 2)
        G[rows[called:], v] = -9
    G[:, 1] = -9
    beta = rng.integers(-8, 9, (V, K)) / 4.0
    return G, beta


@pytest.mark.parametrize("impute", ["mean", "none"])
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_score_class_weights_are_exact_on_quarters(impute, kind):
    G, beta = quarter_cohort()
    counts = np_counts(G)
    p = counts[:, AC] / np.maximum(counts[:, AN], 1)
    assert set(np.unique(p * 4) % 1) == {0.0} and len(np.unique(p)) == 5 and counts[1, AN] == 0
    if kind == "torch":
        Wd, offset, used = (x.numpy() for x in score_class_weights(torch.from_numpy(beta), torch.from_numpy(counts), impute))
    else:
        Wd, offset, used = score_class_weights(beta, counts, impute)
    assert Wd.dtype == np.float64 and Wd.shape == (3,) + beta.shape and offset.shape == (beta.shape[1],) and used.dtype == bool
    want = np_dense_score(G, beta, counts, impute)
    assert np.array_equal(offset[None, :] + np_score_sums(G, Wd), want) and np.abs(want).max() > 10
    # a variant nobody is called at: not used with "mean" (zeros, nothing in the offset), used with "none"
    assert bool(used[1]) == (impute == "none") and np.array_equal(used, counts[:, AN] > 0 if impute == "mean" else np.ones(len(p), bool))
    if impute == "mean":
        assert not Wd[:, 1].any() and np.array_equal(offset, (2.0 * p[:, None] * beta * used[:, None]).sum(0))
    else:
        assert not offset.any() and np.array_equal(Wd[2], 2.0 * beta) and not Wd[0].any()
    # a frequency from other samples: the offsets move, the identity holds (to rounding: p is no longer in quarters)
    other = np_counts(G[:5])
    Wd, offset, used = score_class_weights(beta, other, impute)
    want = np_dense_score(G, beta, other, impute)
    assert np.abs(offset[None, :] + np_score_sums(G, Wd) - want).max() <= 300 * 2.0 ** -50 * np.abs(beta).sum(0).max()
    # beta [V] is beta [V, 1]
    one = score_class_weights(beta[:, 0], counts, impute)
    assert one[0].shape == (3, len(p), 1) and np.array_equal(one[0][..., 0], score_class_weights(beta, counts, impute)[0][..., 0])


def complete_cohort(seed=3, n=48, V=700):
    """two populations without an incomplete call; variant 0 monomorphic"""
    rng = np.random.default_rng(seed)
    pop = np.arange(n) % 2
    base = rng.random(V) * 0.6 + 0.2
    freq = np.stack([base, np.clip(base + rng.uniform(-0.3, 0.3, V), 0.02, 0.98)])
    G = (rng.random((n, V, 2)) < freq[pop][:, :, None]).astype(np.int8)
    G[:, 0] = 0
    return G


def np_grm(G, z, used):
    """the float64 relationship matrix of complete data: X X^T / (variants used), X the standardised dosages"""
    dosage = G.sum(2)
    X = np.where(used[None, :], z[dosage, np.arange(G.shape[1])[None, :]], 0.0)
    return X @ X.T / used.sum(), X


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_projection_of_the_fitted_samples_reproduces_eigh(kind):
    """without incomplete calls the relationship matrix is X X^T / M, so X (X^T U / (M values)) = U: a pure-numpy identity"""
    G, k = complete_cohort(), 4
    counts = np_counts(G)
    z, used = standardized_dosages(counts)
    assert z.dtype == np.float32 and not used[0] and used[1:].all()
    grm, _ = np_grm(G, z.astype(np.float64), used)
    values, vectors = top_eigenpairs(grm, k)
    T = np_sums(G, vectors)                                   # [V, 3, k]: hhgt_assoc_sums' sums of the eigenvectors
    if kind == "torch":
        L = loadings_from_sums(torch.from_numpy(T), torch.from_numpy(z), torch.from_numpy(values), int(used.sum()))
        Wd = projection_class_weights(torch.from_numpy(z), L).numpy()
        L = L.numpy()
    else:
        L = loadings_from_sums(T, z, values, int(used.sum()))
        Wd = projection_class_weights(z, L)
    assert L.dtype == np.float64 and L.shape == (G.shape[1], k) and Wd.shape == (3, G.shape[1], k) and not Wd[:, 0].any()
    err = np.abs(np_score_sums(G, Wd) - vectors).max()
    print(f"projection of the fitted samples against eigh's vectors ({kind}): largest difference {err:.3g}")
    assert err <= 1e-9
    # the other kind gives the same loadings
    other = (loadings_from_sums(T, z, values, int(used.sum())) if kind == "torch" else
             loadings_from_sums(torch.from_numpy(T), torch.from_numpy(z), values, int(used.sum())).numpy())
    assert np.abs(other - L).max() <= 1e-15 * np.abs(L).max()


def test_refusals():
    G, beta = quarter_cohort()
    counts = np_counts(G)
    for bad in (dict(beta=beta[:-1]), dict(beta=beta[None]), dict(counts=counts[:, :3]), dict(impute="median"),
                dict(beta=torch.from_numpy(beta))):
        with pytest.raises(ValueError):
            score_class_weights(**{**dict(beta=beta, counts=counts, impute="mean"), **bad})
    T, z = np.zeros((5, 3, 2)), np.zeros((3, 5), np.float32)
    assert loadings_from_sums(T, z, [2.0, 1.0], 5).shape == (5, 2)
    for values in ([2.0, 0.0], [2.0, -1e-3], [float("nan"), 1.0]):
        with pytest.raises(ValueError, match="eigenvalue"):
            loadings_from_sums(T, z, values, 5)
    for bad in (dict(T=T[:, :2]), dict(z=z[:, :4]), dict(z=z[:2]), dict(values=[1.0]), dict(n_variants=0)):
        with pytest.raises(ValueError):
            loadings_from_sums(**{**dict(T=T, z=z, values=[2.0, 1.0], n_variants=5), **bad})
    for bad in ((z[:2], np.zeros((5, 2))), (z, np.zeros((4, 2))), (z, np.zeros(5))):
        with pytest.raises(ValueError):
            projection_class_weights(*bad)


def test_lib_declares_hhgt_score_sums_as_the_header_does():
    from haplohyped_varawareml_amd import _lib, build
    build.build()
    L = _lib.load()
    args = header_prototype("hhgt_score_sums")
    assert args == ["hhgt_ctx *ctx", "const uint32_t *d_planes", "uint64_t n_rows", "uint64_t row_words", "uint64_t w_lo",
                    "uint64_t w_hi", "const double *d_w", "uint32_t n_cols", "double *d_sums", "void *stream"]
    want = [ctypes.c_void_p if "*" in a else {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}[a.split()[0]]
            for a in args]
    assert list(L.hhgt_score_sums.argtypes) == want and L.hhgt_score_sums.restype == ctypes.c_int
    assert "score.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "include", "hhgt.h")).read()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1))                    # noqa: E731
    assert define("HHGT_N_STAGES") == _lib.N_STAGES == len(_lib.STAGE_NAMES) == 16          # no stage of its own
    assert define("HHGT_SCORE_SLICE") == SCORE_SLICE and define("HHGT_SCORE_SPAN") == SCORE_SPAN and SCORE_MAX_COLS == 64
