"""The case / control scan's host side (store_stats): the design and its null fit, the numpy reference of the per-variant
Newton iteration against the same model fitted in numpy.longdouble, the statistics and status codes read from the records, the
normal tail, the score test from sums, and the C declaration.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd.store import (LOGIT_BETA, LOGIT_COLLINEAR, LOGIT_MAX_COLS, LOGIT_NO_CALL, LOGIT_NOT_CONVERGED,
                                             LOGIT_ONE_CLASS, LOGIT_P, LOGIT_REC, LOGIT_SCORE_CHI2, LOGIT_SCORE_P, LOGIT_SE,
                                             LOGIT_TESTED, LOGIT_Z, REC_ALT, REC_COMPLETE, REC_GAMMA, REC_HET, REC_HINV,
                                             REC_HINV0, REC_STATUS, REC_STEPS, REC_U0, logistic_design, logistic_fit_reference,
                                             logistic_from_fit, logistic_score_design, logistic_score_from_sums,
                                             normal_two_sided)
from tests.test_assoc_stats import np_sums, synthetic
from tests.test_grm_stats import ROOT, header_prototype

# Relative tolerance of LOGIT_BETA and LOGIT_SE on the device against logistic_fit_reference: 1000 x the largest difference
# between that reference (float64) and the same model fitted in numpy.longdouble, measured on the CPU over the cases of
# test_reference_matches_longdouble, 3.62e-13 (the four cases give 6.56e-14, 3.62e-13, 1.22e-13, 1.32e-13) — the margin that
# separates test_assoc_stats.STAT_RTOL from its measurement.  The device differs from the reference in the order of its sums,
# its fused multiply-adds and its exp, the same kinds of rounding that separate float64 from longdouble here.  A value below
# 1e-3 in magnitude is compared as if it were 1e-3 (wald_diff).
LOGIT_RTOL = 3.62e-10
# the same for LOGIT_SCORE_CHI2, a value below 1e-3 compared as if it were 1e-3 (score_diff): measured 7.15e-14 (6.58e-14,
# 7.15e-14, 4.02e-14, 3.12e-14)
SCORE_RTOL = 7.15e-11

# (n, q0, seed) of synthetic(): seed 20 is one at which the reference leaves no variant unconverged among those the classing rule
# admits, in all four cases — picked on the CPU from the reference alone
CASES = [(200, 2, 20), (200, 0, 20), (96, 1, 20), (200, 10, 20)]


# ---- the inputs ------------------------------------------------------------------------------------------------------------
def dosages(G):
    """genotypes int8 [S, V, 2] -> float64 [V, S]: 0, 1, 2 for a complete call, NaN for one that is not"""
    ok = ((G == 0) | (G == 1)).all(axis=2)
    return np.where(ok, G.clip(0).sum(axis=2), np.nan).T.astype(np.float64)


def case_control(n, q0, seed):
    """-> (G, y, cov, dependent): synthetic(seed, n, 300, q0)'s genotypes and covariates, and a phenotype drawn as
    Bernoulli(sigma(0.5 x the dosage of variant 5 + the first covariate - 0.5))"""
    G, _, cov, dependent = synthetic(seed, n=n, V=300, q0=q0)
    rng = np.random.default_rng(1000 + seed)
    eta = 0.5 * G[:, 5].clip(0).sum(1) + (cov[:, 0] if q0 else 0.0) - 0.5
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    return G, y, cov, dependent


def wald_diff(got, want):
    """the largest difference of LOGIT_BETA and LOGIT_SE relative to max(|want|, 1e-3), over the variants `want` tests"""
    ok = ~np.isnan(want[:, LOGIT_BETA])
    d = np.abs(got - want)[ok][:, [LOGIT_BETA, LOGIT_SE]] / np.maximum(np.abs(want[ok][:, [LOGIT_BETA, LOGIT_SE]]), 1e-3)
    return float(d.max(initial=0.0))


def score_diff(got, want):
    """the largest difference of LOGIT_SCORE_CHI2 relative to max(want, 1e-3) — a chi^2 near 0 is the square of a sum that
    cancels —, over the variants `want` tests"""
    ok = ~np.isnan(want[:, LOGIT_SCORE_CHI2])
    d = np.abs(got - want)[ok, LOGIT_SCORE_CHI2] / np.maximum(want[ok, LOGIT_SCORE_CHI2], 1e-3)
    return float(d.max(initial=0.0))


# ---- the independent route: numpy.longdouble, a Cholesky written out, two steps past convergence ------------------------------
def ld_cholesky_solve(H, U):
    """longdouble H [p, p], U [p] -> (H^-1 U, (H^-1)[-1, -1])"""
    p = len(U)
    L = np.zeros((p, p), dtype=np.longdouble)
    for i in range(p):
        for j in range(i + 1):
            s = H[i, j] - (L[i, :j] * L[j, :j]).sum()
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    z = np.zeros(p, dtype=np.longdouble)
    for i in range(p):
        z[i] = (U[i] - (L[i, :i] * z[:i]).sum()) / L[i, i]
    d = np.zeros(p, dtype=np.longdouble)
    for i in range(p - 1, -1, -1):
        d[i] = (z[i] - (L[i + 1:, i] * d[i + 1:]).sum()) / L[i, i]
    return d, 1 / (L[-1, -1] * L[-1, -1])


def ld_evaluate(Xt, y, theta):
    mu = 1 / (1 + np.exp(-(Xt @ theta)))
    return Xt.T @ (y - mu), Xt.T @ ((mu * (1 - mu))[:, None] * Xt)


def longdouble_fit(g, X, y, beta0):
    """one variant's fit in longdouble from the same start -> (beta, se, chi2) as float64: Newton until max |delta| <= 1e-8,
    two steps more, then the evaluation that gives the standard error"""
    ld = np.longdouble
    Xt = np.concatenate([X, g[:, None]], axis=1).astype(ld)
    y = y.astype(ld)
    theta = np.concatenate([beta0, [0.0]]).astype(ld)
    U, H = ld_evaluate(Xt, y, theta)
    delta, hinv = ld_cholesky_solve(H, U)
    chi2 = U[-1] * U[-1] * hinv
    extra = 0
    for _ in range(40):
        theta = theta + delta
        extra += extra > 0 or np.abs(delta).max() <= 1e-8
        U, H = ld_evaluate(Xt, y, theta)
        delta, hinv = ld_cholesky_solve(H, U)
        if extra == 3:
            return float(theta[-1]), float(np.sqrt(hinv)), float(chi2)
    raise AssertionError("the longdouble fit did not converge")


def longdouble_scan(G, X, y, beta0, skip=()):
    """-> float64 [V, 6] in logistic_from_fit's columns (Z, P and SCORE_P by its formulas), NaN for the variants the classing
    rule leaves out and those in `skip`"""
    D = dosages(G)
    out = np.full((len(D), 6), np.nan)
    for v, d in enumerate(D):
        comp = ~np.isnan(d)
        m, h, a = int(comp.sum()), int((d == 1).sum()), int((d == 2).sum())
        if m == 0 or int(m - h - a > 0) + int(h > 0) + int(a > 0) < 2 or v in skip:
            continue
        beta, se, chi2 = longdouble_fit(np.where(comp, d, (h + 2.0 * a) / max(m, 1)), X, y, beta0)
        out[v] = beta, se, beta / se, math.erfc(abs(beta / se) / math.sqrt(2)), chi2, math.erfc(math.sqrt(chi2 / 2))
    return out


# ---- logistic_design ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q0", [0, 3, 13])
def test_design_is_orthonormal_and_null_fit_is_the_optimum(q0):
    rng = np.random.default_rng(q0)
    n = 150
    cov = rng.normal(size=(n, q0)) * 50 + 7 if q0 else None
    y = (rng.random(n) < 0.3).astype(np.float64)
    X, beta0 = logistic_design(y, cov)
    q = 1 + q0
    assert X.dtype == np.float64 and X.shape == (n, q) and beta0.shape == (q,)
    assert np.abs(X.T @ X - n * np.eye(q)).max() < 1e-10 * n
    # X spans [1 | covariates]
    A = np.ones((n, 1)) if cov is None else np.concatenate([np.ones((n, 1)), cov], axis=1)
    assert np.abs(A - X @ np.linalg.lstsq(X, A, rcond=None)[0]).max() < 1e-9 * np.abs(A).max()
    # brute force: gradient ascent polished by Newton in longdouble from 0 reaches the same coefficients
    theta = np.zeros(q, dtype=np.longdouble)
    for _ in range(60):
        U, H = ld_evaluate(X.astype(np.longdouble), y.astype(np.longdouble), theta)
        theta = theta + ld_cholesky_solve(H, U)[0]
    assert np.abs(ld_evaluate(X.astype(np.longdouble), y.astype(np.longdouble), theta)[0]).max() < 1e-15 * n
    assert np.abs(beta0 - theta.astype(np.float64)).max() < 1e-12
    Xt, bt = logistic_design(torch.from_numpy(y), None if cov is None else torch.from_numpy(cov))
    assert np.array_equal(Xt, X) and np.array_equal(bt, beta0)


def test_design_refuses():
    rng = np.random.default_rng(0)
    y, cov = (rng.random(40) < 0.5).astype(np.float64), rng.normal(size=(40, 3))
    logistic_design(y, cov)
    for bad in (np.where(np.arange(40) == 3, 2.0, y), np.where(np.arange(40) == 3, 0.5, y), y + 1):
        with pytest.raises(ValueError, match="neither 0 nor 1"):
            logistic_design(bad, cov)
    with pytest.raises(ValueError, match="finite"):
        logistic_design(np.where(np.arange(40) == 3, np.nan, y), cov)
    with pytest.raises(ValueError, match="one class"):
        logistic_design(np.zeros(40), cov)
    with pytest.raises(ValueError, match="one class"):
        logistic_design(np.ones(40), cov)
    with pytest.raises(ValueError, match="rows"):
        logistic_design(y, cov[:39])
    with pytest.raises(ValueError, match="rank"):
        logistic_design(y, np.concatenate([cov, cov[:, :1] * 2 - cov[:, 1:2]], axis=1))
    with pytest.raises(ValueError, match="degree"):
        logistic_design(np.array([0.0, 1, 0, 1, 1]), cov[:5])           # n - q - 1 = 5 - 4 - 1
    with pytest.raises(ValueError, match=str(LOGIT_MAX_COLS)):
        logistic_design(y, rng.normal(size=(40, 14)))                  # 15 columns and the variant
    logistic_design(y, rng.normal(size=(40, 13)))
    with pytest.raises(ValueError, match="separate"):
        logistic_design(y, np.concatenate([cov, (y * 2 - 1 + 0.1 * rng.normal(size=40))[:, None]], axis=1))
    with pytest.raises(ValueError, match="one phenotype"):
        logistic_design(np.stack([y, y], axis=1), cov)


# ---- logistic_fit_reference ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fits():
    """per case: the inputs, the reference's records and the longdouble scan (computed once, never changed)"""
    out = {}
    for n, q0, seed in CASES:
        G, y, cov, dependent = case_control(n, q0, seed)
        X, beta0 = logistic_design(y, cov)
        rec = logistic_fit_reference(dosages(G), X, y, beta0)
        out[n, q0] = dict(G=G, y=y, cov=cov, dependent=dependent, X=X, beta0=beta0, rec=rec,
                          want=longdouble_scan(G, X, y, beta0, dependent))
    return out


@pytest.mark.parametrize("n, q0", [c[:2] for c in CASES])
def test_reference_matches_longdouble(fits, n, q0):
    f = fits[n, q0]
    stats, calls, info = logistic_from_fit(f["rec"])
    assert stats.dtype == np.float64 and stats.shape == (300, 6) and calls.dtype == np.int64 and info.dtype == np.int64
    D = dosages(f["G"])
    assert np.array_equal(calls, np.stack([(~np.isnan(D)).sum(1), (D == 1).sum(1), (D == 2).sum(1)], axis=1))
    # the constructed variants, and nothing hidden behind "not converged": its share among the admitted variants is 0
    want_status = np.zeros(300, dtype=np.int64)
    want_status[0], want_status[1] = LOGIT_ONE_CLASS, LOGIT_NO_CALL
    want_status[list(f["dependent"])] = LOGIT_COLLINEAR
    assert np.array_equal(info[:, 1], want_status)
    assert np.array_equal(np.isnan(stats), np.isnan(f["want"])) and np.isnan(stats).all(1).sum() == 2 + len(f["dependent"])
    tested = info[:, 1] == LOGIT_TESTED
    assert info[tested, 0].min() >= 1 and info[tested, 0].max() <= 8 and (info[~tested, 0] == 0).all()
    dw, ds = wald_diff(stats, f["want"]), score_diff(stats, f["want"])
    print(f"logistic_fit_reference n={n} q0={q0}: BETA / SE differ from longdouble by {dw:.3g}, the score chi^2 by {ds:.3g}; "
          f"steps {np.bincount(info[tested, 0]).tolist()}")
    assert dw <= LOGIT_RTOL and ds <= SCORE_RTOL
    # Z and the two P follow from the three by the stated formulas
    assert np.allclose(stats[tested, LOGIT_Z], stats[tested, LOGIT_BETA] / stats[tested, LOGIT_SE], rtol=1e-15)
    assert np.allclose(stats[:, LOGIT_P], f["want"][:, LOGIT_P], rtol=1e-9, atol=0, equal_nan=True)
    assert np.allclose(stats[:, LOGIT_SCORE_P], f["want"][:, LOGIT_SCORE_P], rtol=1e-9, atol=0, equal_nan=True)
    assert (stats[tested, LOGIT_SE] > 0).all() and (stats[tested, LOGIT_P] > 0).all() and (stats[tested, LOGIT_P] <= 1).all()
    # one variant alone: the same record; torch answers in kind, with the same numbers
    one = logistic_fit_reference(D[7], f["X"], f["y"], f["beta0"])
    assert one.shape == (LOGIT_REC,) and np.array_equal(one, f["rec"][7])
    ts, tc, ti = logistic_from_fit(torch.from_numpy(f["rec"]))
    assert ts.dtype == torch.float64 and tc.dtype == torch.int64 and np.array_equal(tc.numpy(), calls)
    assert np.array_equal(ti.numpy(), info) and np.allclose(ts.numpy(), stats, rtol=1e-13, atol=0, equal_nan=True)


def test_reference_refuses():
    f = case_control(96, 1, 20)
    X, beta0 = logistic_design(f[1], f[2])
    D = dosages(f[0])
    with pytest.raises(ValueError, match="0, 1, 2"):
        logistic_fit_reference(np.where(np.arange(96) == 3, 0.5, D[7]), X, f[1], beta0)
    for args in ((D[:, :95], X, f[1], beta0), (D, X, f[1][:95], beta0), (D, X, f[1], beta0[:1])):
        with pytest.raises(ValueError):
            logistic_fit_reference(*args)
    with pytest.raises(ValueError):
        logistic_from_fit(np.zeros((4, LOGIT_REC + 1)))


def separated(y, rng, k):
    """k dosage rows [k, n] that separate the classes: a dosage above 0 exactly in the cases"""
    return np.where(y[None, :] == 1, rng.integers(1, 3, (k, len(y))), 0).astype(np.float64)


def test_separated_variant_is_not_converged():
    """dosage > 0 exactly in the cases: the likelihood has no maximum, the steps never fall below 1e-8, and the variant comes
    out "not converged" with NaN statistics (Firth's correction is out of scope) — counted one by one"""
    G, y, cov, _ = case_control(200, 2, 20)
    X, beta0 = logistic_design(y, cov[:, :1])
    S = separated(y, np.random.default_rng(4), 3)
    rec = logistic_fit_reference(np.concatenate([S, dosages(G)[3:6]]), X, y, beta0)
    stats, calls, info = logistic_from_fit(rec)
    assert info[:, 1].tolist() == [LOGIT_NOT_CONVERGED] * 3 + [LOGIT_TESTED] * 3
    assert np.isnan(stats[:3]).all() and not np.isnan(stats[3:]).any() and (info[:3, 0] >= 1).all()
    assert np.isnan(rec[:3, REC_GAMMA]).all() and np.isnan(rec[:3, REC_HINV]).all() and not np.isnan(rec[:3, REC_U0]).any()
    assert (calls[:3, 0] == 200).all()


def test_record_layout_is_the_headers():
    src = open(os.path.join(ROOT, "include", "hhgt.h")).read()
    value = lambda name: int(re.search(r"#define\s+HHGT_LOGIT_" + name + r"\s+(\d+)", src).group(1))
    assert [value(n) for n in ("GAMMA", "HINV", "U0", "HINV0", "STEPS", "STATUS", "N_COMPLETE", "N_HET", "N_ALT")] == \
        [REC_GAMMA, REC_HINV, REC_U0, REC_HINV0, REC_STEPS, REC_STATUS, REC_COMPLETE, REC_HET, REC_ALT] == list(range(9))
    assert value("REC") == LOGIT_REC == 9 and value("MAX_COLS") == LOGIT_MAX_COLS == 15 and value("MAX_STEPS") == 25
    assert [value(n) for n in ("TESTED", "NO_CALL", "ONE_CLASS", "COLLINEAR", "NOT_CONVERGED")] == \
        [LOGIT_TESTED, LOGIT_NO_CALL, LOGIT_ONE_CLASS, LOGIT_COLLINEAR, LOGIT_NOT_CONVERGED] == list(range(5))
    assert (LOGIT_BETA, LOGIT_SE, LOGIT_Z, LOGIT_P, LOGIT_SCORE_CHI2, LOGIT_SCORE_P) == tuple(range(6))


# ---- normal_two_sided ------------------------------------------------------------------------------------------------------------
def test_normal_tail():
    z = np.array([0.0, 1e-3, 0.5, 1.0, 1.959963984540054, 3.0, 5.0, 8.0, 12.0, 20.0, 30.0, 37.0])
    p = normal_two_sided(np.concatenate([-z[::-1], z]).reshape(2, -1))
    assert p.dtype == np.float64 and p.shape == (2, len(z)) and np.array_equal(p[0], p[1][::-1])     # even in z
    p = p[1]
    assert p[0] == 1.0 and abs(p[4] - 0.05) < 1e-15 and abs(p[3] - 0.31731050786291415) < 1e-15
    assert (np.diff(p) < 0).all() and (p > 0).all() and p[-1] < 1e-298
    # the tail by its own series, erfc(x) = exp(-x^2) / (x sqrt(pi)) (1 - 1/(2x^2) + 3/(4x^4) - 15/(8x^6) + 105/(16x^8)):
    # relative accuracy down to 1e-300
    x = z[6:] / math.sqrt(2)
    series = np.exp(-x * x) / (x * math.sqrt(math.pi)) * (1 - 1 / (2 * x**2) + 3 / (4 * x**4) - 15 / (8 * x**6) + 105 / (16 * x**8))
    bound = 945 / (32 * x**10) + 1e-12
    assert (np.abs(p[6:] / series - 1) < bound).all() and bound[-1] < 2e-12
    t = normal_two_sided(torch.from_numpy(z))
    assert t.dtype == torch.float64 and np.abs(t.numpy() / p - 1).max() < 1e-12
    assert np.isnan(normal_two_sided(np.array([np.nan]))).all() and normal_two_sided(np.array([np.inf]))[0] == 0.0
    assert torch.isnan(normal_two_sided(torch.tensor([float("nan")], dtype=torch.float64))).all()


# ---- logistic_score_from_sums -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, q0", [c[:2] for c in CASES])
def test_score_from_sums_matches_the_first_evaluation(fits, n, q0):
    f = fits[n, q0]
    want, want_calls, want_info = logistic_from_fit(f["rec"])
    W, XWX = logistic_score_design(f["X"], f["y"], f["beta0"])
    q = f["X"].shape[1]
    assert W.shape == (n, 3 + q) and XWX.shape == (q, q)
    T = np_sums(f["G"], W)
    stats, calls, info = logistic_score_from_sums(T, W.sum(axis=0), q, XWX)
    assert np.array_equal(calls, want_calls) and np.array_equal(info[:, 1], want_info[:, 1]) and not info[:, 0].any()
    assert np.isnan(stats[:, :LOGIT_SCORE_CHI2]).all()
    assert np.array_equal(np.isnan(stats[:, LOGIT_SCORE_CHI2]), np.isnan(want[:, LOGIT_SCORE_CHI2]))
    d = score_diff(stats, want)
    print(f"logistic_score_from_sums n={n} q0={q0}: the chi^2 differs from the reference's first evaluation by {d:.3g}")
    assert d <= SCORE_RTOL
    assert np.allclose(stats[:, LOGIT_SCORE_P], want[:, LOGIT_SCORE_P], rtol=1e-8, atol=0, equal_nan=True)
    ts, tc, ti = logistic_score_from_sums(torch.from_numpy(T), torch.from_numpy(W.sum(axis=0)), q, torch.from_numpy(XWX))
    assert ts.dtype == torch.float64 and np.array_equal(tc.numpy(), calls) and np.array_equal(ti.numpy(), info)
    assert np.allclose(ts.numpy(), stats, rtol=1e-9, atol=1e-18, equal_nan=True)
    with pytest.raises(ValueError):
        logistic_score_from_sums(T, W.sum(axis=0), q + 1, XWX)


def test_score_test_stands_where_the_fit_separates():
    G, y, cov, _ = case_control(200, 2, 20)
    X, beta0 = logistic_design(y, cov[:, :1])
    S = separated(y, np.random.default_rng(4), 2)
    Gs = np.stack([(S >= 1).T, (S >= 2).T], axis=2).astype(np.int8)                     # [n, 2, 2]
    W, XWX = logistic_score_design(X, y, beta0)
    stats, _, info = logistic_score_from_sums(np_sums(Gs, W), W.sum(axis=0), 2, XWX)
    rec = logistic_fit_reference(S, X, y, beta0)
    assert info[:, 1].tolist() == [LOGIT_TESTED] * 2 and rec[:, REC_STATUS].tolist() == [LOGIT_NOT_CONVERGED] * 2
    assert np.allclose(stats[:, LOGIT_SCORE_CHI2], rec[:, REC_U0] ** 2 * rec[:, REC_HINV0], rtol=SCORE_RTOL, atol=0)


# ---- the declaration --------------------------------------------------------------------------------------------------------------
def test_lib_declares_hhgt_logistic_fit_as_the_header_does():
    from haplohyped_varawareml_amd import _lib, build
    build.build()
    L = _lib.load()
    args = header_prototype("hhgt_logistic_fit")
    assert args == ["hhgt_ctx *ctx", "const uint32_t *d_vplanes", "uint64_t n_var", "uint64_t sw", "const uint32_t *d_valid",
                    "const double *d_x", "uint32_t q", "const double *d_y", "const double *d_beta0", "double *d_out",
                    "void *stream"]
    want = [ctypes.c_void_p if "*" in a else {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}[a.split()[0]]
            for a in args]
    assert list(L.hhgt_logistic_fit.argtypes) == want and L.hhgt_logistic_fit.restype == ctypes.c_int
