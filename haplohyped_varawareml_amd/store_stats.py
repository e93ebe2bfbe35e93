"""The columns of GenotypeStore's count tables and the statistics read from them.  Every formula is written once and takes
a numpy array or a torch tensor (on any device), answering in kind: _ops hands it the few operations the two spell
differently."""
import numpy as np

# columns of GenotypeStore.allele_counts (and of hhgt_count_alleles' counters)
AN, AC, HET, HOM_ALT = 0, 1, 2, 3

# columns of GenotypeStore.pair_counts (and of hhgt_pair_counts' table), for the ordered pair (i, j) over the counted variants.
# A call is complete iff both alleles are 0 or 1; a missing allele or an allele >= 2 takes the call out of every column.
NSNP, HETHET, IBS0, HET1 = 0, 1, 2, 3    # both complete; both HET; opposite homozygotes; i HET and j complete

# columns of GenotypeStore.ld_counts (and of hhgt_ld_counts' table), for the ordered pair (u, v) of counted variants, v after
# u, over the counted samples: M = the call is complete, H = HET, A = HOM_ALT.  The dosage of a complete call is 0, 1, 2.
LD_N, LD_HM, LD_AM, LD_MH, LD_MA = 0, 1, 2, 3, 4     # Mu Mv; Hu Mv; Au Mv; Mu Hv; Mu Av
LD_HH, LD_HA, LD_AA = 5, 6, 7                        # Hu Hv; Hu Av or Au Hv; Au Av


def _ops(x):
    """-> (i64, f64, minimum, nan_unless) for x's kind, numpy array or torch tensor: conversion to int64 and to float64,
    the elementwise minimum, and nan_unless(ok, a): a where ok, NaN elsewhere.  (Indexing, arithmetic and .T of a matrix
    are the same in both.)"""
    if type(x).__module__.split(".")[0] == "torch":
        import torch
        return (lambda a: a.to(torch.int64), lambda a: a.to(torch.float64), torch.minimum,
                lambda ok, a: torch.where(ok, a, torch.full_like(a, float("nan"))))
    return (lambda a: np.asarray(a).astype(np.int64), lambda a: a.astype(np.float64), np.minimum,
            lambda ok, a: np.where(ok, a, np.nan))


def ibs_counts(table):
    """pair table [n, n, 4] (numpy or torch, any integer type) -> (IBS0, IBS1, IBS2), int64 [n, n] each: the variants at
    which a pair's complete calls share no, one, both alleles.  IBS2 = 2 HETHET + NSNP - HET1[i][j] - HET1[j][i] - IBS0
    (identical genotypes), IBS1 = NSNP - IBS0 - IBS2."""
    t = _ops(table)[0](table)
    ibs2 = 2 * t[..., HETHET] + t[..., NSNP] - t[..., HET1] - t[..., HET1].T - t[..., IBS0]
    return t[..., IBS0], t[..., NSNP] - t[..., IBS0] - ibs2, ibs2


def kinship_from_counts(table):
    """pair table [n, n, 4] (numpy or torch) -> float64 [n, n]: the KING-robust between-family kinship estimator
    (Manichaikul et al. 2010) as this project defines it,
        phi = 1/2 - (4 IBS0 + HET1[i][j] + HET1[j][i] - 2 HETHET) / (4 min(HET1[i][j], HET1[j][i])),
    in float64 from the integer table, NaN where the minimum is 0.  A sample against itself or against a duplicate gives
    exactly 0.5.  The formula is the contract: equality with plink2's KINSHIP column is neither claimed nor tested."""
    i64, f64, minimum, nan_unless = _ops(table)
    t = i64(table)
    h1, h2 = t[..., HET1], t[..., HET1].T
    num = f64(4 * t[..., IBS0] + h1 + h2 - 2 * t[..., HETHET])
    den = f64(4 * minimum(h1, h2))
    with np.errstate(divide="ignore", invalid="ignore"):
        return nan_unless(den > 0, 0.5 - num / den)


def ld_sums(table):
    """LD table [..., 8] (numpy or torch, any integer type) -> (n, sx, sy, sxx, syy, sxy), int64 each: over the samples at
    which both calls of a pair are complete, their number and the sums of the dosages x (first variant) and y (second),
    of their squares and of their products: sx = HM + 2 AM, sxx = HM + 4 AM, sy = MH + 2 MA, syy = MH + 4 MA,
    sxy = HH + 2 HA + 4 AA."""
    t = _ops(table)[0](table)
    return (t[..., LD_N], t[..., LD_HM] + 2 * t[..., LD_AM], t[..., LD_MH] + 2 * t[..., LD_MA],
            t[..., LD_HM] + 4 * t[..., LD_AM], t[..., LD_MH] + 4 * t[..., LD_MA],
            t[..., LD_HH] + 2 * t[..., LD_HA] + 4 * t[..., LD_AA])


def _ld_products(table):
    """-> (num * num, dx * dy) of an LD table, float64: num = N sxy - sx sy, dx = N sxx - sx^2, dy = N syy - sy^2 in int64,
    converted, and the two products, each rounded once"""
    f64 = _ops(table)[1]
    n, sx, sy, sxx, syy, sxy = ld_sums(table)
    num, dx, dy = f64(n * sxy - sx * sy), f64(n * sxx - sx * sx), f64(n * syy - sy * sy)
    return num * num, dx * dy


def r2_from_counts(table):
    """LD table [n, W, 8] (numpy or torch) -> float64 [n, W]: r^2 = (num * num) / (dx * dy) with num = N sxy - sx sy,
    dx = N sxx - sx^2, dy = N syy - sy^2 of ld_sums — the squared Pearson correlation of the two variants' dosages over
    the samples at which both calls are complete (unphased).  NaN where dx * dy = 0: one of the two is monomorphic among
    those samples, or there are none.  A variant against a duplicate of itself gives exactly 1.0.  The formula is the
    contract: equality with plink2's --r2-unphased column is neither claimed nor tested."""
    nn, den = _ld_products(table)
    with np.errstate(divide="ignore", invalid="ignore"):
        return _ops(table)[3](den != 0, nn / den)


def ld_exceeds(table, r2):
    """LD table [n, W, 8] (numpy or torch) -> bool [n, W]: num * num > r2 * (dx * dy), the three products in float64 and
    each rounded once — the decision hhgt_ld_prune makes from the same integers, bit for bit.  A pair whose r^2 is NaN
    (zero denominator) never exceeds."""
    nn, den = _ld_products(table)
    return nn > float(r2) * den


# plane words of one f32 chain of hhgt_grm (HHGT_GRM_SPAN of include/hhgt.h): the K of its error bound is 32 * GRM_SPAN
GRM_SPAN = 128


def standardized_dosages(counts):
    """allele count table [V, 4] (numpy or torch, columns AN, AC, ...) -> (z, used): z float32 [3, V], the standardised
    value of a complete call of dosage d = 0, 1, 2 (HOM_REF, HET, HOM_ALT) at every variant, and used bool [V].  A variant
    is used iff AN > 0 and 0 < AC < AN; then p = AC / AN and z[d] = (d - 2p) / sqrt(2p(1 - p)), computed in float64 and
    rounded once to float32 (the standardisation of GCTA's and plink2 --make-rel's relationship matrix).  A variant that
    is not used has 0 in all three."""
    i64, f64 = _ops(counts)[:2]
    t = i64(counts)
    an, ac = t[..., AN], t[..., AC]
    used = (an > 0) & (ac > 0) & (ac < an)
    # (a variant that is not used gets p = 1/2 here, so that nothing divides by 0, and 0 at the end)
    p = f64(ac * used + (~used) * 1) / f64(an * used + (~used) * 2)
    sd = (2.0 * p * (1.0 - p)) ** 0.5
    rows = [(float(d) - 2.0 * p) / sd for d in range(3)]
    if type(counts).__module__.split(".")[0] == "torch":
        import torch
        z = torch.stack(rows)
        return torch.where(used, z, torch.zeros_like(z)).to(torch.float32), used
    return np.where(used, np.stack(rows), 0.0).astype(np.float32), used


def grm_from_sums(S, N):
    """(S float64 [n, n], N integer [n, n]) of GenotypeStore.grm_sums (numpy or torch) -> float64 [n, n]: the genetic
    relationship matrix S / N — per pair, the mean over the variants at which both calls are complete of the product of
    the two standardised dosages —, NaN where N == 0.  The formula is the contract: equality with GCTA's or plink2's
    files is neither claimed nor tested."""
    _, f64, _, nan_unless = _ops(S)
    with np.errstate(divide="ignore", invalid="ignore"):
        return nan_unless(N != 0, f64(S) / f64(N))


def top_eigenpairs(grm, k):
    """symmetric float64 [n, n] (host numpy) -> (values float64 [k], vectors float64 [n, k]): the k largest eigenpairs of
    numpy.linalg.eigh, in descending order; every vector of unit length as eigh returns it, its sign chosen so that its
    component of largest magnitude (the first such one) is positive.  ValueError if k is outside 1..n or the matrix holds
    a NaN (the message counts the pairs i <= j)."""
    g = np.asarray(grm, dtype=np.float64)
    n, k = g.shape[0], int(k)
    if g.ndim != 2 or g.shape[1] != n:
        raise ValueError(f"pca: a square matrix, not {g.shape}")
    if not 1 <= k <= n:
        raise ValueError(f"pca: k = {k} (1 to {n})")
    bad = int(np.isnan(g[np.triu_indices(n)]).sum())
    if bad:
        raise ValueError(f"pca: {bad} pair(s) of samples have no jointly complete variant (NaN in the relationship matrix)")
    w, v = np.linalg.eigh(g)
    w, v = w[::-1][:k].copy(), v[:, ::-1][:, :k].copy()
    lead = np.argmax(np.abs(v), axis=0)
    v[:, v[lead, np.arange(k)] < 0] *= -1.0
    return w, v
