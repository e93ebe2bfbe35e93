"""The columns of GenotypeStore's count tables and the statistics read from them.  Every formula is written once and takes
a numpy array or a torch tensor (on any device), answering in kind: _ops hands it the few operations the two spell
differently."""
import math

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


# ---- LD clumping: the rule (include/hhgt.h restates it; hhgt_ld_decisions / hhgt_ld_clump compute it on the device) ----------
# Over the counted variants of a group, in file order: u < v are LINKED iff v - u <= window (in counted variants),
# ld_exceeds(u, v, r2) — strictly > — and, with a distance limit, |pos_v - pos_u| <= max_dist (inclusive).  rank: the place
# in a stable ascending sort by p, ties to the earlier variant.  Walk the variants in rank order: one that is eligible
# (p <= p1) and not yet claimed becomes an INDEX variant and claims every linked variant that is neither an index nor
# claimed.  owner[k]: k for an index; else the index that claimed it, which is the linked index of lowest rank; else -1
# (p > p1 or unclaimed, and no index is linked to it).  With every variant eligible and p strictly ascending in file order
# this is ld_prune's rule: owner[k] == k exactly where it keeps k.  It is this project's rule, not plink's .clumped file
# column for column: no --clump-replicate, no ranges, no secondary lists.

CLUMP_NONE, CLUMP_INDEX, CLUMP_CLUMPED = 0, 1, 2     # roles of clump_summary
CLUMP_ROLE_NAMES = ("none", "index", "clumped")


def clump_rank(p):
    """p [n] (numpy or torch) -> rank [n], int64 in kind: the position of each variant in a stable ascending sort by p, so
    that equal p rank in file order"""
    if type(p).__module__.split(".")[0] == "torch":
        import torch
        order = torch.sort(p, stable=True).indices
        rank = torch.empty_like(order)
        rank[order] = torch.arange(len(order), dtype=order.dtype, device=order.device)
        return rank
    order = np.argsort(np.asarray(p), kind="stable")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return rank


def clump_reference(linked_back, p, p1):
    """the sequential rule above, plain numpy: linked_back bool [n, window] — [k, d]: variant k is linked with the variant
    d + 1 places before it (entries that point before variant 0 are ignored) —, p float [n], p1 the index threshold
    -> owner int64 [n].  This is the contract the device route is held to."""
    linked_back = np.asarray(linked_back, bool)
    p = np.asarray(p, np.float64)
    n, window = len(p), linked_back.shape[1] if linked_back.ndim == 2 else 0
    owner = np.full(n, -1, np.int64)
    is_index = np.zeros(n, bool)
    for k in np.argsort(p, kind="stable").tolist():
        if not p[k] <= p1 or owner[k] >= 0:
            continue
        owner[k], is_index[k] = k, True
        d = np.flatnonzero(linked_back[k, :min(window, k)])
        back = k - 1 - d
        e = np.arange(min(window, n - 1 - k))
        ahead = k + 1 + e[linked_back[k + 1 + e, e]]
        for nb in (back, ahead):
            nb = nb[owner[nb] < 0]
            owner[nb] = k
    return owner


def clump_summary(owner, p):
    """owner int [n] of a clumping and its p [n] (host arrays) -> dict: role int8 [n] (CLUMP_NONE, CLUMP_INDEX,
    CLUMP_CLUMPED), index int64 [m] (the index variants, in file order), n_clumped int64 [m] (the members each claimed,
    itself not counted), members (a list of m int64 arrays, each in file order), best int64 [m] (1 + the number of index
    variants with a lower p, ties to the earlier one: 1 is the strongest signal), n_index, n_clumped_total, n_none"""
    owner, p = np.asarray(owner, np.int64), np.asarray(p, np.float64)
    at = np.arange(len(owner))
    role = np.where(owner == at, CLUMP_INDEX, np.where(owner >= 0, CLUMP_CLUMPED, CLUMP_NONE)).astype(np.int8)
    index = at[role == CLUMP_INDEX]
    claimed = at[role == CLUMP_CLUMPED]
    slot = np.searchsorted(index, owner[claimed])
    n_clumped = np.bincount(slot, minlength=len(index)).astype(np.int64)
    by_slot = claimed[np.argsort(slot, kind="stable")]
    members = np.split(by_slot, np.cumsum(n_clumped)[:-1]) if len(index) else []
    best = np.empty(len(index), np.int64)
    best[np.argsort(p[index], kind="stable")] = np.arange(1, len(index) + 1)
    return dict(role=role, index=index, n_clumped=n_clumped, members=members, best=best, n_index=len(index),
                n_clumped_total=len(claimed), n_none=int((role == CLUMP_NONE).sum()))


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


def check_components(k, n):
    """int(k), the number of principal components asked of n samples: ValueError if it is outside 1..n"""
    if not 1 <= int(k) <= n:
        raise ValueError(f"pca: k = {int(k)} (1 to {n})")
    return int(k)


def top_eigenpairs(grm, k):
    """symmetric float64 [n, n] (host numpy) -> (values float64 [k], vectors float64 [n, k]): the k largest eigenpairs of
    numpy.linalg.eigh, in descending order; every vector of unit length as eigh returns it, its sign chosen so that its
    component of largest magnitude (the first such one) is positive.  ValueError if k is outside 1..n or the matrix holds
    a NaN (the message counts the pairs i <= j)."""
    g = np.asarray(grm, dtype=np.float64)
    if g.ndim != 2 or g.shape[1] != g.shape[0]:
        raise ValueError(f"pca: a square matrix, not {g.shape}")
    n, k = g.shape[0], check_components(k, g.shape[0])
    bad = int(np.isnan(g[np.triu_indices(n)]).sum())
    if bad:
        raise ValueError(f"pca: {bad} pair(s) of samples have no jointly complete variant (NaN in the relationship matrix)")
    w, v = np.linalg.eigh(g)
    w, v = w[::-1][:k].copy(), v[:, ::-1][:, :k].copy()
    lead = np.argmax(np.abs(v), axis=0)
    v[:, v[lead, np.arange(k)] < 0] *= -1.0
    return w, v


# hhgt_score_sums' geometry (HHGT_SCORE_SLICE, HHGT_SCORE_SPAN of include/hhgt.h): plane words whose weights are staged at a
# time, and plane words per span of a range of up to SCORE_SPAN * 65535 words — the kernel's paths change at their multiples
SCORE_SLICE = 1
SCORE_SPAN = 64
# columns of the per-variant weights a call of hhgt_score_sums takes at most
SCORE_MAX_COLS = 64


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def score_class_weights(beta, counts, impute="mean"):
    """the per-class weights of a polygenic score -> (Wd float64 [3, V, K], offset float64 [K], used bool [V]): beta is
    [V, K] (or [V]: K = 1), the effect per ALT allele of every variant in each of K scores, counts an allele count table
    [V, 4] of the frequency samples (numpy or torch, both of one kind).  impute = "mean": with p = AC / AN as in
    standardized_dosages, Wd[d] = (d - 2p) beta for a complete call of dosage d = 0, 1, 2 and offset = the sum over the
    variants of 2p beta; a variant with AN == 0 is not used: zeros, nothing in the offset.  A call that is not complete has
    no bit and contributes 0, so offset + (the sum of Wd over a sample's calls) = the sum over the used variants of beta x
    (the dosage, or 2p where the call is not complete).  impute = "none": Wd[d] = d beta, offset 0, every variant used: a
    call that is not complete counts as dosage 0.  Scores are sums, not per-allele averages: plink2's .sscore is not the
    contract.  ValueError for another impute, a beta that is not [V] or [V, K] or not of counts' length."""
    if impute not in ("mean", "none"):
        raise ValueError(f"score_class_weights: impute {impute!r} (\"mean\" or \"none\")")
    i64, f64 = _ops(counts)[:2]
    stack = _math(counts)[4]
    if _is_torch(beta) != _is_torch(counts):
        raise ValueError("score_class_weights: beta and counts must both be numpy arrays or both torch tensors")
    b = f64(beta)
    if len(b.shape) == 1:
        b = b[:, None]
    if len(b.shape) != 2 or len(counts.shape) != 2 or counts.shape[1] != 4 or b.shape[0] != counts.shape[0]:
        raise ValueError(f"score_class_weights: beta {list(beta.shape)} ([V] or [V, K]) for counts {list(counts.shape)} ([V, 4])")
    t = i64(counts)
    an, ac = t[:, AN], t[:, AC]
    if impute == "none":
        used = an == an
        two_p = f64(an) * 0.0
    else:
        used = an > 0
        # (a variant that is not used gets AN = 1 here, so that nothing divides by 0, and 0 at the end)
        two_p = 2.0 * (f64(ac * used) / f64(an * used + (~used) * 1))
    bu = b * f64(used)[:, None]
    Wd = stack([(float(d) - two_p)[:, None] * bu for d in range(3)])
    return Wd, (two_p[:, None] * bu).sum(0), used


def loadings_from_sums(T, z, values, n_variants):
    """the variant loadings of principal components from the sums over the fitted samples -> float64 [n_counted, k]: T is
    float64 [n_counted, 3, k], GenotypeStore.assoc_sums of the eigenvectors U [n, k] of the relationship matrix (planes
    ASSOC_HET, ASSOC_COMPLETE, ASSOC_ALT), z [3, n_counted] the standardised dosages of the same variants
    (standardized_dosages over the same samples), values [k] the eigenvalues, n_variants the number of variants the matrix
    was averaged over (all groups).  A = z[0] (T_COMPLETE - T_HET - T_ALT) + z[1] T_HET + z[2] T_ALT is X^T U for the
    standardised dosage matrix X (0 where a call is not complete), and loadings = A / (n_variants * values): where no call
    is incomplete the relationship matrix is X X^T / n_variants, so X loadings = U.  ValueError if an eigenvalue is <= 0
    or the shapes disagree."""
    f64 = _ops(T)[1]
    T, z = f64(T), f64(z)
    lam = np.asarray(values.detach().cpu().numpy() if _is_torch(values) else values, dtype=np.float64).reshape(-1)
    if len(T.shape) != 3 or T.shape[1] != 3 or tuple(z.shape) != (3, T.shape[0]) or len(lam) != T.shape[2]:
        raise ValueError(f"loadings_from_sums: T {list(T.shape)} ([n, 3, k]), z {list(z.shape)} ([3, n]), {len(lam)} values (k)")
    if not (lam > 0).all():
        raise ValueError(f"loadings_from_sums: eigenvalue {lam[~(lam > 0)][0]:g} (every eigenvalue must be positive)")
    if int(n_variants) < 1:
        raise ValueError(f"loadings_from_sums: {int(n_variants)} variants")
    ref = T[:, ASSOC_COMPLETE] - T[:, ASSOC_HET] - T[:, ASSOC_ALT]
    A = z[0][:, None] * ref + z[1][:, None] * T[:, ASSOC_HET] + z[2][:, None] * T[:, ASSOC_ALT]
    scale = float(int(n_variants)) * lam
    if _is_torch(T):
        import torch
        scale = torch.from_numpy(scale).to(T.device)
    return A / scale[None, :]


def projection_class_weights(z, loadings):
    """(z [3, V] of standardized_dosages, loadings float64 [V, k]; numpy or torch) -> Wd float64 [3, V, k]:
    Wd[d, v, c] = z[d, v] * loadings[v, c], the weight of a complete call of dosage d in component c — zero where the
    variant is not used, for z is zero there.  ValueError if the shapes disagree."""
    f64 = _ops(z)[1]
    if len(z.shape) != 2 or z.shape[0] != 3 or len(loadings.shape) != 2 or loadings.shape[0] != z.shape[1]:
        raise ValueError(f"projection_class_weights: z {list(z.shape)} ([3, V]), loadings {list(loadings.shape)} ([V, k])")
    return f64(z)[:, :, None] * f64(loadings)[None, :, :]


def _is_integer_dtype(dtype):
    """a numpy or torch dtype (or its name) is an integer type"""
    return "int" in str(dtype)


def call_class_values(counts, coding, impute, dtype=None):
    """the value of each call class at every variant of a feature matrix -> (values float64 [4, V], used bool [V]):
    counts is an allele count table [V, 4] of the frequency samples (numpy or torch; columns AN, AC, ...), the classes
    those of hhgt_gather_calls — 0 HOM_REF, 1 HET, 2 HOM_ALT, 3 not complete.  coding = "dosage": classes 0..2 take 0, 1,
    2; with impute = "mean" class 3 takes 2p, p = AC / AN, and a variant is used iff AN > 0 (an unused one: 0); with
    impute = "missing" class 3 takes the missing marker, every variant is used and the counts are not looked at.  coding =
    "standardized": classes 0..2 are standardized_dosages' z (float32 values, widened) and `used` is that function's;
    class 3 is 0.0, the mean, with "mean" and the missing marker with "missing".  The missing marker is NaN here; the cast
    (cast_class_values) makes it -1 for an integer dtype.  dtype (optional: the type the values will be cast to) only
    checks: "mean" with an integer dtype is a ValueError, for neither 2p nor z is an integer.  ValueError for another
    coding or impute."""
    if coding not in ("dosage", "standardized") or impute not in ("mean", "missing"):
        raise ValueError(f"call_class_values: coding {coding!r} (\"dosage\" or \"standardized\"), impute {impute!r} (\"mean\" or \"missing\")")
    if impute == "mean" and dtype is not None and _is_integer_dtype(dtype):
        raise ValueError(f"call_class_values: impute \"mean\" needs a float dtype, not {dtype} (an imputed value is no integer)")
    if len(counts.shape) != 2 or counts.shape[1] != 4:
        raise ValueError(f"call_class_values: counts {list(counts.shape)} ([V, 4])")
    i64, f64 = _ops(counts)[:2]
    stack = _math(counts)[4]
    t = i64(counts)
    an, ac = t[:, AN], t[:, AC]
    zero = f64(an) * 0.0
    missing = zero + float("nan")
    if coding == "dosage":
        if impute == "missing":
            return stack([zero, zero + 1.0, zero + 2.0, missing]), an == an
        used = an > 0
        # (a variant that is not used gets AN = 1 here, so that nothing divides by 0)
        two_p = 2.0 * (f64(ac * used) / f64(an * used + (~used) * 1))
        return stack([zero, zero + 1.0, zero + 2.0, two_p]), used
    z, used = standardized_dosages(counts)
    z = f64(z)
    return stack([z[0], z[1], z[2], zero if impute == "mean" else missing]), used


def cast_class_values(values, dtype):
    """call_class_values' table (a torch tensor) as elements of a torch dtype: torch's .to(dtype), the missing marker (NaN)
    made -1 first for an integer dtype"""
    import torch
    if _is_integer_dtype(dtype):
        values = torch.where(torch.isnan(values), torch.full_like(values, -1.0), values)
    return values.to(dtype)


# columns of the statistics table of assoc_from_sums (and GenotypeStore.assoc), per variant and phenotype
ASSOC_BETA, ASSOC_SE, ASSOC_T, ASSOC_P = 0, 1, 2, 3
# planes of GenotypeStore.assoc_sums (and of hhgt_assoc_sums' sums), in the kernel's order: HET calls, complete calls (both
# alleles 0 or 1), HOM_ALT calls
ASSOC_HET, ASSOC_COMPLETE, ASSOC_ALT = 0, 1, 2
# columns of the per-sample matrix a call of hhgt_assoc_sums takes at most
ASSOC_MAX_COLS = 64


def _host_f64(x, name):
    """numpy array or torch tensor -> float64 numpy array on the host, every value finite"""
    if type(x).__module__.split(".")[0] == "torch":
        x = x.detach().cpu().numpy()
    a = np.asarray(x, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError(f"assoc_design: {name} holds a value that is not finite")
    return a


def assoc_design(y, covariates=None):
    """the per-sample matrix of an association scan -> (W, q, yy), host numpy, float64: y is [n] or [n, P] (P phenotypes),
    covariates [n, q0] or None (numpy or torch).  Q = the orthonormal basis of [1 | covariates] from numpy.linalg.qr
    (q = 1 + q0 columns), Yr = Y - Q Q^T Y the phenotypes with the covariates regressed out, W = [1 | Q | Yr],
    [n, 1 + q + P], and yy [P] the column sums of Yr^2.  ValueError for a value that is not finite, covariates of another
    row count than y, a rank-deficient [1 | covariates] (a diagonal entry of R below n * eps times the largest in
    magnitude), n - q - 1 < 1 (no degree of freedom left for the variant) and 1 + q + P > 64 (hhgt_assoc_sums' columns)."""
    Y = _host_f64(y, "y")
    if Y.ndim == 1:
        Y = Y[:, None]
    if Y.ndim != 2:
        raise ValueError(f"assoc_design: y of shape {Y.shape} ([n] or [n, P])")
    n, P = Y.shape
    X = np.ones((n, 1))
    if covariates is not None:
        cov = _host_f64(covariates, "covariates")
        if cov.ndim != 2 or cov.shape[0] != n:
            raise ValueError(f"assoc_design: covariates of shape {cov.shape} for {n} rows of y ([n, q0])")
        X = np.concatenate([X, cov], axis=1)
    q = X.shape[1]
    if n - q - 1 < 1:
        raise ValueError(f"assoc_design: {n} samples leave no degree of freedom beside {q} covariate columns and the variant")
    if 1 + q + P > ASSOC_MAX_COLS:
        raise ValueError(f"assoc_design: 1 + {q} covariate columns + {P} phenotypes exceed {ASSOC_MAX_COLS} columns")
    Q, R = np.linalg.qr(X)
    d = np.abs(np.diag(R))
    if d.min() < n * np.finfo(np.float64).eps * d.max():
        raise ValueError("assoc_design: [1 | covariates] is rank-deficient")
    Yr = Y - Q @ (Q.T @ Y)
    return np.concatenate([np.ones((n, 1)), Q, Yr], axis=1), q, (Yr * Yr).sum(axis=0)


def _math(x):
    """-> (log1p, exp, absolute, where, stack) for x's kind, numpy array or torch tensor"""
    if type(x).__module__.split(".")[0] == "torch":
        import torch
        return torch.log1p, torch.exp, torch.abs, torch.where, torch.stack
    return np.log1p, np.exp, np.abs, np.where, np.stack


def _beta_fraction(a, b, x, steps, absolute, where):
    """the continued fraction of the incomplete beta function at x (array), parameters a, b (numbers), by the modified
    Lentz recurrence run for `steps` double steps whatever the values"""
    tiny = 1e-300

    def guard(v):
        return where(absolute(v) < tiny, v * 0.0 + tiny, v)

    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = x * 0.0 + 1.0
    d = 1.0 / guard(1.0 - qab * x / qap)
    h = d
    for m in range(1, steps + 1):
        m2 = 2.0 * m
        for aa in (m * (b - m) / ((qam + m2) * (a + m2)), -(a + m) * (qab + m) / ((a + m2) * (qap + m2))):
            d = 1.0 / guard(1.0 + aa * x * d)
            c = guard(1.0 + aa * x / c)
            h = h * d * c
    return h


def student_t_two_sided(t, df):
    """the two-sided p-value of Student's t with df degrees of freedom (a number) at t (numpy or torch, any shape) ->
    float64 of t's shape: I_x(df / 2, 1 / 2) at x = df / (df + t^2), the regularised incomplete beta function, from its
    continued fraction.  The fraction has a fixed length that depends on df alone (50 + 8 sqrt(df / 2) double steps of the
    modified Lentz recurrence: it converges in O(sqrt(max(a, b))) steps), so every element does the same work and numpy
    and torch run the same operations.  For x above (a + 1) / (a + b + 2) the fraction is that of 1 - I_(1-x)(1/2, df/2);
    log x and log (1 - x) come from log1p of t^2 / df and df / t^2, so that a small p keeps its relative accuracy.
    t = 0 gives 1, an infinite t 0, NaN stays NaN."""
    log1p, exp, absolute, where, _ = _math(t)
    f64 = _ops(t)[1]
    df = float(df)
    a, b = 0.5 * df, 0.5
    steps = 50 + int(8.0 * math.sqrt(max(a, b)))
    lbeta = math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = f64(t) * f64(t)
        x, y = df / (df + u), u / (df + u)                      # y = 1 - x
        lnx, lny = -log1p(u / df), -log1p(df / u)
        front = exp(a * lnx + b * lny + lbeta)
        # (an infinite t: x is 0, y is NaN, and the direct branch, which is taken, is 0)
        direct = front * _beta_fraction(a, b, x, steps, absolute, where) / a
        mirror = 1.0 - front * _beta_fraction(b, a, y, steps, absolute, where) / b
        return where(x < (a + 1.0) / (a + b + 2.0), direct, mirror)


def assoc_from_sums(T, W_total, q, yy):
    """the statistics of a single-variant linear regression scan from the sums of GenotypeStore.assoc_sums ->
    (stats, calls): T float64 [V, 3, C] (planes ASSOC_HET, ASSOC_COMPLETE, ASSOC_ALT; columns those of assoc_design's
    W = [1 | Q | Yr], C = 1 + q + P), W_total [C] the column sums of W, yy [P] (numpy or torch, all of one kind).
    calls is int64 [V, 3]: the complete, HET and HOM_ALT calls of each variant among the listed samples (column 0 of T:
    exact).  With n = W_total[0], m, h, a those counts and mu = (h + 2a) / m — the dosage of a call that is not complete
    is imputed to the mean of the complete ones —,
        g.w_c = T[HET][c] + 2 T[ALT][c] + mu (W_total[c] - T[COMPLETE][c])      g.g = h + 4a + mu^2 (n - m)
        D = g.g - sum_j (g.Q_j)^2      U_p = g.Yr_p      beta = U / D      rss = yy - U^2 / D      df = n - q - 1
        se = sqrt(rss / df / D)        t = beta / se     p = student_t_two_sided(t, df)
    stats is float64 [V, P, 4], columns ASSOC_BETA, ASSOC_SE, ASSOC_T, ASSOC_P: the coefficient of the dosage in the least-
    squares fit of phenotype p on [1 | covariates | dosage].  All four are NaN where the variant is not tested: m == 0,
    fewer than two of the three complete classes (HOM_REF, HET, HOM_ALT) non-empty, or D <= 1e-12 g.g (the covariates
    explain the dosage).  The formula is the contract: plink2's .glm.linear, which drops the samples without a complete
    call per variant where this imputes, is not."""
    i64, f64, _, nan_unless = _ops(T)
    stack = _math(T)[4]
    q = int(q)
    T, W_total, yy = f64(T), f64(W_total), f64(yy)
    calls = stack([i64(T[:, ASSOC_COMPLETE, 0]), i64(T[:, ASSOC_HET, 0]), i64(T[:, ASSOC_ALT, 0])], -1)
    n = W_total[0]
    m, h, a = T[:, ASSOC_COMPLETE, 0], T[:, ASSOC_HET, 0], T[:, ASSOC_ALT, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = (h + 2.0 * a) / m
        gw = T[:, ASSOC_HET] + 2.0 * T[:, ASSOC_ALT] + mu[:, None] * (W_total[None, :] - T[:, ASSOC_COMPLETE])
        gg = h + 4.0 * a + mu * mu * (n - m)
        D = gg - (gw[:, 1:1 + q] * gw[:, 1:1 + q]).sum(-1)
        classes = i64(m - h - a > 0) + i64(h > 0) + i64(a > 0)
        tested = (m > 0) & (classes >= 2) & (D > 1e-12 * gg)
        U = gw[:, 1 + q:]
        df = n - q - 1
        beta = U / D[:, None]
        rss = yy[None, :] - U * U / D[:, None]
        se = (rss / df / D[:, None]) ** 0.5
        t = beta / se
        p = student_t_two_sided(t, float(df))
        stats = stack([beta, se, t, p], -1)
        return nan_unless(tested[:, None, None], stats), calls


# ---- the case / control scan: a logistic regression per variant -----------------------------------------------------------------
# columns of the statistics table of logistic_from_fit (and GenotypeStore.assoc_logistic), per variant and phenotype
LOGIT_BETA, LOGIT_SE, LOGIT_Z, LOGIT_P, LOGIT_SCORE_CHI2, LOGIT_SCORE_P = 0, 1, 2, 3, 4, 5
# columns of [X | dosage] that hhgt_logistic_fit's tile takes at most (HHGT_LOGIT_MAX_COLS): X has one fewer
LOGIT_MAX_COLS = 15
# Newton steps at most (HHGT_LOGIT_MAX_STEPS), the step below which they end, the pivot below which an evaluation fails
LOGIT_MAX_STEPS, LOGIT_STEP_TOL, LOGIT_PIVOT_TOL = 25, 1e-8, 1e-12
# the per-variant record of hhgt_logistic_fit and logistic_fit_reference (HHGT_LOGIT_* of include/hhgt.h): the dosage's
# coefficient and (H^-1)_gg after the last step, the dosage's entry of the gradient and (H^-1)_gg at the first evaluation,
# steps, status, complete / HET / HOM_ALT calls
LOGIT_REC = 9
REC_GAMMA, REC_HINV, REC_U0, REC_HINV0, REC_STEPS, REC_STATUS, REC_COMPLETE, REC_HET, REC_ALT = range(9)
# the status of a variant: fitted; no complete call; fewer than two of HOM_REF / HET / HOM_ALT; the first evaluation's
# factorisation failed (the covariates explain the dosage); a later one failed or the last permitted step was too large
LOGIT_TESTED, LOGIT_NO_CALL, LOGIT_ONE_CLASS, LOGIT_COLLINEAR, LOGIT_NOT_CONVERGED = 0, 1, 2, 3, 4
LOGIT_STATUS_NAMES = ("tested", "no call", "one class", "collinear", "not converged")


def normal_two_sided(z):
    """the two-sided p-value of a standard normal at z (numpy or torch, any shape) -> float64 of z's shape:
    erfc(|z| / sqrt 2), from the C library's erfc (numpy: math.erfc element by element) or torch.special.erfc — both keep
    their relative accuracy in the tail, down to the smallest normal numbers.  NaN stays NaN."""
    f64 = _ops(z)[1]
    x = _math(z)[2](f64(z)) / math.sqrt(2.0)
    if _is_torch(z):
        import torch
        return torch.special.erfc(x)
    x = np.asarray(x, dtype=np.float64)
    return np.frompyfunc(math.erfc, 1, 1)(x).astype(np.float64).reshape(x.shape)


def _logit_evaluate(Xt, y, theta):
    """one evaluation of V models at once: Xt [V or 1, n, p], y [n], theta [V, p] -> (U [V, p], H [V, p, p]):
    eta = Xt theta, mu = 1 / (1 + exp(-eta)), w = mu (1 - mu), U = Xt^T (y - mu), H = Xt^T diag(w) Xt"""
    Xt = np.broadcast_to(Xt, (theta.shape[0],) + Xt.shape[1:])
    with np.errstate(over="ignore", invalid="ignore"):
        mu = 1.0 / (1.0 + np.exp(-np.matmul(Xt, theta[:, :, None])[:, :, 0]))
        w = mu * (1.0 - mu)
        return np.matmul((y[None, :] - mu)[:, None, :], Xt)[:, 0], np.matmul(Xt.transpose(0, 2, 1) * w[:, None, :], Xt)


def _logit_solve(H, U):
    """H [V, p, p], U [V, p] -> (delta [V, p], hinv [V], ok [V]): delta = H^-1 U by a Cholesky factorisation in the order
    of the columns, hinv = (H^-1) of the last column = 1 / its pivot, ok: every pivot was above LOGIT_PIVOT_TOL times its
    diagonal entry of H (a NaN is not)"""
    V, p = U.shape
    A, L, u = H.copy(), np.zeros_like(H), U.copy()
    ok = np.ones(V, dtype=bool)
    z, delta = np.zeros_like(U), np.zeros_like(U)
    with np.errstate(all="ignore"):
        for k in range(p):
            d = A[:, k, k]
            ok &= d > LOGIT_PIVOT_TOL * H[:, k, k]
            L[:, k:, k] = A[:, k:, k] / np.sqrt(d)[:, None]
            A[:, k + 1:, k + 1:] -= L[:, k + 1:, k, None] * L[:, None, k + 1:, k]
        for k in range(p):
            z[:, k] = u[:, k] / L[:, k, k]
            u[:, k + 1:] -= L[:, k + 1:, k] * z[:, k, None]
        for i in range(p - 1, -1, -1):
            delta[:, i] = z[:, i] / L[:, i, i]
            z[:, :i] -= L[:, i, :i] * delta[:, i, None]
        return delta, 1.0 / (L[:, -1, -1] * L[:, -1, -1]), ok


def logistic_design(y, covariates=None):
    """the design of a case / control scan -> (X, beta0), host numpy, float64: y is [n], every value 0 or 1 and both
    present, covariates [n, q0] or None (numpy or torch).  X = sqrt(n) Q, [n, q], Q the orthonormal basis of
    [1 | covariates] from numpy.linalg.qr (q = 1 + q0): X^T X = n I whatever the covariates' units, and the dosage's
    coefficient does not depend on the basis.  beta0 [q] is the fit of y on X alone, by the Newton iteration of
    logistic_fit_reference run until max |delta| <= 1e-12, 50 steps at most.  ValueError for a value that is not finite or
    not 0 / 1, one class only, covariates of another row count, a rank-deficient [1 | covariates] (assoc_design's rule),
    n - q - 1 < 1, q > LOGIT_MAX_COLS - 1 (hhgt_logistic_fit's tile), and a null fit that does not get there (the
    covariates separate the classes)."""
    yv = _host_f64(y, "y")
    if yv.ndim != 1:
        raise ValueError(f"logistic_design: y of shape {yv.shape} ([n]: one phenotype)")
    if not ((yv == 0.0) | (yv == 1.0)).all():
        raise ValueError("logistic_design: y holds a value that is neither 0 nor 1")
    n = len(yv)
    if not 0 < yv.sum() < n:
        raise ValueError("logistic_design: y holds one class only (cases and controls are both needed)")
    A = np.ones((n, 1))
    if covariates is not None:
        cov = _host_f64(covariates, "covariates")
        if cov.ndim != 2 or cov.shape[0] != n:
            raise ValueError(f"logistic_design: covariates of shape {cov.shape} for {n} rows of y ([n, q0])")
        A = np.concatenate([A, cov], axis=1)
    q = A.shape[1]
    if q > LOGIT_MAX_COLS - 1:
        raise ValueError(f"logistic_design: {q} covariate columns and the variant exceed {LOGIT_MAX_COLS} columns")
    if n - q - 1 < 1:
        raise ValueError(f"logistic_design: {n} samples leave no degree of freedom beside {q} covariate columns and the variant")
    Q, R = np.linalg.qr(A)
    d = np.abs(np.diag(R))
    if d.min() < n * np.finfo(np.float64).eps * d.max():
        raise ValueError("logistic_design: [1 | covariates] is rank-deficient")
    X = math.sqrt(n) * Q
    theta = np.zeros((1, q))
    for _ in range(50):
        delta, _, ok = _logit_solve(*_logit_evaluate(X[None], yv, theta)[::-1])
        if not ok[0] or not np.isfinite(delta).all():
            break
        theta += delta
        if np.abs(delta).max() <= 1e-12:
            return X, theta[0]
    raise ValueError("logistic_design: the fit of y on the covariates alone does not converge (they separate the classes)")


def logistic_fit_reference(dosage, X, y, beta0):
    """the per-variant logistic fit, in plain numpy: the contract of hhgt_logistic_fit.  dosage is float [V, n] (or [n]: one
    variant), 0, 1 or 2 for a complete call and NaN for one that is not; X [n, q], y [n], beta0 [q] as logistic_design gives
    them -> the record, float64 [V, LOGIT_REC] (or [LOGIT_REC]), columns REC_*.  A call that is not complete takes the mean
    (h + 2 a) / m of the complete ones.  theta = (beta0, 0); one evaluation at theta: eta = [X | g] theta,
    mu = 1 / (1 + exp(-eta)), w = mu (1 - mu), U = [X | g]^T (y - mu), H = [X | g]^T diag(w) [X | g], delta = H^-1 U by
    Cholesky, the dosage last; a pivot not above 1e-12 times its diagonal entry of H fails the evaluation.  The first
    evaluation gives REC_U0 (the dosage's entry of U) and REC_HINV0 = (H^-1)_gg: the score test.  A step is theta += delta
    and a new evaluation; the steps end after the first one with max |delta_j| <= 1e-8 — the evaluation after it gives
    REC_HINV and takes no step, so a fit that takes a step more or fewer by another route differs at second order only —
    or after LOGIT_MAX_STEPS.  Status: LOGIT_NO_CALL without a complete call, LOGIT_ONE_CLASS with fewer than two of
    HOM_REF, HET, HOM_ALT (assoc_from_sums' rule), LOGIT_COLLINEAR when the first evaluation fails — four NaNs each —,
    LOGIT_NOT_CONVERGED when a later one fails (a NaN or an infinity fails one) or step LOGIT_MAX_STEPS is still above
    1e-8: separation, REC_GAMMA and REC_HINV NaN (Firth's correction is not made).  ValueError for a dosage outside
    0, 1, 2, NaN or shapes that disagree."""
    D = np.asarray(dosage, dtype=np.float64)
    single = D.ndim == 1
    D = D.reshape(1, -1) if single else D
    X, y, beta0 = (np.asarray(t, dtype=np.float64) for t in (X, y, beta0))
    n, q = X.shape
    if D.ndim != 2 or D.shape[1] != n or y.shape != (n,) or beta0.shape != (q,):
        raise ValueError(f"logistic_fit_reference: dosage {D.shape}, X {X.shape}, y {y.shape}, beta0 {beta0.shape}")
    comp = ~np.isnan(D)
    if not (~comp | (D == 0.0) | (D == 1.0) | (D == 2.0)).all():
        raise ValueError("logistic_fit_reference: a dosage that is not 0, 1, 2 or NaN")
    V = D.shape[0]
    m, h, a = comp.sum(1), (D == 1.0).sum(1), (D == 2.0).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (h + 2.0 * a) / m
    g = np.where(comp, D, mean[:, None])
    rec = np.full((V, LOGIT_REC), np.nan)
    rec[:, REC_COMPLETE], rec[:, REC_HET], rec[:, REC_ALT], rec[:, REC_STEPS] = m, h, a, 0.0
    classes = (m - h - a > 0).astype(int) + (h > 0) + (a > 0)
    status = np.where(m == 0, LOGIT_NO_CALL, np.where(classes < 2, LOGIT_ONE_CLASS, LOGIT_TESTED))
    run = np.flatnonzero(status == LOGIT_TESTED)                      # the variants still fitted
    theta = np.concatenate([np.broadcast_to(beta0, (V, q)), np.zeros((V, 1))], axis=1)
    steps = np.zeros(V, dtype=np.int64)
    last = np.zeros(V, dtype=bool)
    for ev in range(LOGIT_MAX_STEPS + 1):
        if not len(run):
            break
        Xt = np.concatenate([np.broadcast_to(X, (len(run), n, q)), g[run][:, :, None]], axis=2)
        U, H = _logit_evaluate(Xt, y, theta[run])
        delta, hinv, ok = _logit_solve(H, U)
        if ev == 0:
            status[run[~ok]] = LOGIT_COLLINEAR
            rec[run[ok], REC_U0], rec[run[ok], REC_HINV0] = U[ok, -1], hinv[ok]
        else:
            status[run[~ok]] = LOGIT_NOT_CONVERGED
        done = last[run] & ok
        rec[run[done], REC_HINV] = hinv[done]
        step = ok & ~done
        with np.errstate(invalid="ignore", over="ignore"):
            theta[run[step]] += delta[step]
            biggest = np.abs(np.nan_to_num(delta, nan=np.inf)).max(axis=1)
        steps[run[step]] += 1
        last[run[step & (biggest <= LOGIT_STEP_TOL)]] = True
        lost = step & ~(biggest <= LOGIT_STEP_TOL) & ((steps[run] == LOGIT_MAX_STEPS) | ~np.isfinite(biggest))
        status[run[lost]] = LOGIT_NOT_CONVERGED
        run = run[step & ~lost]
    tested = status == LOGIT_TESTED
    rec[:, REC_GAMMA] = np.where(tested, theta[:, -1], np.nan)
    rec[~tested, REC_HINV] = np.nan
    rec[:, REC_STEPS], rec[:, REC_STATUS] = steps, status
    return rec[0] if single else rec


def logistic_from_fit(raw):
    """the statistics of a case / control scan from the records of hhgt_logistic_fit or logistic_fit_reference ->
    (stats, calls, info): raw float64 [V, LOGIT_REC] (numpy or torch).  stats is float64 [V, 6]: LOGIT_BETA the log odds
    ratio per ALT allele, LOGIT_SE = sqrt((H^-1)_gg) at the fitted model, LOGIT_Z = BETA / SE, LOGIT_P =
    normal_two_sided(Z) (the Wald test), LOGIT_SCORE_CHI2 = U^2 (H^-1)_gg at the null model and LOGIT_SCORE_P =
    normal_two_sided(sqrt(CHI2)) (the score test, one degree of freedom) — all six NaN where the status is not LOGIT_TESTED.
    calls is int64 [V, 3]: complete, HET, HOM_ALT calls, as assoc_from_sums gives them; info int64 [V, 2]: steps, status."""
    i64, f64, _, nan_unless = _ops(raw)
    stack = _math(raw)[4]
    raw = f64(raw)
    if len(raw.shape) != 2 or raw.shape[1] != LOGIT_REC:
        raise ValueError(f"logistic_from_fit: records of shape {list(raw.shape)} ([V, {LOGIT_REC}])")
    calls = stack([i64(raw[:, REC_COMPLETE]), i64(raw[:, REC_HET]), i64(raw[:, REC_ALT])], -1)
    info = stack([i64(raw[:, REC_STEPS]), i64(raw[:, REC_STATUS])], -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        beta, se = raw[:, REC_GAMMA], raw[:, REC_HINV] ** 0.5
        z = beta / se
        chi2 = raw[:, REC_U0] * raw[:, REC_U0] * raw[:, REC_HINV0]
        stats = stack([beta, se, z, normal_two_sided(z), chi2, normal_two_sided(chi2 ** 0.5)], -1)
    return nan_unless((info[:, 1] == LOGIT_TESTED)[:, None], stats), calls, info


def logistic_score_design(X, y, beta0):
    """what the score test by sums needs of a design -> (W, XWX), host numpy, float64: with mu0 = 1 / (1 + exp(-X beta0))
    and w0 = mu0 (1 - mu0), W = [1 | y - mu0 | w0 | w0 X], [n, 3 + q], the per-sample matrix for assoc_sums, and
    XWX = X^T diag(w0) X, [q, q]"""
    X, y, beta0 = (np.asarray(t, dtype=np.float64) for t in (X, y, beta0))
    mu = 1.0 / (1.0 + np.exp(-(X @ beta0)))
    w = mu * (1.0 - mu)
    return np.concatenate([np.ones((len(y), 1)), (y - mu)[:, None], w[:, None], w[:, None] * X], axis=1), X.T @ (w[:, None] * X)


def logistic_score_from_sums(T, W_total, q, XWX):
    """the score test of a case / control scan at the null model from the sums of GenotypeStore.assoc_sums, without a fit
    -> (stats, calls, info) as logistic_from_fit gives them, the four Wald columns NaN and steps 0: T float64
    [V, 3, 3 + q] over logistic_score_design's W = [1 | y - mu0 | w0 | w0 X], W_total [3 + q] the column sums of W, XWX
    [q, q] (numpy or torch, all of one kind).  With m, h, a and the imputed mean mu as in assoc_from_sums and
    g.c = T[HET][c] + 2 T[ALT][c] + mu (W_total[c] - T[COMPLETE][c]) for a column c of W:
        U = g.(y - mu0)      b = g.(w0 X)      gWg = T[HET][w0] + 4 T[ALT][w0] + mu^2 (W_total[w0] - T[COMPLETE][w0])
        V = gWg - b XWX^-1 b^T      LOGIT_SCORE_CHI2 = U^2 / V      LOGIT_SCORE_P = normal_two_sided(sqrt(CHI2))
    — the first evaluation of logistic_fit_reference by another route: V is the pivot of the dosage there.  Status
    LOGIT_NO_CALL and LOGIT_ONE_CLASS as there, LOGIT_COLLINEAR where V <= 1e-12 gWg, LOGIT_TESTED else; never
    LOGIT_NOT_CONVERGED: a variant that separates the classes has a score test."""
    i64, f64, _, nan_unless = _ops(T)
    stack = _math(T)[4]
    q = int(q)
    T, W_total, XWX = f64(T), f64(W_total), f64(XWX)
    if len(T.shape) != 3 or T.shape[1] != 3 or T.shape[2] != 3 + q or tuple(XWX.shape) != (q, q):
        raise ValueError(f"logistic_score_from_sums: T {list(T.shape)} ([V, 3, {3 + q}]), XWX {list(XWX.shape)} ([{q}, {q}])")
    m, h, a = T[:, ASSOC_COMPLETE, 0], T[:, ASSOC_HET, 0], T[:, ASSOC_ALT, 0]
    calls = stack([i64(m), i64(h), i64(a)], -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = (h + 2.0 * a) / m
        gw = T[:, ASSOC_HET] + 2.0 * T[:, ASSOC_ALT] + mu[:, None] * (W_total[None, :] - T[:, ASSOC_COMPLETE])
        gWg = T[:, ASSOC_HET, 2] + 4.0 * T[:, ASSOC_ALT, 2] + mu * mu * (W_total[2] - T[:, ASSOC_COMPLETE, 2])
        b = gw[:, 3:]
        if _is_torch(T):
            import torch
            sol = torch.linalg.solve(XWX, b.T).T
        else:
            sol = np.linalg.solve(XWX, b.T).T
        Vg = gWg - (b * sol).sum(-1)
        chi2 = gw[:, 1] * gw[:, 1] / Vg
        classes = i64(m - h - a > 0) + i64(h > 0) + i64(a > 0)
        status = (i64(m == 0) * LOGIT_NO_CALL + i64((m > 0) & (classes < 2)) * LOGIT_ONE_CLASS
                  + i64((m > 0) & (classes >= 2) & ~(Vg > LOGIT_PIVOT_TOL * gWg)) * LOGIT_COLLINEAR)
        nan = chi2 * 0.0 + float("nan")
        stats = stack([nan, nan, nan, nan, chi2, normal_two_sided(chi2 ** 0.5)], -1)
    return nan_unless((status == LOGIT_TESTED)[:, None], stats), calls, stack([status * 0, status], -1)


# ---- region burden scores: the rare variants of a gene collapsed into one per-sample number -------------------------------------
def burden_class_weights(weights, counts, impute="mean"):
    """the per-class weights of a burden score -> (Wd float64 [3, V, K], o float64 [V, K], used bool [V]): weights is [V, K]
    (or [V]: K = 1), the weight per ALT allele of every variant in each of K scores, counts the allele count table [V, 4] of
    the frequency samples (numpy or torch, both of one kind).  Wd and used are score_class_weights'; o is its offset before
    the sum over the variants: with impute = "mean", o[v] = 2 p_v weights[v] at a used variant (AN > 0; p = AC / AN) and 0
    at the others, so that (the sum of Wd over a sample's complete calls of a region) + (the sum of o over the region) is
    the sum over the region's used variants of weight x (the dosage, or 2p where the call is not complete); with "none",
    Wd[d] = d weights and o = 0.  The counted alleles are ALT alleles: nothing is flipped to the minor one."""
    Wd, _, used = score_class_weights(weights, counts, impute)
    return Wd, 0.0 - Wd[0], used


def region_totals(o, regions):
    """the sums of a per-variant table over regions -> float64 [R, K]: o is [V, K] (numpy or torch), regions int64 [R, 2],
    host, variant intervals [lo, hi) — in any order, overlapping or empty; clipped to [0, V).  A segmented sum without a
    loop over the regions: the difference of two entries of the running sum of o down the variants, so a region's total
    carries the rounding of the prefix before it: its error is bounded by about V 2^-53 times the sum of |o| over the
    variants before the region's end, and the same input gives the same bits."""
    f64 = _ops(o)[1]
    o = f64(o)
    V = int(o.shape[0])
    regions = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    lo = np.clip(regions[:, 0], 0, V)
    hi = np.maximum(np.clip(regions[:, 1], 0, V), lo)
    if _is_torch(o):
        import torch
        running = torch.cat([torch.zeros_like(o[:1]), torch.cumsum(o, 0)])
        lo, hi = torch.from_numpy(lo).to(o.device), torch.from_numpy(hi).to(o.device)
    else:
        running = np.concatenate([np.zeros_like(o[:1]), np.cumsum(o, axis=0)])
    return running[hi] - running[lo]


def beta_density_weights(counts):
    """SKAT's Beta(1, 25) density at the minor allele frequency of every variant of an allele count table [V, 4] (numpy or
    torch) -> float64 [V]: 25 (1 - maf)^24, maf = min(p, 1 - p), p = AC / AN; 0 where AN == 0.  The weight goes with the
    ALT allele whichever allele is the minor one."""
    i64, f64, minimum, _ = _ops(counts)
    t = i64(counts)
    an, ac = t[:, AN], t[:, AC]
    used = an > 0
    p = f64(ac * used) / f64(an * used + (~used) * 1)
    return 25.0 * (1.0 - minimum(p, 1.0 - p)) ** 24 * f64(used)


def dense_assoc(B, W, q, yy):
    """the tail of assoc_from_sums for real-valued columns: the linear regression of every phenotype on [1 | covariates |
    g] for each column g = B[:, r] of B float64 [n, R] — burden scores, one row per sample of assoc_design's W = [1 | Q |
    Yr] [n, 1 + q + P]; yy [P] (numpy or torch, all of one kind) -> float64 [R, P, 4], columns ASSOC_BETA, ASSOC_SE, ASSOC_T,
    ASSOC_P.  With g.w_c = B^T W and g.g = the column sums of B^2,
        D = g.g - sum_j (g.Q_j)^2      U_p = g.Yr_p      beta = U / D      rss = yy - U^2 / D      df = n - q - 1
        se = sqrt(rss / df / D)        t = beta / se     p = student_t_two_sided(t, df)
    exactly as there.  All four are NaN where D <= 1e-12 g.g: a constant column, or one in the covariates' span."""
    _, f64, _, nan_unless = _ops(B)
    stack = _math(B)[4]
    q = int(q)
    B, W, yy = f64(B), f64(W), f64(yy)
    if len(B.shape) != 2 or len(W.shape) != 2 or B.shape[0] != W.shape[0] or W.shape[1] != 1 + q + yy.shape[0]:
        raise ValueError(f"dense_assoc: B {list(B.shape)} ([n, R]), W {list(W.shape)} ([n, 1 + {q} + P]), yy {list(yy.shape)} ([P])")
    n = B.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        gw = B.T @ W
        gg = (B * B).sum(0)
        D = gg - (gw[:, 1:1 + q] * gw[:, 1:1 + q]).sum(-1)
        U = gw[:, 1 + q:]
        df = n - q - 1
        beta = U / D[:, None]
        rss = yy[None, :] - U * U / D[:, None]
        se = (rss / df / D[:, None]) ** 0.5
        t = beta / se
        stats = stack([beta, se, t, student_t_two_sided(t, float(df))], -1)
        return nan_unless((D > 1e-12 * gg)[:, None, None], stats)


def dense_logistic_score(B, W, q, XWX):
    """the score test of logistic_score_from_sums for real-valued columns -> float64 [R, 2], columns the statistic and its
    p-value (LOGIT_SCORE_CHI2, LOGIT_SCORE_P of the scan's table): B float64 [n, R], one row per sample of
    logistic_score_design's W = [1 | y - mu0 | w0 | w0 X] [n, 3 + q], XWX [q, q] (numpy or torch, all of one kind).  For a
    column g of B:
        U = g.(y - mu0)      b = g.(w0 X)      gWg = sum w0 g^2      V = gWg - b XWX^-1 b^T
        chi2 = U^2 / V       p = normal_two_sided(sqrt(chi2))
    — the first evaluation of logistic_fit_reference with g as the dosage.  Both NaN where V <= 1e-12 gWg: a constant
    column, or one in the span of X under the null weights.  No fit is made: there is no Wald test of a burden column."""
    _, f64, _, nan_unless = _ops(B)
    stack = _math(B)[4]
    q = int(q)
    B, W, XWX = f64(B), f64(W), f64(XWX)
    if len(B.shape) != 2 or len(W.shape) != 2 or B.shape[0] != W.shape[0] or W.shape[1] != 3 + q or tuple(XWX.shape) != (q, q):
        raise ValueError(f"dense_logistic_score: B {list(B.shape)} ([n, R]), W {list(W.shape)} ([n, {3 + q}]), XWX {list(XWX.shape)} ([{q}, {q}])")
    with np.errstate(divide="ignore", invalid="ignore"):
        gw = B.T @ W
        gWg = (B * B).T @ W[:, 2]
        b = gw[:, 3:]
        if _is_torch(B):
            import torch
            sol = torch.linalg.solve(XWX, b.T).T
        else:
            sol = np.linalg.solve(XWX, b.T).T
        Vg = gWg - (b * sol).sum(-1)
        chi2 = gw[:, 1] * gw[:, 1] / Vg
        stats = stack([chi2, normal_two_sided(chi2 ** 0.5)], -1)
        return nan_unless((Vg > 1e-12 * gWg)[:, None], stats)


# ---- the mixed-model scan: y = X alpha + g beta + u + e, Var(u) = sg2 K, variance components fixed at the null model -----------
# columns of the statistics table of mixed_from_forms (and store_mixed.assoc_mixed), per variant and phenotype
MIXED_BETA, MIXED_SE, MIXED_Z, MIXED_P = 0, 1, 2, 3
# the grid of the null model's search for h2: k / MIXED_GRID, k = 0 .. MIXED_GRID - 1, and the golden-section steps after it
MIXED_GRID, MIXED_STEPS = 100, 60


def _reml_profile(lam, Xt, yt, h2):
    """the REML log-likelihood of h2, profiled over sigma2 and up to a constant, in the eigenbasis of K -> (value, sigma2):
    lam [n] the eigenvalues, Xt = U^T X, yt = U^T y.  With d = h2 lam + (1 - h2), P = D^-1 - D^-1 Xt (Xt^T D^-1 Xt)^-1 Xt^T D^-1
    and sigma2 = yt^T P yt / (n - q):  -1/2 ((n - q) log sigma2 + sum log d + log det (Xt^T D^-1 Xt))"""
    n, q = Xt.shape
    d = h2 * lam + (1.0 - h2)
    Xd = Xt / d[:, None]
    XdX = Xt.T @ Xd
    b = np.linalg.solve(XdX, Xd.T @ yt)
    sigma2 = float(yt @ (yt / d) - (Xd.T @ yt) @ b) / (n - q)
    return -0.5 * ((n - q) * math.log(sigma2) + float(np.log(d).sum()) + float(np.linalg.slogdet(XdX)[1])), sigma2


def mixed_null(K, y, covariates=None):
    """the null model of a mixed-model association scan, y = X alpha + u + e with Var(u) = sg2 K and Var(e) = se2 I, fitted
    by REML (EMMAX's and GCTA --mlma's approach: the variance components are estimated once, without a variant, and held
    fixed in the scan) -> dict(h2, sigma2, M, My, q), host float64.  K is the relationship matrix [n, n] (numpy or torch;
    grm_from_sums), y [n], covariates [n, q0] or None; X = [1 | covariates], q = 1 + q0 columns, checked as assoc_design
    checks them.  numpy.linalg.eigh(K), its negative eigenvalues set to 0; the profile likelihood (_reml_profile) in
    h2 = sg2 / (sg2 + se2) is evaluated at k / 100, k = 0..99, and refined by 60 golden-section steps between the best grid
    point's neighbours (the best point itself where it is the first or the last): a fixed number of evaluations, none
    beyond 0.99, the same answer on every call.  sigma2 is the profiled REML estimate of sg2 + se2 at that h2, and with
    V = sigma2 (h2 K + (1 - h2) I)
        M = V^-1 - V^-1 X (X^T V^-1 X)^-1 X^T V^-1,
    symmetrised as (M + M^T) / 2: M X = 0, and for a variant x the generalised least-squares estimate of its effect is
    x^T M y / x^T M x with variance 1 / x^T M x (mixed_from_forms).  My = M y.  ValueError for a K that is not [n, n], holds
    a value that is not finite (a pair of samples without a jointly complete variant is NaN in grm_from_sums) or is not
    symmetric to 1e-8 of its largest magnitude, a y that is not [n], and what assoc_design refuses."""
    K = K.detach().cpu().numpy() if _is_torch(K) else K
    K = np.asarray(K, dtype=np.float64)
    yv = _host_f64(y, "y")
    if yv.ndim != 1:
        raise ValueError(f"mixed_null: y of shape {yv.shape} ([n]: one phenotype)")
    n = len(yv)
    if K.shape != (n, n):
        raise ValueError(f"mixed_null: a relationship matrix of shape {K.shape} for {n} samples ([n, n])")
    bad = int((~np.isfinite(K[np.triu_indices(n)])).sum())
    if bad:
        raise ValueError(f"mixed_null: {bad} pair(s) of samples have no finite relationship (no jointly complete variant?)")
    if np.abs(K - K.T).max() > 1e-8 * max(np.abs(K).max(), 1e-300):
        raise ValueError("mixed_null: the relationship matrix is not symmetric")
    X = assoc_design(yv, covariates)[0][:, :1]                          # (the checks; X itself is rebuilt: W holds Q, not X)
    if covariates is not None:
        X = np.concatenate([X, _host_f64(covariates, "covariates")], axis=1)
    q = X.shape[1]
    lam, U = np.linalg.eigh((K + K.T) / 2.0)
    lam = np.maximum(lam, 0.0)
    Xt, yt = U.T @ X, U.T @ yv
    f = lambda h2: _reml_profile(lam, Xt, yt, h2)[0]
    grid = [f(k / MIXED_GRID) for k in range(MIXED_GRID)]
    best = int(np.argmax(grid))
    lo, hi = max(best - 1, 0) / MIXED_GRID, min(best + 1, MIXED_GRID - 1) / MIXED_GRID
    g = (math.sqrt(5.0) - 1.0) / 2.0
    a, b = hi - g * (hi - lo), lo + g * (hi - lo)
    fa, fb = f(a), f(b)
    for _ in range(MIXED_STEPS):
        if fa >= fb:
            hi, b, fb = b, a, fa
            a = hi - g * (hi - lo)
            fa = f(a)
        else:
            lo, a, fa = a, b, fb
            b = lo + g * (hi - lo)
            fb = f(b)
    h2 = 0.5 * (lo + hi)
    if grid[best] >= f(h2):                                           # (a flat or ragged likelihood: the grid point stands)
        h2 = best / MIXED_GRID
    sigma2 = _reml_profile(lam, Xt, yt, h2)[1]
    d = sigma2 * (h2 * lam + (1.0 - h2))
    Vinv = (U / d[None, :]) @ U.T
    VX = Vinv @ X
    M = Vinv - VX @ np.linalg.solve(X.T @ VX, VX.T)
    M = (M + M.T) / 2.0
    return dict(h2=float(h2), sigma2=float(sigma2), M=M, My=M @ yv, q=q)


def mixed_coefficients(T):
    """the coefficients that make hhgt_quad_forms' x the mean-centred dosage -> float64 [V, 3] in kind: T is float64
    [V, 3, C] (numpy or torch), assoc_sums of a W whose column 0 is all ones, so that m, h, a = the complete, HET and
    HOM_ALT calls of column 0 and mu = (h + 2a) / m.  Row v is (1, -mu, 2) — x = HET - mu COMPLETE + 2 HOM_ALT: dosage - mu
    at a complete call, 0 elsewhere —, and (0, 0, 0) for a variant without a complete call."""
    _, f64, _, _ = _ops(T)
    where, stack = _math(T)[3:5]
    T = f64(T)
    m, h, a = T[:, ASSOC_COMPLETE, 0], T[:, ASSOC_HET, 0], T[:, ASSOC_ALT, 0]
    some = m > 0
    one = f64(some)
    mu = (h + 2.0 * a) / where(some, m, m * 0.0 + 1.0)
    return stack([one, -mu * one, 2.0 * one], -1)


def mixed_from_forms(T, q, trace_m_over_n):
    """the statistics of a mixed-model scan from the sums and the quadratic forms of store_mixed.mixed_sums ->
    (stats, calls): T float64 [V, 3, 2], assoc_sums of W = [1 | My] (planes ASSOC_HET, ASSOC_COMPLETE, ASSOC_ALT; My of
    mixed_null), q float64 [V] = x^T M x for x of mixed_coefficients (numpy or torch, both of one kind), trace_m_over_n the
    number trace(M) / n.  calls is int64 [V, 3]: the complete, HET and HOM_ALT calls (column 0 of T: exact).  With m, h, a
    those counts and mu = (h + 2a) / m — a call that is not complete is imputed to the mean, and M 1 = 0 —,
        U = T[HET][1] + 2 T[ALT][1] - mu T[COMPLETE][1] = x^T M y
        beta = U / q      se = q^-1/2      z = U / sqrt(q)      p = normal_two_sided(z)
    (z^2 is the chi-square on 1 df that GCTA --mlma reports).  stats is float64 [V, 4], columns MIXED_BETA, MIXED_SE, MIXED_Z,
    MIXED_P; all four are NaN unless m > 0, at least two of the three complete classes (HOM_REF, HET, HOM_ALT) are
    non-empty and q > 1e-12 (h + 4a - mu^2 m) trace(M) / n — x^T x times the mean eigenvalue of M: below it the covariates
    explain the dosage.  The formulas are the contract: GCTA's .mlma file is not."""
    i64, f64, _, nan_unless = _ops(T)
    stack = _math(T)[4]
    T, q = f64(T), f64(q)
    if len(T.shape) != 3 or tuple(T.shape[1:]) != (3, 2) or tuple(q.shape) != (T.shape[0],):
        raise ValueError(f"mixed_from_forms: T {list(T.shape)} ([V, 3, 2]), q {list(q.shape)} ([V])")
    m, h, a = T[:, ASSOC_COMPLETE, 0], T[:, ASSOC_HET, 0], T[:, ASSOC_ALT, 0]
    calls = stack([i64(m), i64(h), i64(a)], -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = (h + 2.0 * a) / m
        U = T[:, ASSOC_HET, 1] + 2.0 * T[:, ASSOC_ALT, 1] - mu * T[:, ASSOC_COMPLETE, 1]
        xx = h + 4.0 * a - mu * mu * m
        classes = i64(m - h - a > 0) + i64(h > 0) + i64(a > 0)
        tested = (m > 0) & (classes >= 2) & (q > 1e-12 * xx * float(trace_m_over_n))
        root = q ** 0.5
        z = U / root
        stats = stack([U / q, 1.0 / root, z, normal_two_sided(z)], -1)
        return nan_unless(tested[:, None], stats), calls


def mixed_reference(dosage, complete, M, y):
    """the quantities of a mixed-model scan in plain dense numpy, the reference of the device route -> dict(x, q, U, stats,
    calls): dosage is an integer array [n, V] (0, 1, 2: ALT alleles; ignored where the call is not complete), complete bool
    [n, V], M [n, n] and y [n] as in mixed_null.  x float64 [n, V] is dosage - mu at a complete call (mu the variant's mean
    over them) and 0 elsewhere, q = x^T M x, U = x^T (M y) per variant, and stats [V, 4], calls [V, 3] are
    mixed_from_forms' of them."""
    complete = np.asarray(complete, bool)
    d = np.where(complete, np.asarray(dosage), 0).astype(np.float64)
    M, y = np.asarray(M, np.float64), np.asarray(y, np.float64)
    m, h, a = complete.sum(0).astype(np.float64), (d == 1).sum(0).astype(np.float64), (d == 2).sum(0).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = np.where(m > 0, (h + 2.0 * a) / m, 0.0)
    x = np.where(complete, d - mu[None, :], 0.0)
    My = M @ y
    q = ((M @ x) * x).sum(0)
    T = np.zeros((x.shape[1], 3, 2))
    T[:, ASSOC_HET, 0], T[:, ASSOC_COMPLETE, 0], T[:, ASSOC_ALT, 0] = h, m, a
    T[:, ASSOC_HET, 1], T[:, ASSOC_COMPLETE, 1], T[:, ASSOC_ALT, 1] = (d == 1).T @ My, complete.T @ My, (d == 2).T @ My
    stats, calls = mixed_from_forms(T, q, np.trace(M) / len(y))
    return dict(x=x, q=q, U=x.T @ My, stats=stats, calls=calls)


def loco_sums(sums_by_group, nsnp_by_group, group):
    """leave one chromosome out: grm_sums is additive over groups, so the relationship matrix without `group` is
    grm_from_sums of the other groups' sums -> (S, N): sums_by_group and nsnp_by_group map every group to its S [n, n] and
    N [n, n] (numpy or torch).  ValueError if `group` is not among them or no other group is left."""
    if group not in sums_by_group or set(sums_by_group) != set(nsnp_by_group):
        raise ValueError(f"loco_sums: group {group!r} of {sorted(sums_by_group)} (sums) and {sorted(nsnp_by_group)} (counts)")
    others = [g for g in sums_by_group if g != group]
    if not others:
        raise ValueError(f"loco_sums: {group!r} is the only group: leaving it out leaves no variant for the relationship matrix")
    S, N = sums_by_group[others[0]], nsnp_by_group[others[0]]
    for g in others[1:]:
        S, N = S + sums_by_group[g], N + nsnp_by_group[g]
    return S, N
