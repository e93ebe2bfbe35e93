"""The mixed-model association scan over a GenotypeStore: y = X alpha + g beta + u + e with Var(u) = sg2 K, K the
relationship matrix, the variance components fixed at the null model (EMMAX, GCTA --mlma).  Functions that take the store as
their first argument, not methods of it; rows from store._variant_rows: cached chunks used, the read cache neither filled
nor evicted."""
import numpy as np

from .store import _table_budget
from .store_stats import ASSOC_MAX_COLS, mixed_coefficients, mixed_from_forms, mixed_null


def mixed_sums(store, group, A, W, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None, plane_bytes=None,
               max_table_bytes=None):
    """the sums and the quadratic forms behind a mixed-model scan of a group -> (T, q) on the device: T float64
    [n_counted, 3, C] is store.assoc_sums(group, W, ...) — same selection arguments, same planes —, and q float64 [n_counted]
    is x^T A x of every counted variant for x = the dosage minus the variant's mean dosage at a complete call and 0
    elsewhere (store_stats.mixed_coefficients of T).  W is float64 [len(samples), C], 1 <= C <= 64, its column 0 all ones
    (checked: the call counts are read from it); A float64 [n, n], host or device, symmetric (checked bit for bit: one
    triangle is read), row and column i for samples[i].  The samples must be distinct: ValueError before anything is
    allocated.  A is scattered once to [32 sw, 32 sw] over the plane rows of the samples, zeros elsewhere — ValueError if
    its bytes exceed max_table_bytes (default 2 GiB) —, and every plane window is reduced by one hhgt_assoc_sums and one
    hhgt_quad_forms call (the f64 MFMA; include/hhgt.h states their arithmetic and error bounds).  No genotype and no dosage
    is written anywhere."""
    import torch
    idx = store._query("mixed_sums", group, samples, v_lo, v_hi, variant_mask, single=True)[0]
    n = len(idx)
    W = W if torch.is_tensor(W) else torch.from_numpy(np.ascontiguousarray(W))
    A = A if torch.is_tensor(A) else torch.from_numpy(np.ascontiguousarray(A))
    if W.dtype != torch.float64 or W.dim() != 2 or W.shape[0] != n or not 1 <= W.shape[1] <= ASSOC_MAX_COLS:
        raise ValueError(f"mixed_sums: W must be float64 [{n}, 1 to {ASSOC_MAX_COLS}], not {W.dtype} {list(W.shape)}")
    if A.dtype != torch.float64 or tuple(A.shape) != (n, n):
        raise ValueError(f"mixed_sums: A must be float64 [{n}, {n}], not {A.dtype} {list(A.shape)}")
    rows, sw, scattered = store._design_rows("mixed_sums", idx)
    _table_budget("mixed_sums", "the matrix over the plane rows needs {} bytes;", 8 * (32 * sw) ** 2, max_table_bytes)
    if not bool((W[:, 0] == 1.0).all()) or not torch.equal(A, A.T):
        raise ValueError("mixed_sums: column 0 of W must be all ones and A symmetric")
    _, _, _, n_counted, vrows = store._variant_rows("mixed_sums", group, idx, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes,
                                                    "assoc_plane_blocks")
    d_w = scattered(W)
    d_A = scattered(scattered(A).T.contiguous())                      # rows, then columns, to the plane rows: A is symmetric
    ctx = store._context()
    Ts, qs = [], []
    for v in vrows:
        T = ctx.assoc_sums(v, d_w)
        Ts.append(T)
        qs.append(ctx.quad_forms(v, mixed_coefficients(T), d_A))
    store.stats["assoc_variants"] += n_counted
    if not Ts:                      # (without a sample there is no row of bits: every sum is 0)
        return (torch.zeros((n_counted, 3, W.shape[1]), dtype=torch.float64, device=d_w.device),
                torch.zeros((n_counted,), dtype=torch.float64, device=d_w.device))
    return torch.cat(Ts), torch.cat(qs)


def assoc_mixed(store, group, y, grm, covariates=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None,
                plane_bytes=None, max_table_bytes=None):
    """mixed-model association scan of a group -> (stats, calls, nulls): y is [n] or [n, P], covariates [n, q0] or None, grm
    the relationship matrix [n, n], host or device (store.grm; leave the scanned group out of it with
    store_stats.loco_sums for a leave-one-chromosome-out scan), all aligned with samples.  Every phenotype gets its own null
    model — store_stats.mixed_null on the host: one eigendecomposition and one n x n matrix M each — and its own pass over
    the planes (mixed_sums of M and W = [1 | M y]): P phenotypes cost P null fits and P passes.  stats is float64
    [n_counted, P, 4] on the device — MIXED_BETA, MIXED_SE, MIXED_Z, MIXED_P of store_stats.mixed_from_forms, NaN where the
    variant is not tested —, calls int64 [n_counted, 3]: complete, HET, HOM_ALT calls; nulls a list of P dicts (h2, sigma2,
    q: mixed_null's without its matrices).  The samples must be distinct: ValueError before anything is allocated, as for
    a grm that is not finite or not symmetric and a design assoc_design refuses."""
    import torch
    idx = store._query("assoc_mixed", group, samples, v_lo, v_hi, variant_mask, single=True)[0]
    if len(np.unique(idx)) != len(idx):
        raise ValueError("assoc_mixed: a sample is listed twice")
    Y = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y, dtype=np.float64)
    Y = Y[:, None] if Y.ndim == 1 else Y
    if Y.ndim != 2 or Y.shape[0] != len(idx):
        raise ValueError(f"assoc_mixed: y of shape {Y.shape} for {len(idx)} samples ([n] or [n, P])")
    K = grm.detach().cpu().numpy() if torch.is_tensor(grm) else np.asarray(grm, dtype=np.float64)
    stats, calls, nulls = [], None, []
    for p in range(Y.shape[1]):
        null = mixed_null(K, Y[:, p], covariates)
        s, calls = scan_under_null(store, group, null, samples, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes, max_table_bytes)
        stats.append(s)
        nulls.append({k: null[k] for k in ("h2", "sigma2", "q")})
    return torch.stack(stats, 1), calls, nulls


def scan_under_null(store, group, null, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None, plane_bytes=None,
                    max_table_bytes=None):
    """one phenotype's scan of a group under a fitted null model (store_stats.mixed_null's dict, aligned with samples) ->
    (stats float64 [n_counted, 4], calls int64 [n_counted, 3]) on the device: mixed_sums of M and W = [1 | M y], then
    store_stats.mixed_from_forms"""
    M, n = null["M"], len(null["My"])
    T, q = mixed_sums(store, group, M, np.stack([np.ones(n), null["My"]], axis=1), samples, v_lo, v_hi, variant_mask, slab_bytes,
                      plane_bytes, max_table_bytes)
    return mixed_from_forms(T, q, float(np.trace(M)) / n)
