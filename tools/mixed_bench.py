#!/usr/bin/env python3
"""Mixed-model association scan at cohort shape: store_mixed.mixed_sums and assoc_mixed on the input of tools/grm_bench.py (a
2504-sample cohort file with one chr1-sized group, 230 k synthetic variants, converter output in /dev/shm), all samples, 10
covariates and 1 phenotype; the relationship matrix is store.grm over the first 20 000 variants.

Reports, as one JSON line and in profiles/mixed_bench.json: the calls' ms cold (every chunk read from the file and
uploaded) and with every chunk in the read cache; the kernel ms of k_quad_forms (the "assoc" stage of ctx.profile_read() over
mixed_sums minus the same stage over assoc_sums of the same W), its MFMA count and f64 rate; the host ms of
store_stats.mixed_null (one eigendecomposition of 2504 x 2504: measured once); and, alternating with it repetition by
repetition in the same warmed-up process, the torch route on the cached chunks: read_windows of every sample, a float64
matrix X [S, V] of mean-centred dosages (0 where a call is not complete) and (M @ X * X).sum(0) (timed alone as well).
Medians of the runs and every run; the first repetition is printed but kept out of the medians.  Before any time is taken the
two routes' quadratic forms are compared under hhgt_quad_forms' bound, 32 sw 2^-51 |x|^T |M| |x|.  Not timed: building and
converting the cohort, the relationship matrix, the warm-up.
usage: mixed_bench.py [variants] [runs]"""
import os, shutil, sys, tempfile, time
import numpy as np
import torch
from cohort_bench import build_cohort, report, summarize, timed
from haplohyped_varawareml_amd import device as dev
from haplohyped_varawareml_amd.store import GenotypeStore, mixed_null
from haplohyped_varawareml_amd.store_mixed import assoc_mixed, mixed_sums

V = int(sys.argv[1]) if len(sys.argv) > 1 else 230_000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
S, SEED, G = 2504, 1001, "chr_1"
BIG = 1 << 40
COVARIATES = 10
GRM_VARIANTS = 20_000


def torch_route(st, d_M, times=None, with_bound=False):
    """read_windows of every sample (slices of 256), the centred float64 dosages X [S, V], (M @ X * X).sum(0) -> q [V]
    (and |x|^T |M| |x| [V])"""
    X = torch.empty((S, V), dtype=torch.float64, device=d_M.device)
    C = torch.empty((S, V), dtype=torch.bool, device=d_M.device)
    for i in range(0, S, 256):
        x = torch.stack(st.read_windows([(G, s, 0, V) for s in range(i, min(i + 256, S))]))   # [n, V, 2] int8
        a, b = x[..., 0], x[..., 1]
        done = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
        X[i:i + x.shape[0]] = torch.where(done, (a + b).double(), torch.zeros((), dtype=torch.float64, device=d_M.device))
        C[i:i + x.shape[0]] = done
    m = C.sum(0).double()
    mu = X.sum(0) / torch.where(m > 0, m, torch.ones_like(m))
    X = torch.where(C, X - mu[None, :], torch.zeros((), dtype=torch.float64, device=d_M.device))
    del C
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    q = ((d_M @ X) * X).sum(0)
    torch.cuda.synchronize()
    if times is not None:
        times.append((time.perf_counter() - t0) * 1e3)
    if not with_bound:
        return q
    X.abs_()
    return q, ((d_M.abs() @ X) * X).sum(0)


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    ctx = dev.Context(0)
    h5 = build_cohort(ctx, tmp, V, S, SEED)
    ctx.profile(True)
    rng = np.random.default_rng(SEED)
    cov, y = rng.normal(size=(S, COVARIATES)), rng.normal(size=S)
    warm = GenotypeStore(h5, ctx=ctx, cache_bytes=BIG)
    K = warm.grm(G, v_hi=min(GRM_VARIANTS, V)).cpu().numpy()
    t0 = time.perf_counter()
    null = mixed_null(K, y, cov)
    out = dict(samples=S, variants=V, runs=RUNS, covariates=COVARIATES, phenotypes=1, grm_variants=min(GRM_VARIANTS, V),
               mixed_null_host_ms=(time.perf_counter() - t0) * 1e3, h2=null["h2"], sigma2=null["sigma2"])
    W = np.stack([np.ones(S), null["My"]], axis=1)
    d_M, d_W = torch.from_numpy(null["M"]).to(ctx.device), torch.from_numpy(W).to(ctx.device)
    sw = -(-(-(-S // 64) * 64) // 32)

    # correctness first, which is also the warm-up of both routes (code objects loaded, the allocator grown)
    ref, bound = torch_route(warm, d_M, with_bound=True)
    _, got = mixed_sums(warm, G, d_M, d_W)
    ratio = float(((got - ref).abs() / (32 * sw * 2.0 ** -51 * bound).clamp_min(1e-300)).max())
    assert ratio <= 1.0, ratio
    out.update(largest_error_over_bound=ratio)
    del ref, bound, got

    cold = GenotypeStore(h5, ctx=ctx)
    runs = dict(sums_cold_ms=[], sums_cached_ms=[], call_cold_ms=[], call_cached_ms=[], assoc_stage_ms=[], quad_kernel_ms=[],
                torch_cached_ms=[], torch_matmul_ms=[])
    for _ in range(RUNS + 1):
        runs["sums_cold_ms"].append(timed(lambda: mixed_sums(cold, G, d_M, d_W))[1])
        runs["torch_cached_ms"].append(timed(lambda: torch_route(warm, d_M, runs["torch_matmul_ms"]))[1])
        ctx.profile_reset()
        runs["sums_cached_ms"].append(timed(lambda: mixed_sums(warm, G, d_M, d_W))[1])
        both = ctx.profile_read()["assoc"]["ms"]
        ctx.profile_reset()
        warm.assoc_sums(G, d_W)
        torch.cuda.synchronize()
        runs["assoc_stage_ms"].append(both)
        runs["quad_kernel_ms"].append(both - ctx.profile_read()["assoc"]["ms"])
    for _ in range(2):                                  # (a null fit each: the host's seconds, so fewer repetitions)
        runs["call_cold_ms"].append(timed(lambda: assoc_mixed(cold, G, y, K, cov))[1])
        runs["call_cached_ms"].append(timed(lambda: assoc_mixed(warm, G, y, K, cov))[1])
    medians, spreads = summarize(runs)                  # (of every repetition but the first)
    out.update(runs_ms=runs, **medians, **spreads)
    mfma = -(-V // 16) * 64 * sum(min(4 * b + 4, sw) for b in range(-(-sw // 4)))
    out.update(quad_kernel_mfma=mfma, quad_kernel_f64_tflops=mfma * 2048 / (out["quad_kernel_ms"] * 1e-3) / 1e12,
               quad_kernel_vs_torch_matmul=out["quad_kernel_ms"] / out["torch_matmul_ms"],
               sums_cached_vs_torch_cached=out["sums_cached_ms"] / out["torch_cached_ms"])
    warm.close()
    cold.close()
    report("mixed_bench", out)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
