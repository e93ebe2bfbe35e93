#!/usr/bin/env python3
"""Single-variant association scan at cohort shape: GenotypeStore.assoc on the input of tools/grm_bench.py (a 2504-sample
cohort file with one chr1-sized group, 230 k synthetic variants, converter output in /dev/shm), all samples, 10 covariates
and 1 phenotype (13 columns of hhgt_assoc_sums).

Reports, as one JSON line and in profiles/assoc_bench.json: the call's ms cold (every chunk read from the file and uploaded)
and with every chunk in the read cache; the kernel ms of its stages (ctx.profile_read(): "decode" holds
hhgt_genotype_planes, "ld_transpose" hhgt_variant_planes, "assoc" hhgt_assoc_sums) and hhgt_assoc_sums' MFMA count and rate;
and, alternating with it repetition by repetition in the same warmed-up process, the torch route on the cached chunks:
read_windows of every sample, a float64 dosage matrix [V, S] with the calls that are not complete imputed to the variant's
mean, and two matmuls (against Q and against the residual phenotypes; also timed alone), then the same formulas.  Medians of
the runs and every run; the first repetition is printed but kept out of the medians.  Before any time is taken the two
routes' statistics are compared: the same variants tested, the largest relative difference of BETA, SE and T reported and
asserted below 1e-6 (a BETA or T near 0 carries the absolute error of its sum).  Not timed: building and converting the
cohort, the design on the host, the warm-up.
usage: assoc_bench.py [variants] [runs]"""
import os, shutil, sys, tempfile, time
import numpy as np
import torch
from cohort_bench import build_cohort, report, summarize, timed
from haplohyped_varawareml_amd import device as dev
from haplohyped_varawareml_amd.store import ASSOC_P, GenotypeStore, assoc_design, student_t_two_sided

V = int(sys.argv[1]) if len(sys.argv) > 1 else 230_000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
S, SEED, G = 2504, 1001, "chr_1"
BIG = 1 << 40
COVARIATES = 10


def torch_route(st, W, q, yy, times=None):
    """read_windows of every sample (slices of 256), the mean-imputed float64 dosages [V, S], their products with Q and with
    the residual phenotypes, the statistics -> float64 [V, 1, 4]"""
    d_w = torch.from_numpy(W).to(st._context().device)
    D = torch.empty((V, S), dtype=torch.float64, device=d_w.device)
    M = torch.empty((V, S), dtype=torch.bool, device=d_w.device)
    for i in range(0, S, 256):
        x = torch.stack(st.read_windows([(G, s, 0, V) for s in range(i, min(i + 256, S))]))   # [n, V, 2] int8
        a, b = x[..., 0], x[..., 1]
        done = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
        D[:, i:i + x.shape[0]] = torch.where(done, (a + b).double(), torch.zeros((), dtype=torch.float64, device=d_w.device)).T
        M[:, i:i + x.shape[0]] = done.T
    m = M.sum(1).double()
    mu = D.sum(1) / m
    D = torch.where(M, D, mu[:, None])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gq, u = D @ d_w[:, 1:1 + q], D @ d_w[:, 1 + q:]
    torch.cuda.synchronize()
    if times is not None:
        times.append((time.perf_counter() - t0) * 1e3)
    gg = (D * D).sum(1)
    den = gg - (gq * gq).sum(1)
    df = S - q - 1
    beta = u / den[:, None]
    se = ((torch.from_numpy(yy).to(u.device)[None, :] - u * u / den[:, None]) / df / den[:, None]) ** 0.5
    t = beta / se
    classes = ((D == 0) & M).any(1).long() + ((D == 1) & M).any(1).long() + ((D == 2) & M).any(1).long()
    tested = (m > 0) & (classes >= 2) & (den > 1e-12 * gg)
    stats = torch.stack([beta, se, t, student_t_two_sided(t, float(df))], -1)
    return torch.where(tested[:, None, None], stats, torch.full_like(stats, float("nan")))


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    ctx = dev.Context(0)
    h5 = build_cohort(ctx, tmp, V, S, SEED)
    ctx.profile(True)
    rng = np.random.default_rng(SEED)
    cov, y = rng.normal(size=(S, COVARIATES)), rng.normal(size=S)
    W, q, yy = assoc_design(y, cov)
    out = dict(samples=S, variants=V, runs=RUNS, covariates=COVARIATES, phenotypes=1, columns=int(W.shape[1]))

    # correctness first, which is also the warm-up of both routes (code objects loaded, the allocator grown)
    warm = GenotypeStore(h5, ctx=ctx, cache_bytes=BIG)
    ref = torch_route(warm, W, q, yy)
    got, calls = warm.assoc(G, y, cov)
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    ok = ~torch.isnan(ref[..., :3])
    rel = float(((got[..., :3] - ref[..., :3]).abs()[ok] / ref[..., :3].abs()[ok]).max())
    assert rel < 1e-6, rel
    out.update(same_variants_tested=True, variants_tested=int(ok[:, 0, 0].sum()), largest_relative_difference=rel,
               smallest_p=float(got[..., ASSOC_P][ok[..., 0]].min()))
    del ref, got, calls, ok

    cold = GenotypeStore(h5, ctx=ctx)
    runs = dict(call_cold_ms=[], call_cached_ms=[], sums_cached_ms=[], planes_kernel_ms=[], transpose_kernel_ms=[],
                assoc_kernel_ms=[], torch_cached_ms=[], torch_matmul_ms=[])
    for _ in range(RUNS + 1):
        runs["call_cold_ms"].append(timed(lambda: cold.assoc(G, y, cov))[1])
        runs["torch_cached_ms"].append(timed(lambda: torch_route(warm, W, q, yy, runs["torch_matmul_ms"]))[1])
        runs["call_cached_ms"].append(timed(lambda: warm.assoc(G, y, cov))[1])
        ctx.profile_reset()
        warm.stats.update(assoc_plane_blocks=0, assoc_variants=0)
        runs["sums_cached_ms"].append(timed(lambda: warm.assoc_sums(G, W))[1])
        prof = ctx.profile_read()
        runs["planes_kernel_ms"].append(prof["decode"]["ms"])
        runs["transpose_kernel_ms"].append(prof["ld_transpose"]["ms"])
        runs["assoc_kernel_ms"].append(prof["assoc"]["ms"])
    medians, spreads = summarize(runs)                  # (of every repetition but the first)
    out.update(runs_ms=runs, **medians, **spreads)
    sw = -(-(-(-S // 64) * 64) // 32)
    mfma = 3 * -(-V // 16) * 8 * sw * -(-W.shape[1] // 16)
    out.update(plane_blocks_decoded=warm.stats["assoc_plane_blocks"], assoc_kernel_mfma=mfma,
               assoc_kernel_f64_tflops=mfma * 2048 / (out["assoc_kernel_ms"] * 1e-3) / 1e12,
               assoc_kernel_vs_torch_matmul=out["assoc_kernel_ms"] / out["torch_matmul_ms"],
               call_cached_vs_torch_cached=out["call_cached_ms"] / out["torch_cached_ms"])
    warm.close()
    cold.close()
    report("assoc_bench", out)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
