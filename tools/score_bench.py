#!/usr/bin/env python3
"""Per-sample sums of per-variant weights at cohort shape: GenotypeStore.score_sums on the input of tools/grm_bench.py (a
2504-sample cohort file with one chr1-sized group, 230 k synthetic variants, converter output in /dev/shm), all samples,
K = 1, 10 and 64 columns of weights (class weights d * beta: the dosage times a per-allele effect).

Reports, as one JSON line and in profiles/score_bench.json, per K: the call's ms cold (every chunk read from the file and
uploaded) and with every chunk in the read cache; the kernel ms of its stages (ctx.profile_read(): "decode" holds
hhgt_genotype_planes, "assoc" hhgt_score_sums' two launches — a scoring call runs no hhgt_assoc_sums) and hhgt_score_sums'
MFMA count and rate; and, alternating with it repetition by repetition in the same warmed-up process, the torch route on
the cached chunks: read_windows of every sample, a float64 dosage matrix [S, V] (0 where the call is not complete) and one
matmul with the effects (also timed alone).  Medians of the runs and every run; the first repetition is printed but kept
out of the medians.  Before any time is taken the two routes' sums are compared: the largest difference over
V 2^-50 sum |beta| reported and asserted at most 1.  Not timed: building and converting the cohort, the weights' upload,
the warm-up.
usage: score_bench.py [variants] [runs]"""
import os, shutil, sys, tempfile, time
import numpy as np
import torch
from cohort_bench import build_cohort, report, summarize, timed
from haplohyped_varawareml_amd import device as dev
from haplohyped_varawareml_amd.store import GenotypeStore

V = int(sys.argv[1]) if len(sys.argv) > 1 else 230_000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
S, SEED, G = 2504, 1001, "chr_1"
BIG = 1 << 40
COLUMNS = (1, 10, 64)


def torch_route(st, beta, times=None):
    """read_windows of every sample (slices of 256), the float64 dosages [S, V] (0 where the call is not complete), one
    matmul with beta [V, K] -> float64 [S, K]"""
    D = torch.empty((S, V), dtype=torch.float64, device=beta.device)
    for i in range(0, S, 256):
        x = torch.stack(st.read_windows([(G, s, 0, V) for s in range(i, min(i + 256, S))]))   # [n, V, 2] int8
        a, b = x[..., 0], x[..., 1]
        done = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
        D[i:i + x.shape[0]] = torch.where(done, (a + b).double(), torch.zeros((), dtype=torch.float64, device=beta.device))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = D @ beta
    torch.cuda.synchronize()
    if times is not None:
        times.append((time.perf_counter() - t0) * 1e3)
    return out


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    ctx = dev.Context(0)
    h5 = build_cohort(ctx, tmp, V, S, SEED)
    ctx.profile(True)
    rng = np.random.default_rng(SEED)
    out = dict(samples=S, variants=V, runs=RUNS, columns=list(COLUMNS))
    warm, cold = GenotypeStore(h5, ctx=ctx, cache_bytes=BIG), GenotypeStore(h5, ctx=ctx)
    rows, words = -(-S // 64) * 64, -(-V // 4096) * 128         # plane rows; plane words of whole Blosc blocks
    for K in COLUMNS:
        beta = torch.from_numpy(rng.normal(size=(V, K))).to(ctx.device)
        Wd = torch.stack([d * beta for d in (0.0, 1.0, 2.0)])

        # correctness first, which is also the warm-up of both routes (code objects loaded, the allocator grown)
        ref = torch_route(warm, beta)
        got = warm.score_sums(Wd, G)
        ratio = float(((got - ref).abs() / (V * 2.0 ** -50 * beta.abs().sum(0))[None, :]).max())
        assert ratio <= 1.0, ratio
        del ref, got

        runs = dict(call_cold_ms=[], call_cached_ms=[], planes_kernel_ms=[], score_kernel_ms=[], torch_cached_ms=[],
                    torch_matmul_ms=[])
        for _ in range(RUNS + 1):
            runs["call_cold_ms"].append(timed(lambda: cold.score_sums(Wd, G))[1])
            runs["torch_cached_ms"].append(timed(lambda: torch_route(warm, beta, runs["torch_matmul_ms"]))[1])
            ctx.profile_reset()
            warm.stats.update(score_plane_blocks=0, score_variants=0)
            runs["call_cached_ms"].append(timed(lambda: warm.score_sums(Wd, G))[1])
            prof = ctx.profile_read()
            runs["planes_kernel_ms"].append(prof["decode"]["ms"])
            runs["score_kernel_ms"].append(prof["assoc"]["ms"])
        medians, spreads = summarize(runs)                  # (of every repetition but the first)
        mfma = 3 * (rows // 16) * 8 * words * -(-K // 16)
        res = dict(largest_difference_over_tolerance=ratio, runs_ms=runs, **medians, **spreads,
                   plane_blocks_decoded=warm.stats["score_plane_blocks"], score_kernel_mfma=mfma)
        res.update(score_kernel_f64_tflops=mfma * 2048 / (res["score_kernel_ms"] * 1e-3) / 1e12,
                   score_kernel_vs_torch_matmul=res["score_kernel_ms"] / res["torch_matmul_ms"],
                   call_cached_vs_torch_cached=res["call_cached_ms"] / res["torch_cached_ms"])
        out[f"k{K}"] = res
        del beta, Wd
    warm.close()
    cold.close()
    report("score_bench", out)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
