#!/usr/bin/env python3
"""Genetic relationship sums at cohort shape: GenotypeStore.grm_sums on the input of tools/pair_count_bench.py (a
2504-sample cohort file with one chr1-sized group, 230 k synthetic variants, converter output in /dev/shm), all samples.

Reports, as one JSON line and in profiles/grm_bench.json: the call's ms cold (every chunk read from the file and uploaded)
and with every chunk in the read cache; the kernel ms of its stages (ctx.profile_read(): "decode" holds hhgt_count_alleles
and hhgt_genotype_planes — the allele count alone is timed beside it and subtracted —, "pairs" hhgt_pair_counts, "grm"
hhgt_grm) and hhgt_grm's fraction of the f32 MFMA peak (155 TFLOP/s measured), counting 2 x (pairs computed, tile padding
included) x bit positions; and, alternating with it repetition by repetition in the same warmed-up process, the torch
route on the cached chunks: the same allele count and z, read_windows of every sample, a float32 Z [S, V], Z @ Z.T (also
timed alone), and the completeness indicator as bf16 multiplied in variant slabs (exact) for N.  Medians of the runs and
every run; the first repetition is printed but kept out of the medians.  Before any time is taken N is asserted equal and
the store's S of the first 256 samples is asserted within the chain bound of a float64 product of the same Z.  Last,
numpy.linalg.eigh of the matrix on the host, once.  Not timed: building and converting the cohort, the warm-up.
usage: grm_bench.py [variants] [runs]"""
import os, shutil, sys, tempfile, time
import numpy as np
import torch
from cohort_bench import build_cohort, report, summarize, timed
from haplohyped_varawareml_amd import device as dev
from haplohyped_varawareml_amd.store import GRM_SPAN, GenotypeStore, grm_from_sums, standardized_dosages

V = int(sys.argv[1]) if len(sys.argv) > 1 else 230_000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
S, SEED, G = 2504, 1001, "chr_1"
BIG = 1 << 40
SLAB = 1 << 16            # variants per product of N: 65 536 < 2^24
PEAK_F32_MFMA = 155e12


def torch_route(st, times=None):
    """allele counts and z, read_windows of every sample (slices of 256), Z and the completeness indicator, Z @ Z.T and
    the indicator's products per variant slab -> (S float32 [S, S], N int32 [S, S], Z)"""
    z, used = standardized_dosages(st.allele_counts(G))
    z = z * used                                                                            # [3, V]
    Z = torch.empty((S, V), dtype=torch.float32, device=z.device)
    M = torch.empty((S, V), dtype=torch.bfloat16, device=z.device)
    for i in range(0, S, 256):
        x = torch.stack(st.read_windows([(G, s, 0, V) for s in range(i, min(i + 256, S))]))   # [n, V, 2] int8
        a, b = x[..., 0], x[..., 1]
        done = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1)) & used
        d = torch.where(done, (a + b).to(torch.int64), torch.zeros((), dtype=torch.int64, device=z.device))
        n = x.shape[0]
        Z[i:i + n] = torch.where(done, torch.gather(z.T, 1, d.T).T, torch.zeros((), device=z.device))
        M[i:i + n] = done
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sums = Z @ Z.T
    torch.cuda.synchronize()
    if times is not None:
        times.append((time.perf_counter() - t0) * 1e3)
    N = torch.zeros((S, S), dtype=torch.int32, device=z.device)
    for v in range(0, V, SLAB):
        m = M[:, v:v + SLAB]
        N += torch.matmul(m, m.T).float().to(torch.int32)
    return sums, N, Z


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    ctx = dev.Context(0)
    h5 = build_cohort(ctx, tmp, V, S, SEED)
    ctx.profile(True)
    out = dict(samples=S, variants=V, runs=RUNS, grm_span=GRM_SPAN)

    # correctness first, which is also the warm-up of both routes (code objects loaded, the allocator grown)
    warm = GenotypeStore(h5, ctx=ctx, cache_bytes=BIG)
    ref_s, ref_n, Z = torch_route(warm)
    got_s, got_n = warm.grm_sums(G)
    assert torch.equal(got_n, ref_n)
    head = Z[:256].double()
    exact, total = head @ head.T, head.abs() @ head.abs().T
    assert bool(((got_s[:256, :256] - exact).abs() <= (32 * GRM_SPAN + 4) * 2.0 ** -24 * total).all())
    out.update(nsnp_same_as_torch=True, nsnp_max=int(got_n.max()),
               store_error_over_bound=float(((got_s[:256, :256] - exact).abs() / ((32 * GRM_SPAN + 4) * 2.0 ** -24 * total)).max()),
               torch_f32_error_over_bound=float(((ref_s[:256, :256].double() - exact).abs()
                                                 / ((32 * GRM_SPAN + 4) * 2.0 ** -24 * total)).max()))
    grm = grm_from_sums(got_s, got_n).cpu().numpy()
    del ref_s, ref_n, Z, head, exact, total, got_s, got_n

    cold = GenotypeStore(h5, ctx=ctx)
    runs = dict(call_cold_ms=[], call_cached_ms=[], decode_kernels_ms=[], count_kernel_ms=[], pairs_kernel_ms=[],
                grm_kernel_ms=[], torch_cached_ms=[], torch_matmul_ms=[])
    for _ in range(RUNS + 1):
        runs["call_cold_ms"].append(timed(lambda: cold.grm_sums(G))[1])
        runs["torch_cached_ms"].append(timed(lambda: torch_route(warm, runs["torch_matmul_ms"]))[1])
        ctx.profile_reset()
        warm.allele_counts(G)
        torch.cuda.synchronize()
        runs["count_kernel_ms"].append(ctx.profile_read()["decode"]["ms"])
        ctx.profile_reset()
        warm.stats.update(grm_plane_blocks=0, grm_words=0)
        runs["call_cached_ms"].append(timed(lambda: warm.grm_sums(G))[1])
        prof = ctx.profile_read()
        runs["decode_kernels_ms"].append(prof["decode"]["ms"])
        runs["pairs_kernel_ms"].append(prof["pairs"]["ms"])
        runs["grm_kernel_ms"].append(prof["grm"]["ms"])
    medians, spreads = summarize(runs)                  # (of every repetition but the first)
    out.update(runs_ms=runs, **medians, **spreads)
    tiles = -(-S // 64)
    flop = 2.0 * (tiles * (tiles + 1) // 2) * 64 * 64 * 32 * warm.stats["grm_words"]
    out.update(planes_kernel_ms=out["decode_kernels_ms"] - out["count_kernel_ms"],
               plane_blocks_decoded=warm.stats["grm_plane_blocks"], plane_words_per_row=warm.stats["grm_words"],
               grm_kernel_flop=flop, grm_kernel_fraction_of_f32_mfma_peak=flop / (out["grm_kernel_ms"] * 1e-3) / PEAK_F32_MFMA,
               grm_kernel_vs_torch_matmul=out["grm_kernel_ms"] / out["torch_matmul_ms"],
               call_cached_vs_torch_cached=out["call_cached_ms"] / out["torch_cached_ms"])
    warm.close()
    cold.close()
    t0 = time.perf_counter()
    w = np.linalg.eigh(grm)[0]
    out.update(host_eigh_ms=(time.perf_counter() - t0) * 1e3, largest_eigenvalue=float(w[-1]))
    report("grm_bench", out)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
