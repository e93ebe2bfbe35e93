#!/usr/bin/env python3
"""LD pruning at cohort shape: GenotypeStore.ld_prune (window 50, r2 0.2) on the input of tools/allele_count_bench.py (a
2504-sample cohort file with one chr1-sized group, 230 k synthetic variants, converter output in /dev/shm), all samples.

Reports, as one JSON line (also written to profiles/ld_bench.json): the call's ms cold (every chunk read from the file and
uploaded) and with every chunk in the read cache, the kernel ms of its five stages (hhgt_genotype_planes under "decode",
hhgt_variant_planes under "ld_transpose", hhgt_ld_counts under "ld", hhgt_ld_prune's decisions under "ld_prune" and its
walk under "ld_walk": ctx.profile_read()), and, alternating with it repetition by repetition in the same warmed-up process,
the torch route on the cached chunks: read_windows of every sample, dosage and completeness matrices [V, S] as fp32, per neighbour distance d the six banded
products (sums over the jointly complete samples; 0 / 1 / 2 / 4 operands and S < 2^24: exact), the same float64 decision,
and the same greedy walk on the host.  Medians of the runs and every run; the first repetition is printed but kept out of
the medians.  The torch mask is asserted equal to ld_prune's before any time is taken.  The synthetic generator's variants
are independent, so nearly every variant is kept: the cost does not depend on that, the kept count is reported.  Not timed:
building and converting the cohort, the warm-up.
usage: ld_bench.py [variants] [runs]"""
import os, shutil, sys, tempfile, time
import numpy as np
import torch
from cohort_bench import build_cohort, report, summarize, timed
from haplohyped_varawareml_amd import device as dev
from haplohyped_varawareml_amd.store import GenotypeStore

V = int(sys.argv[1]) if len(sys.argv) > 1 else 230_000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
S, SEED, G = 2504, 1001, "chr_1"
WINDOW, R2 = 50, 0.2
BIG = 1 << 40


def torch_route(st):
    """read_windows of every sample (slices of 256) -> x (dosage where complete), m (complete) fp32 [V, S]; per distance d
    the sums over the jointly complete samples as row-wise products; the decision in float64; the walk on the host"""
    device = st._context().device
    x = torch.empty((V, S), dtype=torch.float32, device=device)
    m = torch.empty((V, S), dtype=torch.float32, device=device)
    for i in range(0, S, 256):
        g = torch.stack(st.read_windows([(G, s, 0, V) for s in range(i, min(i + 256, S))]))   # [n, V, 2] int8
        a, b = g[..., 0], g[..., 1]
        done = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
        n = g.shape[0]
        m[:, i:i + n] = done.T
        x[:, i:i + n] = (done * (a + b)).T
    xx = x * x
    ex = torch.zeros((V, WINDOW), dtype=torch.bool, device=device)
    for d in range(WINDOW):
        u, v = slice(0, V - 1 - d), slice(1 + d, V)
        s = lambda p, q: (p[u] * q[v]).sum(1).to(torch.int64)
        n, sx, sy, sxx, syy, sxy = s(m, m), s(x, m), s(m, x), s(xx, m), s(m, xx), s(x, x)
        num, dx, dy = (n * sxy - sx * sy).double(), (n * sxx - sx * sx).double(), (n * syy - sy * sy).double()
        ex[u, d] = num * num > R2 * (dx * dy)
    ex = ex.cpu().numpy()
    keep = np.zeros(V, bool)
    for v in range(V):
        lo = max(v - WINDOW, 0)
        us = np.arange(lo, v)
        keep[v] = not (keep[us] & ex[us, v - us - 1]).any()
    return keep


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    ctx = dev.Context(0)
    h5 = build_cohort(ctx, tmp, V, S, SEED)
    ctx.profile(True)
    out = dict(date=time.strftime("%Y-%m-%d"), samples=S, variants=V, window=WINDOW, r2=R2, runs=RUNS)

    # correctness first, which is also the warm-up of both routes (code objects loaded, the allocator grown)
    warm = GenotypeStore(h5, ctx=ctx, cache_bytes=BIG)
    ref = torch_route(warm)
    got = warm.ld_prune(G, window=WINDOW, r2=R2)
    assert np.array_equal(got.cpu().numpy(), ref)
    out.update(same_as_torch=True, kept=int(ref.sum()))
    del ref, got

    cold = GenotypeStore(h5, ctx=ctx)
    stages = dict(planes_kernel_ms="decode", transpose_kernel_ms="ld_transpose", counts_kernel_ms="ld",
                  decide_kernel_ms="ld_prune", walk_kernel_ms="ld_walk")
    runs = dict(call_cold_ms=[], call_cached_ms=[], torch_cached_ms=[], **{k: [] for k in stages})
    for _ in range(RUNS + 1):
        runs["call_cold_ms"].append(timed(lambda: cold.ld_prune(G, window=WINDOW, r2=R2))[1])
        runs["torch_cached_ms"].append(timed(lambda: torch_route(warm))[1])
        ctx.profile_reset()
        warm.stats.update(ld_plane_blocks=0, ld_pairs=0)
        runs["call_cached_ms"].append(timed(lambda: warm.ld_prune(G, window=WINDOW, r2=R2))[1])
        prof = ctx.profile_read()
        for k, stage in stages.items():
            runs[k].append(prof[stage]["ms"])
    medians, spreads = summarize(runs)                  # (of every repetition but the first)
    out.update(runs_ms=runs, **medians, **spreads)
    out.update(plane_blocks_decoded=warm.stats["ld_plane_blocks"], pairs_counted=warm.stats["ld_pairs"],
               call_cached_vs_torch_cached=out["call_cached_ms"] / out["torch_cached_ms"])
    warm.close()
    cold.close()
    report("ld_bench", out)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
