#!/usr/bin/env python3
"""Per-sample genotype counts at cohort shape: GenotypeStore.sample_counts on the input of tools/allele_count_bench.py (a
2504-sample cohort file with one chr1-sized group, 230 k synthetic variants, converter output in /dev/shm), over all
samples and over a random 64-sample subset, unmasked and under a MAF >= 0.05 variant mask.

Reports, as one JSON line, for each of the four cases: the count kernel's ms (k_count_samples, ctx.profile_read()), the
call's ms cold (every chunk read from the file and uploaded) and with every chunk in the read cache (medians of the runs),
Blosc blocks decoded per call; alternating with the calls repetition by repetition, after one warm-up of both paths, the
naive path over all samples (read_windows of every sample over the whole group, then a torch reduction of the int8
matrix), cold (a fresh store) and cached.  Then, alternating in the same process over all samples: k_count_samples,
k_count_alleles on the same selections and k_decode_blocks on the same chunks (kernel ms per repetition, so the spread
and the first, slower, repetition can be seen).  The fused counts are asserted equal to the naive ones before any
time is printed.
usage: sample_count_bench.py [variants] [runs]"""
import os, shutil, sys, tempfile
import numpy as np
import torch
from cohort_bench import build_cohort, report, summarize, timed
from haplohyped_varawareml_amd import device as dev
from haplohyped_varawareml_amd.store import GenotypeStore

V = int(sys.argv[1]) if len(sys.argv) > 1 else 230_000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
S, SEED, G = 2504, 1001, "chr_1"
BIG = 1 << 40


def naive(st, idx, keep=None):
    """read_windows of every sample over the group, reduced in torch -> int32 [n, 4]; samples in slices of 256 (the whole
    int8 matrix of 2504 samples is 1.15 GB, its boolean temporaries several times that)"""
    out = []
    for i in range(0, len(idx), 256):
        x = torch.stack(st.read_windows([(G, int(s), 0, V) for s in idx[i:i + 256]]))          # [n, V, 2] int8
        if keep is not None:
            x = x[:, keep]
        a, b = x[..., 0], x[..., 1]
        out.append(torch.stack([(x >= 0).sum((1, 2)), (x == 1).sum((1, 2)), ((a >= 0) & (b >= 0) & (a != b)).sum(1),
                                ((a == 1) & (b == 1)).sum(1)], 1).to(torch.int32))
    return torch.cat(out)


def kernel_ms(ctx, fn):
    ctx.profile_reset()
    r = fn()
    return r, ctx.profile_read()["decode"]["ms"]


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    ctx = dev.Context(0)
    h5 = build_cohort(ctx, tmp, V, S, SEED)
    ctx.profile(True)
    every, sub = np.arange(S), np.sort(np.random.default_rng(3).choice(S, 64, replace=False))
    out = dict(samples=S, variants=V, runs=RUNS)

    # correctness first: fused == naive, for both sample sets, with and without the mask (also the warm-up of both paths:
    # code objects loaded, the allocator grown to the naive path's matrix)
    warm = GenotypeStore(h5, ctx=ctx, cache_bytes=BIG)
    ref_all = naive(warm, every)
    maf = warm.variant_mask(G, min_maf=0.05)
    out.update(maf_variants=int(maf.sum()), naive_matrix_bytes=2 * V * S)
    assert torch.equal(warm.sample_counts(G), ref_all)
    assert torch.equal(warm.sample_counts(G, variant_mask=maf), naive(warm, every, maf))
    assert torch.equal(warm.sample_counts(G, sub), ref_all[torch.from_numpy(sub).to(ref_all.device)])
    assert torch.equal(warm.sample_counts(G, sub, variant_mask=maf), naive(warm, sub, maf))
    out["same_as_naive"] = True
    del ref_all

    # the calls, alternating repetition by repetition: fused cold (a store whose cache stays empty: every chunk read from the
    # file and uploaded), naive cold (a fresh store whose cache takes the whole group), naive and fused with every chunk cached
    cold = GenotypeStore(h5, ctx=ctx)
    cases = (("all", None, None), ("all_maf", None, maf), ("subset64", sub, None), ("subset64_maf", sub, maf))
    res = {name: dict(kernel_ms=[], call_cold_ms=[], call_cached_ms=[]) for name, _, _ in cases}
    nv = dict(cold=[], cached=[])
    for _ in range(RUNS):
        fresh = GenotypeStore(h5, ctx=ctx, cache_bytes=BIG)
        for name, idx, mask in cases:
            cold.stats.update(sample_count_blocks=0)
            (_, ms), k = kernel_ms(ctx, lambda: timed(lambda: cold.sample_counts(G, idx, variant_mask=mask)))
            res[name]["kernel_ms"].append(k)
            res[name]["call_cold_ms"].append(ms)
            res[name]["blocks_decoded"] = cold.stats["sample_count_blocks"]
            if name == "all":
                nv["cold"].append(timed(lambda: naive(fresh, every))[1])
                nv["cached"].append(timed(lambda: naive(fresh, every))[1])
            res[name]["call_cached_ms"].append(timed(lambda: warm.sample_counts(G, idx, variant_mask=mask))[1])
        fresh.close()
    for name, r in res.items():
        out[name] = dict({k: float(np.median(r[k])) for k in ("kernel_ms", "call_cold_ms", "call_cached_ms")},
                         kernel_ms_runs=r["kernel_ms"], call_cold_ms_runs=r["call_cold_ms"], blocks_decoded=r["blocks_decoded"])
    naive_cold, naive_cached = float(np.median(nv["cold"])), float(np.median(nv["cached"]))
    out.update(naive_cold_ms=naive_cold, naive_cached_ms=naive_cached, naive_cold_ms_runs=nv["cold"],
               naive_cached_ms_runs=nv["cached"])

    # the three kernels on the same device-resident chunks, alternating
    g = warm.meta["groups"][G]
    parts = [warm._read_chunk(G, v, s) for v in range(g["n_vcol"]) for s in range(g["n_scol"])]
    rel = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    src = torch.from_numpy(np.concatenate(parts)).to(ctx.device)
    d_off = torch.from_numpy(rel).to(ctx.device)
    cn, bs = warm.meta["sc"] * warm.meta["vc"] * 2, warm.meta["blocksize"]
    runs = dict(count_samples=[], count_alleles=[], decode_blocks=[])
    for _ in range(RUNS + 1):
        runs["count_samples"].append(kernel_ms(ctx, lambda: warm.sample_counts(G))[1])
        runs["count_alleles"].append(kernel_ms(ctx, lambda: warm.allele_counts(G))[1])
        (_, bad), ms = kernel_ms(ctx, lambda: ctx.decompress(src, d_off, len(parts), cn, typesize=2, blocksize=bs))
        assert bad == 0
        runs["decode_blocks"].append(ms)
    medians, spreads = summarize(runs)                  # (of every repetition but the first)
    out["kernels"] = dict(runs_ms=runs, **medians, **spreads)
    out["kernels"]["count_samples_vs_count_alleles"] = out["kernels"]["count_samples_ms"] / out["kernels"]["count_alleles_ms"]
    out["kernels"]["count_samples_vs_decode_blocks"] = out["kernels"]["count_samples_ms"] / out["kernels"]["decode_blocks_ms"]
    out["call_cold_vs_naive_cold"] = out["all"]["call_cold_ms"] / naive_cold
    out["call_cached_vs_naive_cached"] = out["all"]["call_cached_ms"] / naive_cached
    out.update(group_compressed_bytes=int(rel[-1]), group_chunks=len(parts))
    warm.close()
    cold.close()
    report("sample_count_bench", out)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
