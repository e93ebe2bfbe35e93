#!/usr/bin/env python3
"""LD clumping at cohort shape: GenotypeStore.ld_clump on the input of tools/ld_bench.py (a 2504-sample cohort file with one
chr1-sized group, 230 k synthetic variants, converter output in /dev/shm), all samples.  Two cases:

(a) "scan": p from GenotypeStore.assoc of a simulated phenotype (standard normal, no covariates), at the default thresholds
    (p1 1e-4, p2 1e-2, r2 0.5, window 1024, kb 250): about 1 % of the variants are counted;
(b) "ct": p1 = p2 = 1 under min_maf 0.01, r2 0.5, window 1024, kb 250: every variant of the mask is counted — the
    clumping + thresholding case, with the scan's p.

Reports per case, as one JSON line (also written to profiles/clump_bench.json): the call's ms cold (every chunk read from the
file and uploaded) and with every chunk in the read cache, the kernel ms of its stages (hhgt_genotype_planes under "decode",
hhgt_variant_planes under "ld_transpose", hhgt_ld_counts under "ld", hhgt_ld_decisions under "ld_prune", hhgt_ld_clump —
blockers, rounds and owners — under "ld_walk": ctx.profile_read()), the rounds and the clumps; k_ld_walk's ms on the same
tiles (GenotypeStore.ld_prune over the same counted variants at the same window, in the same process); and, alternating with
the call repetition by repetition in the same warmed-up process, the comparator route: the same link bits
(GenotypeStore._clump_links) downloaded and store_stats.clump_reference run on the host (the download and the walk timed
apart).  Medians of the runs and every run; the first repetition is printed but kept out of the medians.  The owners of the
two routes are asserted equal before any time is taken.  The synthetic generator's variants are independent, so the clumps
are nearly all singletons and few rounds decide: the cost of the rounds depends on their number, which is reported.  Not
timed: building and converting the cohort, the scan that makes p, the warm-up.
usage: clump_bench.py [variants] [runs]"""
import os, shutil, sys, tempfile, time
import numpy as np
import torch
from cohort_bench import build_cohort, report, summarize, timed
from haplohyped_varawareml_amd import device as dev
from haplohyped_varawareml_amd.store import ASSOC_P, GenotypeStore, clump_reference

V = int(sys.argv[1]) if len(sys.argv) > 1 else 230_000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
S, SEED, G = 2504, 1001, "chr_1"
WINDOW, R2, KB = 1024, 0.5, 250.0
BIG = 1 << 40


def host_route(st, p, mask, p1, p2, times=None):
    """the link bits of the device route, downloaded, and the sequential rule on the host -> owner int64 [V] (offsets into
    the group, -1 outside the counted set)"""
    lo, hi, counted, bits, pc = st._clump_links(G, p, None, 0, None, mask, p1, p2, R2, WINDOW, KB, None, None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    words, at, pc = bits.cpu().numpy().view(np.uint64), counted.cpu().numpy(), pc.cpu().numpy()
    t1 = time.perf_counter()
    linked = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :WINDOW].astype(bool)    # bit d of word d // 64
    own = clump_reference(linked, pc, p1)
    out = np.full(hi - lo, -1, np.int64)
    out[at] = np.where(own >= 0, at[np.maximum(own, 0)], -1)
    if times is not None:
        times[0].append((t1 - t0) * 1e3)
        times[1].append((time.perf_counter() - t1) * 1e3)
    return out


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    ctx = dev.Context(0)
    h5 = build_cohort(ctx, tmp, V, S, SEED)
    ctx.profile(True)
    warm = GenotypeStore(h5, ctx=ctx, cache_bytes=BIG)
    cold = GenotypeStore(h5, ctx=ctx)
    y = np.random.default_rng(SEED).normal(size=S)
    p = warm.assoc(G, y, None)[0][:, 0, ASSOC_P].contiguous()       # NaN where a variant is not tested
    maf = warm.variant_mask(G, min_maf=0.01)
    out = dict(date=time.strftime("%Y-%m-%d"), samples=S, variants=V, window=WINDOW, r2=R2, kb=KB, runs=RUNS)
    stages = dict(planes_kernel_ms="decode", transpose_kernel_ms="ld_transpose", counts_kernel_ms="ld",
                  decide_kernel_ms="ld_prune", clump_kernel_ms="ld_walk")
    for name, mask, p1, p2 in (("scan", None, 1e-4, 1e-2), ("ct", maf, 1.0, 1.0)):
        call = lambda st: st.ld_clump(G, p, variant_mask=mask, p1=p1, p2=p2, r2=R2, window=WINDOW, kb=KB)      # noqa: E731
        # correctness first, which is also the warm-up of both routes (code objects loaded, the allocator grown)
        warm.stats.update(clump_rounds=0, clump_window_short=0)
        got = call(warm).cpu().numpy()
        ref = host_route(warm, p, mask, p1, p2)
        assert np.array_equal(got, ref)
        counted = torch.isfinite(p) & (p <= p2) if mask is None else torch.isfinite(p) & (p <= p2) & mask
        n_counted, n_index = int(counted.sum()), int((got == np.arange(V)).sum())
        n_clumped = int(((got >= 0) & (got != np.arange(V))).sum())
        res = dict(same_as_host=True, counted=n_counted, rounds=warm.stats["clump_rounds"], clumps=n_index, clumped=n_clumped,
                   none=n_counted - n_index - n_clumped, window_short=warm.stats["clump_window_short"])
        del got, ref
        runs = dict(call_cold_ms=[], call_cached_ms=[], host_route_cached_ms=[], host_download_ms=[], host_walk_ms=[],
                    prune_cached_ms=[], prune_walk_kernel_ms=[], **{k: [] for k in stages})
        for _ in range(RUNS + 1):
            runs["call_cold_ms"].append(timed(lambda: call(cold))[1])
            runs["host_route_cached_ms"].append(timed(lambda: host_route(warm, p, mask, p1, p2,
                                                                         (runs["host_download_ms"], runs["host_walk_ms"])))[1])
            ctx.profile_reset()
            runs["call_cached_ms"].append(timed(lambda: call(warm))[1])
            prof = ctx.profile_read()
            for k, stage in stages.items():
                runs[k].append(prof[stage]["ms"])
            # k_ld_walk on the same tiles: ld_prune over the same counted variants at the same window
            ctx.profile_reset()
            runs["prune_cached_ms"].append(timed(lambda: warm.ld_prune(G, variant_mask=counted, window=WINDOW, r2=R2))[1])
            runs["prune_walk_kernel_ms"].append(ctx.profile_read()["ld_walk"]["ms"])
        medians, spreads = summarize(runs)                  # (of every repetition but the first)
        res.update(runs_ms=runs, **medians, **spreads)
        res.update(call_cached_vs_host_route=res["call_cached_ms"] / res["host_route_cached_ms"],
                   clump_kernel_vs_prune_walk_kernel=res["clump_kernel_ms"] / res["prune_walk_kernel_ms"])
        out[name] = res
    warm.close()
    cold.close()
    report("clump_bench", out)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
