#!/usr/bin/env python3
"""Region burden scores at cohort shape: GenotypeStore.region_sums / burden on the input of tools/grm_bench.py (a 2504-sample
cohort file with one chr1-sized group, 230 k synthetic variants, converter output in /dev/shm), all samples, the variants
with a minor allele frequency of at most 0.01 and at least one ALT allele, in tiled 100-kb regions, unit weights.

Reports, as one JSON line and in profiles/burden_bench.json: the ms of region_sums (the class weights given) and of burden
(allele counts, weights, region_sums, totals) cold — every chunk read from the file and uploaded — and with every chunk in the
read cache; the kernel ms of its stages (ctx.profile_read(): "decode" holds hhgt_genotype_planes, "assoc" hhgt_region_sums'
two launches); and, alternating with it repetition by repetition in the same warmed-up process, two other routes on the
cached chunks: (a) the device route there was before — GenotypeStore.score_sums under the same mask with one-hot region
columns, 64 regions per pass, the [3, V, 64] weight tensors of all passes built beforehand and not timed —, (b) torch:
read_windows of every sample, a float64 dosage matrix [S, V] (0 where the call is not complete) and one matmul with a one-hot
matrix [V, R] (also timed alone).  Medians of the runs and every run; the first repetition is printed but kept out of the
medians.  Before any time is taken the three routes' tables are compared: unit weights, integers, so they must be equal.
Not timed: building and converting the cohort, the mask, the uploads, the warm-up.
usage: burden_bench.py [variants] [runs]"""
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
TILE, MAX_MAF, PER_PASS = 100_000, 0.01, 64


def torch_route(st, onehot, times=None):
    """read_windows of every sample (slices of 256), the float64 dosages [S, V] (0 where the call is not complete), one
    matmul with onehot [V, R] (zero rows where the mask leaves a variant out) -> float64 [S, R]"""
    D = torch.empty((S, V), dtype=torch.float64, device=onehot.device)
    for i in range(0, S, 256):
        x = torch.stack(st.read_windows([(G, s, 0, V) for s in range(i, min(i + 256, S))]))   # [n, V, 2] int8
        a, b = x[..., 0], x[..., 1]
        done = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
        D[i:i + x.shape[0]] = torch.where(done, (a + b).double(), torch.zeros((), dtype=torch.float64, device=onehot.device))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = D @ onehot
    torch.cuda.synchronize()
    if times is not None:
        times.append((time.perf_counter() - t0) * 1e3)
    return out


def one_hot_route(st, passes, mask):
    """score_sums over one-hot region columns, PER_PASS regions a pass -> float64 [S, R]"""
    return torch.cat([st.score_sums(w, G, variant_mask=mask) for w in passes], dim=1)


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    ctx = dev.Context(0)
    h5 = build_cohort(ctx, tmp, V, S, SEED)
    ctx.profile(True)
    warm, cold = GenotypeStore(h5, ctx=ctx, cache_bytes=BIG), GenotypeStore(h5, ctx=ctx)
    start = warm.variants(G)[0].astype(np.int64)
    tile = start // TILE
    ids = np.unique(tile)
    regions = np.stack([np.searchsorted(tile, ids, side="left"), np.searchsorted(tile, ids, side="right")], axis=1).astype(np.int64)
    R = len(regions)
    mask = warm.variant_mask(G, None, max_maf=MAX_MAF, min_ac=1)
    out = dict(samples=S, variants=V, runs=RUNS, regions=R, tile_bp=TILE, max_maf=MAX_MAF, masked_variants=int(mask.sum()),
               regions_per_pass=PER_PASS, passes=-(-R // PER_PASS))
    dosage = torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64, device=ctx.device)
    Wd = (dosage[:, None, None] * torch.ones((1, V, 1), dtype=torch.float64, device=ctx.device)).contiguous()
    member = torch.zeros((V, R), dtype=torch.float64, device=ctx.device)
    member[torch.arange(V, device=ctx.device), torch.from_numpy(np.searchsorted(ids, tile)).to(ctx.device)] = 1.0
    passes = [(dosage[:, None, None] * member[None, :, k:k + PER_PASS]).contiguous() for k in range(0, R, PER_PASS)]
    onehot = member * mask.to(torch.float64)[:, None]

    # correctness first, which is also the warm-up of the routes (code objects loaded, the allocator grown)
    got = warm.region_sums(G, regions, Wd, variant_mask=mask)[:, :, 0]
    B, used = warm.burden(G, regions, None, variant_mask=mask, impute="none")
    assert torch.equal(got, one_hot_route(warm, passes, mask)) and torch.equal(got, torch_route(warm, onehot))
    assert torch.equal(got, B[:, :, 0]) and int(used.sum()) == out["masked_variants"]
    out.update(nonzero_fraction=float((got != 0).double().mean()), largest_count=float(got.max()))
    del got, B

    runs = dict(region_sums_cold_ms=[], region_sums_cached_ms=[], burden_cold_ms=[], burden_cached_ms=[], planes_kernel_ms=[],
                region_kernel_ms=[], one_hot_cached_ms=[], one_hot_planes_kernel_ms=[], one_hot_score_kernel_ms=[],
                torch_cached_ms=[], torch_matmul_ms=[])
    for _ in range(RUNS + 1):
        runs["region_sums_cold_ms"].append(timed(lambda: cold.region_sums(G, regions, Wd, variant_mask=mask))[1])
        runs["burden_cold_ms"].append(timed(lambda: cold.burden(G, regions, None, variant_mask=mask))[1])
        runs["torch_cached_ms"].append(timed(lambda: torch_route(warm, onehot, runs["torch_matmul_ms"]))[1])
        ctx.profile_reset()
        runs["one_hot_cached_ms"].append(timed(lambda: one_hot_route(warm, passes, mask))[1])
        prof = ctx.profile_read()
        runs["one_hot_planes_kernel_ms"].append(prof["decode"]["ms"])
        runs["one_hot_score_kernel_ms"].append(prof["assoc"]["ms"])
        ctx.profile_reset()
        warm.stats.update(region_plane_blocks=0, region_pieces=0, region_variants=0)
        runs["region_sums_cached_ms"].append(timed(lambda: warm.region_sums(G, regions, Wd, variant_mask=mask))[1])
        prof = ctx.profile_read()
        runs["planes_kernel_ms"].append(prof["decode"]["ms"])
        runs["region_kernel_ms"].append(prof["assoc"]["ms"])
        pieces, blocks = warm.stats["region_pieces"], warm.stats["region_plane_blocks"]
        runs["burden_cached_ms"].append(timed(lambda: warm.burden(G, regions, None, variant_mask=mask))[1])
    medians, spreads = summarize(runs)                      # (of every repetition but the first)
    out.update(runs_ms=runs, pieces=pieces, plane_blocks_decoded=blocks, **medians, **spreads)
    out.update(region_sums_cached_vs_one_hot=out["region_sums_cached_ms"] / out["one_hot_cached_ms"],
               region_sums_cached_vs_torch=out["region_sums_cached_ms"] / out["torch_cached_ms"])
    warm.close()
    cold.close()
    report("burden_bench", out)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
