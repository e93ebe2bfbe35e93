#!/usr/bin/env python3
"""The feature matrix at cohort shape: GenotypeStore.feature_matrix on the input of tools/grm_bench.py (a 2504-sample cohort
file with one chr1-sized group, 230 k synthetic variants, converter output in /dev/shm) against the torch route it replaces.
Three configurations: (a) every sample, float16 standardized, the variants with MAF >= 0.01 that ld_prune(50, 0.2) keeps;
(b) 256 random samples in random order, the same mask; (c) every sample, every variant, int8 dosage (-1 where the call is
not complete).

Reports, as one JSON line and in profiles/feature_bench.json, per configuration: the call's ms cold (every chunk read from
the file and uploaded) and with every chunk in the read cache — the call includes its allele-count pass over the listed
samples where the coding needs frequencies, also timed alone —; alternating with it repetition by repetition in the same
warmed-up process, the torch route on the cached chunks: read_windows of the same samples (slices of 256), indexing with
the columns, the class of every call, a lookup in the same 4 x M table (handed to it: its counts are not timed), which is the
cast; the "decode" stage's kernel ms (ctx.profile_read()) of the call, of its count pass alone, and of
hhgt_genotype_planes over the same samples and mask (the same Blosc blocks decoded: the difference to the gather is the
price of compaction and stores).  Medians of the runs and every run; the first repetition is printed but kept out of the
medians.  Before any time is taken the two routes' matrices are compared byte for byte.  Not timed: building and converting
the cohort, the masks, the warm-up.
`feature_bench.py kernels [variants]` runs only configuration (a)'s cached call and the plane walk, three times each, for
a `rocprofv3 --kernel-trace --stats` run around it; HHGT_FEATURE_KSTATS = that run's kernel_stats csv adds k_gather_calls'
and k_genotype_planes' calls and total ms from it to the result.
usage: feature_bench.py [variants] [runs]"""
import csv, os, shutil, sys, tempfile
import numpy as np
import torch
from cohort_bench import build_cohort, report, summarize, timed
from haplohyped_varawareml_amd import device as dev
from haplohyped_varawareml_amd.store import GenotypeStore, call_class_values, cast_class_values

KERNELS = len(sys.argv) > 1 and sys.argv[1] == "kernels"
ARGS = sys.argv[2:] if KERNELS else sys.argv[1:]
V = int(ARGS[0]) if len(ARGS) > 0 else 230_000
RUNS = int(ARGS[1]) if len(ARGS) > 1 else 5
S, SEED, G = 2504, 1001, "chr_1"
BIG = 1 << 40


def torch_route(st, idx, cols, table):
    """read_windows of the samples idx (slices of 256), the columns `cols`, the class of every call, its entry of `table`
    [4, M] -> [len(idx), M] of the table's dtype"""
    X = torch.empty((len(idx), cols.numel()), dtype=table.dtype, device=table.device)
    at = torch.arange(cols.numel(), device=table.device)[None, :]
    for i in range(0, len(idx), 256):
        x = torch.stack(st.read_windows([(G, int(s), 0, V) for s in idx[i:i + 256]])).index_select(1, cols)   # [n, M, 2] int8
        a, b = x[..., 0].long(), x[..., 1].long()
        done = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
        X[i:i + x.shape[0]] = table[torch.where(done, a + b, torch.full_like(a, 3)), at]
    return X


def plane_pass(st, idx, mask):
    """hhgt_genotype_planes over the samples and mask of a configuration: the blocks the gather decodes"""
    vmask = None if mask is None else st._device_mask(mask, 0, V)
    for _ in st._plane_walk(G, np.unique(idx), 0, V, V, "pair_plane_blocks", None, None, vmask):
        pass


def decode_ms(ctx, fn):
    ctx.profile_reset()
    fn()
    torch.cuda.synchronize()
    return ctx.profile_read()["decode"]["ms"]


def kernel_stats(path):
    """{kernel: (calls, total ms)} of k_gather_calls and k_genotype_planes from a rocprofv3 kernel_stats csv"""
    out = {}
    for row in csv.DictReader(open(path)):
        for k in ("k_gather_calls", "k_genotype_planes"):
            if k in row["Name"]:
                out[k] = dict(calls=int(row["Calls"]), total_ms=float(row["TotalDurationNs"]) / 1e6)
    return out


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    ctx = dev.Context(0)
    h5 = build_cohort(ctx, tmp, V, S, SEED)
    ctx.profile(True)
    rng = np.random.default_rng(SEED)
    warm, cold = GenotypeStore(h5, ctx=ctx, cache_bytes=BIG), GenotypeStore(h5, ctx=ctx)
    every = np.arange(S)
    pruned = warm.ld_prune(G, variant_mask=warm.variant_mask(G, min_maf=0.01), window=50, r2=0.2)
    configs = dict(
        a_all_samples_f16_standardized_pruned=(every, pruned, dict(coding="standardized", dtype=torch.float16)),
        b_256_samples_f16_standardized_pruned=(rng.permutation(S)[:256], pruned, dict(coding="standardized", dtype=torch.float16)),
        c_all_samples_int8_dosage_dense=(every, None, dict(coding="dosage", dtype=torch.int8, impute="missing")))
    out = dict(samples=S, variants=V, runs=RUNS, pruned_variants=int(pruned.sum()))
    if KERNELS:
        idx, mask, kw = configs["a_all_samples_f16_standardized_pruned"]
        warm.read_windows([(G, int(s), 0, V) for s in range(0, S, 64)])           # every chunk into the cache
        for _ in range(3):
            warm.feature_matrix(G, idx, variant_mask=mask, **kw)
            plane_pass(warm, idx, mask)
        torch.cuda.synchronize()
        print("kernels: 3 x (feature_matrix, plane walk) of configuration (a)")
        sys.exit(0)
    for name, (idx, mask, kw) in configs.items():
        # correctness first, which is also the warm-up of both routes (code objects loaded, the allocator grown, the cache filled)
        got, columns = warm.feature_matrix(G, idx, variant_mask=mask, **kw)
        cols = columns[0][1]
        needs_counts = not (kw["coding"] == "dosage" and kw.get("impute") == "missing")
        counts = warm.allele_counts(G, np.unique(idx)) if needs_counts else torch.zeros((V, 4), dtype=torch.int32, device=ctx.device)
        table = cast_class_values(call_class_values(counts, kw["coding"], kw.get("impute", "mean"))[0][:, cols], kw["dtype"])
        ref = torch_route(warm, idx, cols, table)
        view = torch.int16 if got.element_size() == 2 else torch.int8
        assert got.shape == ref.shape and torch.equal(got.view(view), ref.view(view)), name
        assert torch.equal(cold.feature_matrix(G, idx, variant_mask=mask, **kw)[0].view(view), ref.view(view)), name
        del got, ref

        runs = dict(call_cold_ms=[], call_cached_ms=[], torch_cached_ms=[], count_pass_cached_ms=[], call_decode_kernel_ms=[],
                    count_decode_kernel_ms=[], planes_decode_kernel_ms=[])
        for _ in range(RUNS + 1):
            runs["call_cold_ms"].append(timed(lambda: cold.feature_matrix(G, idx, variant_mask=mask, **kw))[1])
            runs["torch_cached_ms"].append(timed(lambda: torch_route(warm, idx, cols, table))[1])
            ctx.profile_reset()
            warm.stats.update(gather_blocks=0)
            runs["call_cached_ms"].append(timed(lambda: warm.feature_matrix(G, idx, variant_mask=mask, **kw))[1])
            runs["call_decode_kernel_ms"].append(ctx.profile_read()["decode"]["ms"])
            if needs_counts:
                ctx.profile_reset()
                runs["count_pass_cached_ms"].append(timed(lambda: warm.allele_counts(G, np.unique(idx)))[1])
                runs["count_decode_kernel_ms"].append(ctx.profile_read()["decode"]["ms"])
            else:
                runs["count_pass_cached_ms"].append(0.0)
                runs["count_decode_kernel_ms"].append(0.0)
            runs["planes_decode_kernel_ms"].append(decode_ms(ctx, lambda: plane_pass(warm, idx, mask)))
        medians, spreads = summarize({k: v for k, v in runs.items() if any(v)})
        res = dict(rows=len(idx), columns=int(cols.numel()), bytes=len(idx) * int(cols.numel()) * table.element_size(),
                   gather_blocks_decoded=warm.stats["gather_blocks"], runs_ms=runs, **medians, **spreads)
        res.update(gather_kernel_ms=res["call_decode_kernel_ms"] - res.get("count_decode_kernel_ms", 0.0),
                   call_cached_vs_torch_cached=res["call_cached_ms"] / res["torch_cached_ms"])
        res["gather_kernel_vs_planes_kernel"] = res["gather_kernel_ms"] / res["planes_decode_kernel_ms"]
        out[name] = res
        del table
    if os.environ.get("HHGT_FEATURE_KSTATS"):
        out["rocprofv3_kernel_stats_configuration_a_3_calls"] = kernel_stats(os.environ["HHGT_FEATURE_KSTATS"])
    warm.close()
    cold.close()
    report("feature_bench", out)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
