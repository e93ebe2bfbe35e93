#!/usr/bin/env python3
"""Per-variant allele counts at cohort shape: GenotypeStore.allele_counts on a 2504-sample cohort file with one chr1-sized
group (230 k synthetic variants, converter output in /dev/shm), over all samples and over a random 64-sample subset.

Reports, as one JSON line, for each sample set: the count kernel's ms (hhgt_count_alleles, ctx.profile_read()) and the
call's ms (chunks read from the file, uploaded, counted; median of the runs), compressed bytes read and Blosc blocks
decoded per call; the naive path on the same samples (read_windows of every sample over the whole group, then a torch
reduction of the int8 matrix), its ms and the bytes of matrix it writes; and hhgt_decompress_chunks (k_decode_blocks) on
every chunk of the same group, the whole-chunk decode the fused kernel is measured against.  The fused and the naive
counts are compared.
usage: allele_count_bench.py [variants] [runs]"""
import os, shutil, sys, tempfile
import numpy as np
import torch
from cohort_bench import build_cohort, report, timed
from haplohyped_varawareml_amd import device as dev
from haplohyped_varawareml_amd.store import GenotypeStore

V = int(sys.argv[1]) if len(sys.argv) > 1 else 230_000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
S, SEED, G = 2504, 1001, "chr_1"


def naive(st, idx):
    """read_windows of every sample over the group, reduced in torch -> int32 [V, 4]"""
    rows = st.read_windows([(G, int(s), 0, V) for s in idx])
    x = torch.stack(rows)                                          # [n, V, 2] int8
    a, b = x[..., 0], x[..., 1]
    out = torch.stack([(x >= 0).sum((0, 2)), (x == 1).sum((0, 2)), ((a >= 0) & (b >= 0) & (a != b)).sum(0),
                       ((a == 1) & (b == 1)).sum(0)], 1)
    return out.to(torch.int32)


def measure(ctx, h5, idx):
    st = GenotypeStore(h5, ctx=ctx)
    samples = None if len(idx) == S else idx
    first = st.allele_counts(G, samples)                          # warm-up (code objects loaded)
    call_ms, kern_ms = [], []
    for _ in range(RUNS):
        st.stats.update(count_blocks=0, count_compressed_bytes_read=0)
        ctx.profile_reset()
        c, ms = timed(lambda: st.allele_counts(G, samples))
        call_ms.append(ms)
        kern_ms.append(ctx.profile_read()["decode"]["ms"])
        assert torch.equal(c, first)
    res = dict(kernel_ms=float(np.median(kern_ms)), call_ms=float(np.median(call_ms)),
               compressed_bytes_read=st.stats["count_compressed_bytes_read"], blocks_decoded=st.stats["count_blocks"])
    st.close()
    # naive: a store whose cache holds the whole group, so a second call measures decode + reduction only
    st = GenotypeStore(h5, ctx=ctx, cache_bytes=1 << 40)
    nv_ms = []
    for _ in range(2):
        nv, ms = timed(lambda: naive(st, idx))
        nv_ms.append(ms)
    res.update(naive_cold_ms=nv_ms[0], naive_warm_ms=nv_ms[1], naive_matrix_bytes=2 * V * len(idx),
               same_as_naive=bool(torch.equal(nv, first)))
    st.close()
    del nv
    return res


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    ctx = dev.Context(0)
    h5 = build_cohort(ctx, tmp, V, S, SEED)
    ctx.profile(True)
    out = dict(samples=S, variants=V, runs=RUNS, all=measure(ctx, h5, np.arange(S)),
               subset64=measure(ctx, h5, np.sort(np.random.default_rng(3).choice(S, 64, replace=False))))

    # k_decode_blocks on every chunk of the same group (device-resident), as tools/decode_bench.py times it
    st = GenotypeStore(h5, ctx=ctx)
    meta = st.meta
    g = meta["groups"][G]
    parts = [st._read_chunk(G, v, s) for v in range(g["n_vcol"]) for s in range(g["n_scol"])]
    rel = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    src = torch.from_numpy(np.concatenate(parts)).to(ctx.device)
    d_off = torch.from_numpy(rel).to(ctx.device)
    cn = meta["sc"] * meta["vc"] * 2
    _, bad = ctx.decompress(src, d_off, len(parts), cn, typesize=2, blocksize=meta["blocksize"])
    assert bad == 0
    ctx.profile_reset()
    for _ in range(RUNS):
        _, bad = ctx.decompress(src, d_off, len(parts), cn, typesize=2, blocksize=meta["blocksize"])
    out.update(decode_blocks_kernel_ms=ctx.profile_read()["decode"]["ms"] / RUNS, group_compressed_bytes=int(rel[-1]),
               group_chunks=len(parts))
    out["all"]["kernel_vs_decode_blocks"] = out["all"]["kernel_ms"] / out["decode_blocks_kernel_ms"]
    st.close()
    report("allele_count_bench", out)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
