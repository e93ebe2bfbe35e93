#!/usr/bin/env python3
"""Read side at cohort shape: RandomHaplotypeDataset on a 2504-sample store with one chr1-sized group (230 k synthetic
variants, converter output), batch 32 x seq_length 131072 x 5 channels, BED of random regions in the group.

Reports, as one JSON line: cold ms per batch (a fresh GenotypeStore for every batch: every chunk read from the file) and
warm ms per batch (every chunk of the group in the device cache); compressed bytes read and bytes decoded per batch; decode
and one-hot kernel ms (ctx.profile_read()); the one-hot write rate against 8 TB/s; and the same items through the
whole-chunk-row decode the store used before windowed reads (every chunk of the donor's 64-sample chunk row decoded with
hhgt_decompress_chunks, one sample kept, copied to the host and back), rebuilt here as the comparison point.
usage: window_bench.py [variants] [batches]"""
import os, shutil, sys, tempfile, time
import numpy as np
import torch
from cohort_bench import build_cohort, report
from haplohyped_varawareml_amd import device as dev, synth
from haplohyped_varawareml_amd.dataset import RandomHaplotypeDataset
from haplohyped_varawareml_amd.store import GenotypeStore

V = int(sys.argv[1]) if len(sys.argv) > 1 else 230_000
NB = int(sys.argv[2]) if len(sys.argv) > 2 else 10
S, B, L, SEED = 2504, 32, 131072, 1001
tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    ctx = dev.Context(0)
    h5 = build_cohort(ctx, tmp, V, S, SEED)
    names, samples = synth.sample_names(S), os.path.join(tmp, "samples.txt")
    rng = np.random.default_rng(5)
    span = int(synth.variant_table(SEED, V, S)["pos"][-1]) + 1000
    np.savez(os.path.join(tmp, "ref.npz"), chr1=np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, span)])
    bed = os.path.join(tmp, "regions.bed")
    with open(bed, "w") as f:
        for a in sorted(rng.integers(0, span - 2000, 1000).tolist()):
            f.write(f"chr1\t{a}\t{a + 1000}\n")
    ds = RandomHaplotypeDataset(bed, h5, os.path.join(tmp, "ref.npz"), samples, seed=42, batch_size=B, seq_length=L, ctx=ctx)
    ds[0]                                              # group tables and reference bases on the device, kernels loaded
    torch.cuda.synchronize()

    # cold: a fresh store (empty chunk cache) for every batch
    cold_ms, cold_items, reads, decoded = [], [], [], []
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(NB):
        ds.store.close()
        ds.store = GenotypeStore(h5, ctx=ctx)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h1, h2 = ds[0]
        torch.cuda.synchronize()
        cold_ms.append((time.perf_counter() - t0) * 1e3)
        cold_items.append(list(ds.last_items))
        reads.append(ds.store.stats["compressed_bytes_read"])
        decoded.append(ds.store.stats["bytes_decoded"])
    prof = ctx.profile_read()
    meta = ds.store.meta
    g = meta["groups"]["chr_1"]

    # warm: every chunk of the group in the device cache first (one request per sample chunk row)
    ds.store.close()
    ds.store = GenotypeStore(h5, ctx=ctx, cache_bytes=1 << 40)
    ds.store.read_windows([("chr_1", sc * meta["sc"], 0, V) for sc in range(g["n_scol"])])
    assert ds.store.stats["chunks_read"] == g["n_chunks"]
    before = dict(ds.store.stats)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(NB):
        ds[0]
    torch.cuda.synchronize()
    warm_ms = (time.perf_counter() - t0) * 1e3 / NB
    assert ds.store.stats["chunks_read"] == before["chunks_read"]

    # the whole-chunk-row decode on the same items as the cold batches (the store's read path before windowed reads)
    old = GenotypeStore(h5, ctx=ctx)
    cn, idx = meta["sc"] * meta["vc"] * 2, {s: i for i, s in enumerate(names)}
    ctx.profile_reset()
    old_ms, old_read = [], []
    for items in cold_items:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nbytes = 0
        for it in items:
            s = idx[it["donor"]]
            scol, sin = divmod(s, meta["sc"])
            parts = old._chunk_row("chr_1", scol)
            rel = np.concatenate([[0], np.cumsum([p.size for p in parts])])
            nbytes += int(rel[-1])
            src = torch.from_numpy(np.concatenate(parts)).to(ctx.device)
            d_off = torch.from_numpy(rel.astype(np.int64)).to(ctx.device)
            out, bad = ctx.decompress(src, d_off, len(parts), cn, typesize=meta["typesize"], blocksize=meta["blocksize"])
            assert bad == 0
            row = out.view(torch.int8).view(len(parts), meta["sc"], meta["vc"], 2)[:, sin].reshape(-1, 2)[:V].cpu().numpy()
            torch.from_numpy(row).to(ctx.device)
        torch.cuda.synchronize()
        old_ms.append((time.perf_counter() - t0) * 1e3)
        old_read.append(nbytes)
    old_prof = ctx.profile_read()
    old_decoded = B * g["n_vcol"] * cn
    old.close()

    onehot_ms = prof["onehot"]["ms"] / NB
    out_bytes = 2 * B * L * ds.n_channels * 4
    res = dict(samples=S, variants=V, batch=B, seq_length=L, channels=ds.n_channels, batches=NB,
               cold_ms_per_batch=float(np.median(cold_ms)), cold_ms_min=min(cold_ms), cold_ms_max=max(cold_ms),
               warm_ms_per_batch=warm_ms,
               compressed_bytes_read_per_batch=float(np.mean(reads)), bytes_decoded_per_batch=float(np.mean(decoded)),
               decode_kernel_ms_per_batch=prof["decode"]["ms"] / NB, onehot_kernel_ms_per_batch=onehot_ms,
               onehot_write_GBps=out_bytes / (onehot_ms * 1e-3) / 1e9, onehot_write_floor_us=out_bytes / 8e12 * 1e6,
               old_ms_per_batch=float(np.median(old_ms)), old_compressed_bytes_read_per_batch=float(np.mean(old_read)),
               old_bytes_decoded_per_batch=old_decoded, old_decode_kernel_ms_per_batch=old_prof["decode"]["ms"] / NB,
               decoded_bytes_ratio=old_decoded / max(float(np.mean(decoded)), 1.0),
               cold_target_5ms_met=bool(np.median(cold_ms) <= 5.0))
    ds.close()
    report("window_bench", res)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
