"""-m gpu: windowed genotype reads.  hhgt_decompress_blocks (one Blosc block per workgroup, a byte range of it written out)
against the whole-chunk decode and the source bytes; bad selections counted exactly; GenotypeStore.read_windows /
sample_row / VCFH5Reader.fetch_region on converter output (the .h5 and the directory store) against the synthetic
generator's own genotypes; the dataset at cohort shape against a numpy restatement of its rules."""
import os

import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd import device as dev, synth
from haplohyped_varawareml_amd.device import SEL_DTYPE

pytestmark = pytest.mark.gpu


def genotype_like(rng, n):
    """mostly 0, some 1, a few -9: compresses like genotype chunks"""
    a = (rng.random(n) < 0.05).astype(np.int8)
    a[rng.random(n) < 0.003] = -9
    return a.view(np.uint8)


def make_chunks(ctx, rng, n_chunks, chunk_nbytes, typesize, blocksize, fmt, memcpyed=None):
    raw = np.concatenate([rng.integers(0, 256, chunk_nbytes, dtype=np.uint8) if i == memcpyed else
                          genotype_like(rng, chunk_nbytes) for i in range(n_chunks)])
    src = torch.from_numpy(raw).to(ctx.device)
    dst, off, total = ctx.compress(src, chunk_nbytes, typesize=typesize, blocksize=blocksize, fmt=fmt)
    return raw, dst, off.cpu().numpy().astype(np.int64), total


def random_selections(rng, dst, off, chunk_nbytes, bs, n, aligned=4):
    """n random selections (duplicates and any block order), written end to end with gaps of 0..17 bytes (unaligned
    lo / hi / dst_off), plus `aligned` selections at 16-byte aligned destinations: whole blocks, and 16-byte aligned ranges
    with 0 < lo < hi < block size"""
    nchunks, nblocks = len(off) - 1, -(-chunk_nbytes // bs)
    rows, pos = [], 0
    for k in range(n + aligned):
        if k > 0 and k % 7 == 0:
            rows.append(rows[int(rng.integers(len(rows)))][:4])        # a duplicate of an earlier selection
        else:
            i, b = int(rng.integers(nchunks)), int(rng.integers(nblocks))
            bsize = min(bs, chunk_nbytes - b * bs)
            if k >= n and ((k - n) % 2 == 0 or bsize < 48):
                lo, hi = 0, bsize
            elif k >= n:                                                 # 16-byte aligned, strictly inside the block
                lo = 16 * int(rng.integers(1, bsize // 16 - 1))
                hi = 16 * int(rng.integers(lo // 16 + 1, bsize // 16))
            else:
                lo = int(rng.integers(bsize))
                hi = int(rng.integers(lo + 1, bsize + 1))
            rows.append((i, b, lo, hi))
        i, b, lo, hi = rows[-1]
        pos = (pos + 15) // 16 * 16 if k >= n else pos + int(rng.integers(0, 18))
        rows[-1] = (i, b, lo, hi, pos)
        pos += hi - lo
    sel = np.zeros(len(rows), SEL_DTYPE)
    for j, (i, b, lo, hi, d) in enumerate(rows):
        sel[j] = (dst.data_ptr() + int(off[i]), int(off[i + 1] - off[i]), d, b, lo, hi, 0)
    return sel, rows, pos


CASES = [  # fmt, typesize, blocksize, chunk_nbytes
    (dev.BLOSC1, 2, 8192, 3 * 8192 + 1400),      # split streams, short last block
    (dev.BLOSC2, 2, 8192, 3 * 8192 + 1400),
    (dev.BLOSC1, 1, 4096, 2 * 4096 + 1001),      # typesize 1
    (dev.BLOSC2, 1, 8192, 4 * 8192),
    (dev.BLOSC2, 2, 128, 1000),                  # typesize 2, unsplit (blocksize / typesize < 128)
    (dev.BLOSC1, 4, 2048, 4 * 2048 + 404),       # typesize 4, split
]


@pytest.mark.parametrize("fmt,ts,bs,cn", CASES)
def test_blocks_match_full_decode(ctx, fmt, ts, bs, cn):
    rng = np.random.default_rng(ts * 1000 + bs + fmt)
    n_chunks = 4
    raw, dst, off, total = make_chunks(ctx, rng, n_chunks, cn, ts, bs, fmt, memcpyed=2)
    hdr = dst[:total].cpu().numpy()
    assert hdr[off[2] + 2] & 0x2 and not hdr[off[0] + 2] & 0x2       # chunk 2 is stored memcpyed, chunk 0 compressed
    full, bad = ctx.decompress(dst, torch.from_numpy(off).to(ctx.device), n_chunks, cn, typesize=ts, blocksize=bs)
    assert bad == 0 and np.array_equal(full.cpu().numpy(), raw)
    sel, rows, size = random_selections(rng, dst, off, cn, bs, 40, aligned=8)
    out = torch.full((size + 64,), 0xA5, dtype=torch.uint8, device=ctx.device)
    out, bad = ctx.decompress_blocks(sel, cn, typesize=ts, blocksize=bs, dst=out)
    assert bad == 0
    o = out.cpu().numpy()
    for i, b, lo, hi, d in rows:
        a = i * cn + b * bs
        assert np.array_equal(o[d:d + hi - lo], raw[a + lo:a + hi]), (i, b, lo, hi, d)


def test_bad_selections_counted(ctx):
    rng = np.random.default_rng(5)
    cn, bs, ts = 3 * 8192 + 1400, 8192, 2
    raw, dst, off, total = make_chunks(ctx, rng, 3, cn, ts, bs, dev.BLOSC2)
    broken = dst[:total].clone()
    broken[int(off[1]) + 12] ^= 0x40                                   # chunk 1: cbytes of the header no longer match
    sel, rows, size = random_selections(rng, dst, off, cn, bs, 24, aligned=2)
    extra = np.zeros(4, SEL_DTYPE)
    nblocks = -(-cn // bs)
    extra[0] = (broken.data_ptr() + int(off[1]), int(off[2] - off[1]), size, 0, 0, 100, 0)     # corrupt chunk
    extra[1] = (dst.data_ptr(), int(off[1] - off[0]), size, nblocks, 0, 10, 0)                # block past the end
    extra[2] = (dst.data_ptr(), int(off[1] - off[0]), size, nblocks - 1, 0, cn - (nblocks - 1) * bs + 1, 0)  # hi past the block
    extra[3] = (dst.data_ptr(), int(off[1] - off[0]), size, 0, 7, 7, 0)                       # lo == hi
    allsel = np.concatenate([sel[:10], extra[:2], sel[10:], extra[2:]])
    out = torch.zeros(size + 8192, dtype=torch.uint8, device=ctx.device)
    out, bad = ctx.decompress_blocks(allsel, cn, typesize=ts, blocksize=bs, dst=out)
    assert bad == 4
    o = out.cpu().numpy()
    for i, b, lo, hi, d in rows:
        a = i * cn + b * bs
        assert np.array_equal(o[d:d + hi - lo], raw[a + lo:a + hi])
    _, bad = ctx.decompress_blocks(sel, cn, typesize=ts, blocksize=bs)
    assert bad == 0


# ---- the store ---------------------------------------------------------------------------------------------------------
S3, V3, SEED3, CHROM3 = 1000, 20_000, 31, 5


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    """1000 x 20 000 synthetic chr5 converted twice: default (direct .h5) and HHGT_KEEP_STORE=1 (store + exported .h5)"""
    from haplohyped_varawareml_amd.reader import write_bgzf_native
    from haplohyped_varawareml_amd.vcf_to_h5 import VCFtoHDF5Converter
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = tmp_path_factory.mktemp("cohort")
    tab = synth.variant_table(SEED3, V3, S3)
    text, _ = synth.render_fixed_numpy(f"chr{CHROM3}", tab, S3, seed=SEED3)
    (tmp / "vcf").mkdir()
    write_bgzf_native(str(tmp / "vcf" / f"chr{CHROM3}.filtered.vcf.gz"), text)
    samples = tmp / "samples.txt"
    samples.write_text("\n".join(synth.sample_names(S3)) + "\n")
    direct = VCFtoHDF5Converter("c", str(tmp / "vcf"), str(tmp / "a"), str(samples), 2, 1).run()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("HHGT_KEEP_STORE", "1")
        conv = VCFtoHDF5Converter("c", str(tmp / "vcf"), str(tmp / "b"), str(samples), 2, 1)
        exported = conv.run()
    assert os.path.isdir(conv.store_path)
    bits = synth.genotype_bits(SEED3, 0, V3, S3, tab["thr"]).astype(np.int8)    # [V, S, 2]
    return dict(paths=[direct, exported, conv.store_path], tab=tab, bits=bits)


def window_requests(rng, group):
    reqs = [(group, 5, 0, 0), (group, S3 - 1, V3 - 1, V3), (group, 999, 0, V3), (group, 0, V3, V3)]
    for edge in (4096, 8192, 12288, 16384):
        reqs.append((group, int(rng.integers(S3)), edge - int(rng.integers(1, 300)), edge + int(rng.integers(1, 300))))
    for _ in range(20):
        a = int(rng.integers(V3))
        reqs.append((group, int(rng.integers(S3)), a, min(V3, a + int(rng.integers(0, 3000)))))
    return reqs


def test_store_read_windows(ctx, cohort):
    from haplohyped_varawareml_amd.store import GenotypeStore
    g = f"chr_{CHROM3}"
    for path in cohort["paths"]:
        st = GenotypeStore(path, ctx=ctx)
        assert (st.meta["sc"], st.meta["vc"], st.meta["groups"][g]["n_scol"], st.meta["groups"][g]["n_vcol"]) == (64, 8192, 16, 3)
        reqs = window_requests(np.random.default_rng(7), g)
        rows = st.read_windows(reqs)
        assert len(rows) == len(reqs)
        for (_, s, a, b), r in zip(reqs, rows):
            assert r.is_cuda and r.dtype == torch.int8 and tuple(r.shape) == (b - a, 2)
            assert np.array_equal(r.cpu().numpy(), cohort["bits"][a:b, s]), (path, s, a, b)
        # a second call is served from the chunk cache
        n = st.stats["chunks_read"]
        again = st.read_windows(reqs[4:8])
        assert st.stats["chunks_read"] == n
        assert all(np.array_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(again, rows[4:8]))
        st.close()


def test_chunk_cache_keeps_its_budget(ctx, cohort):
    """a small byte budget: device memory held by the store stays near it across calls, and evicted chunks are read again"""
    import gc
    from haplohyped_varawareml_amd.store import GenotypeStore
    g = f"chr_{CHROM3}"
    st0 = GenotypeStore(cohort["paths"][2], ctx=ctx)
    off = np.load(os.path.join(cohort["paths"][2], g, "offsets.npy")).astype(np.int64)
    biggest = int(np.diff(off).max())
    budget = 4 * biggest
    st0.close()
    for path in cohort["paths"]:
        gc.collect()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        st = GenotypeStore(path, ctx=ctx, cache_bytes=budget)
        first = [(g, s, 0, V3) for s in (0, 64, 128)]                 # 9 chunks: more than the budget holds
        rows = st.read_windows(first)
        assert all(np.array_equal(r.cpu().numpy(), cohort["bits"][:, s]) for (_, s, _, _), r in zip(first, rows))
        del rows
        for q in range(12):                                          # rows of other sample chunks, one call each
            s = 64 * (3 + q % 12) + q
            r = st.read_windows([(g, s, 0, V3)])[0]
            assert np.array_equal(r.cpu().numpy(), cohort["bits"][:, s])
            del r
            gc.collect()
            assert st._cache_used <= budget
            # the cached chunks, each in an allocation of its own (rounded up by the allocator), and nothing else
            assert torch.cuda.memory_allocated() - base <= budget + 16 * 1024, (q, torch.cuda.memory_allocated() - base)
        n = st.stats["chunks_read"]
        rows = st.read_windows(first)                                # evicted long ago: read from the file again
        assert st.stats["chunks_read"] == n + 9
        assert all(np.array_equal(r.cpu().numpy(), cohort["bits"][:, s]) for (_, s, _, _), r in zip(first, rows))
        del rows
        st.close()
        gc.collect()
        assert torch.cuda.memory_allocated() - base <= 16 * 1024


def test_sample_row_decodes_only_its_blocks(ctx, cohort):
    from haplohyped_varawareml_amd.store import GenotypeStore
    g = f"chr_{CHROM3}"
    s = S3 - 3                                         # in the last, partial sample chunk (960..999)
    for path in cohort["paths"]:
        st = GenotypeStore(path, ctx=ctx)
        row = st.sample_row(g, synth.sample_names(S3)[s])
        assert row.dtype == np.int8 and np.array_equal(row, cohort["bits"][:, s])
        # its blocks: 8 KiB blocks, one row of a chunk = 8192 x 2 bytes = 2 blocks; the last column holds 20000 - 16384
        # variants = 7232 bytes of the row, one block
        bs = st.meta["blocksize"]
        want = sum(-(-2 * min(8192, V3 - v * 8192) // bs) for v in range(3))
        assert want == 5
        assert st.stats["blocks_decoded"] == want and st.stats["bytes_decoded"] == want * bs
        assert st.stats["chunks_read"] == 3
        st.close()


def test_fetch_region(ctx, cohort):
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    tab, bits = cohort["tab"], cohort["bits"]
    start0 = tab["pos"].astype(np.int64) - 1                  # 0-based, as start.npy
    donor = synth.sample_names(S3)[70]
    for path in cohort["paths"][:2]:
        r = VCFH5Reader(path, ctx=ctx)
        full = r.fetch_genotypes(donor, CHROM3)
        rng = np.random.default_rng(3)
        spans = [(0, 1 << 40), (int(start0[100]), int(start0[100]) + 1), (int(start0[8190]), int(start0[8200]) + 5),
                 (5, 5), (int(start0[-1]) + 1, int(start0[-1]) + 100)]
        spans += [tuple(sorted(rng.integers(0, int(start0[-1]) + 10, 2).tolist())) for _ in range(6)]
        for a, e in spans:
            got = r.fetch_region(donor, CHROM3, a, e)
            keep = (full["start"] >= a) & (full["start"] < e)
            assert got.dtype == full.dtype and np.array_equal(got, full[keep]), (a, e)
            m = (start0 >= a) & (start0 < e)
            assert np.array_equal(got["start"], start0[m]) and np.array_equal(got["phase1"], bits[m, 70, 0])
            assert np.array_equal(got["phase2"], bits[m, 70, 1])
        for args in ((donor, 6), ("nobody", CHROM3)):
            with pytest.raises(KeyError) as e1:
                r.fetch_genotypes(*args)
            with pytest.raises(KeyError) as e2:
                r.fetch_region(*args, 0, 100)
            assert str(e1.value) == str(e2.value)
        r.close()


# ---- the dataset at cohort shape ---------------------------------------------------------------------------------------
def test_dataset_at_cohort_shape(ctx, tmp_path):
    """2504 x 50 000 synthetic group, batch 8, seq_length 131072, cold cache: one-hot tensors against the documented rules
    fed from the generator, and no more blocks decoded than the items' ranges touch"""
    from haplohyped_varawareml_amd.reader import write_bgzf_native
    from haplohyped_varawareml_amd.vcf_to_h5 import VCFtoHDF5Converter
    from haplohyped_varawareml_amd.dataset import RandomHaplotypeDataset
    S, V, seed, L, B = 2504, 50_000, 77, 131072, 8
    tab = synth.variant_table(seed, V, S)
    text, n = ctx.synth_fixed("chr3", tab, S, seed=seed)
    (tmp_path / "vcf").mkdir()
    write_bgzf_native(str(tmp_path / "vcf" / "chr3.filtered.vcf.gz"), text[:n].cpu().numpy())
    del text
    names = synth.sample_names(S)
    (tmp_path / "samples.txt").write_text("\n".join(names) + "\n")
    h5 = VCFtoHDF5Converter("c", str(tmp_path / "vcf"), str(tmp_path / "out"), str(tmp_path / "samples.txt"), 2, 1).run()
    rng = np.random.default_rng(4)
    span = int(tab["pos"][-1]) + 1000
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, span)]
    np.savez(tmp_path / "ref.npz", chr3=ref)
    with open(tmp_path / "regions.bed", "w") as f:
        for a in sorted(rng.integers(0, span - 2000, 40).tolist()):
            f.write(f"chr3\t{a}\t{a + 1000}\n")
    ds = RandomHaplotypeDataset(str(tmp_path / "regions.bed"), h5, str(tmp_path / "ref.npz"), str(tmp_path / "samples.txt"),
                                seed=42, batch_size=B, seq_length=L, ctx=ctx)
    start0 = tab["pos"].astype(np.int64) - 1
    for _ in range(2):
        before = dict(ds.store.stats)
        h1, h2 = ds[0]
        st = {k: ds.store.stats[k] - before[k] for k in before}
        e1 = np.zeros((B, L, 5), np.float32)
        e2 = np.zeros_like(e1)
        bound = 0
        for b, it in enumerate(ds.last_items):
            a = it["start"]
            seq = np.full(L, ord("N"), np.uint8)
            e = min(a + L, len(ref))
            seq[:e - a] = ref[a:e]
            hs = [seq.copy(), seq.copy()]
            m = np.nonzero((start0 >= a) & (start0 < a + L))[0]
            assert (it["var_lo"], it["var_hi"]) == ((int(m[0]), int(m[-1]) + 1) if m.size else (it["var_lo"],) * 2)
            s = names.index(it["donor"])
            if m.size:
                gb = synth.genotype_bits(seed, int(m[0]), m.size, S, tab["thr"][m])[:, s]
                for k in (0, 1):
                    hs[k][start0[m] - a] = np.where(gb[:, k] == 1, tab["alt"][m], tab["ref"][m])
                # blocks the item's range touches: row bytes [2 lo, 2 hi) of each chunk column, in 8 KiB blocks
                r = s % 64
                for vcol in range(int(m[0]) // 8192, int(m[-1]) // 8192 + 1):
                    x0 = r * 16384 + 2 * (max(int(m[0]), vcol * 8192) - vcol * 8192)
                    x1 = r * 16384 + 2 * (min(int(m[-1]) + 1, (vcol + 1) * 8192) - vcol * 8192)
                    bound += (x1 - 1) // 8192 - x0 // 8192 + 1
            lut = np.full(256, 4, np.int64)
            lut[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4)
            for k, dst in ((0, e1), (1, e2)):
                dst[b, np.arange(L), lut[hs[k]]] = 1.0
        assert np.array_equal(h1.cpu().numpy(), e1) and np.array_equal(h2.cpu().numpy(), e2)
        assert 0 < st["blocks_decoded"] <= bound
        assert sum(it["var_hi"] - it["var_lo"] for it in ds.last_items) > B
    ds.close()
