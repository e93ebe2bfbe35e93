"""-m gpu: per-variant allele counts.  hhgt_count_alleles (one workgroup per (chunk, Blosc block column), counting in LDS)
against numpy on the raw bytes — shuffled, unshuffled and memcpyed chunks, random row masks and sub-ranges, calls
accumulating into one buffer, bad selections counted, unsupported geometry refused; GenotypeStore.allele_counts /
allele_frequencies, VCFH5Reader.allele_frequencies and the allele_freq CLI on converter output (the direct .h5, the
exported .h5, the directory store) against the synthetic generator's own genotypes; the encoder's multi-allelic mode."""
import os
import struct

import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd import device as dev, synth
from haplohyped_varawareml_amd._lib import HhgtError
from haplohyped_varawareml_amd.device import COUNT_SEL_DTYPE
from haplohyped_varawareml_amd.store import AC, AN, HET, HOM_ALT, plan_counts

pytestmark = pytest.mark.gpu


def np_counts(g):
    """int8 [S, V, 2] -> int64 [V, 4] (AN, AC, HET, HOM_ALT): the contract, restated"""
    a, b = g[..., 0], g[..., 1]
    out = np.zeros((g.shape[1], 4), np.int64)
    out[:, AN] = (a >= 0).sum(0) + (b >= 0).sum(0)
    out[:, AC] = (a == 1).sum(0) + (b == 1).sum(0)
    out[:, HET] = ((a >= 0) & (b >= 0) & (a != b)).sum(0)
    out[:, HOM_ALT] = ((a == 1) & (b == 1)).sum(0)
    return out


def genotype_bytes(rng, n):
    """mostly 0, some 1, a few -9, 2 and 3"""
    a = (rng.random(n) < 0.08).astype(np.int8)
    a[rng.random(n) < 0.01] = -9
    a[rng.random(n) < 0.004] = 2
    a[rng.random(n) < 0.002] = 3
    return a


def raw_blosc1(raw, typesize, blocksize, split):
    """an unshuffled Blosc-1 chunk with every stream stored as is (csize = stream size): what another writer may store"""
    nb = -(-raw.size // blocksize)
    hl = 16 + 4 * nb
    body, starts = b"", []
    for b in range(nb):
        starts.append(hl + len(body))
        blk = raw[b * blocksize:(b + 1) * blocksize].tobytes()
        ns = typesize if split and len(blk) == blocksize else 1
        n = len(blk) // ns
        for j in range(ns):
            body += struct.pack("<I", n) + blk[j * n:(j + 1) * n]
    flags = (1 << 5) | (0 if split else 0x10)
    hdr = struct.pack("<BBBBIII", 2, 1, flags, typesize, raw.size, blocksize, hl + len(body))
    return np.frombuffer(hdr + struct.pack(f"<{nb}I", *starts) + body, np.uint8)


GEOMS = [  # sc, vc, blocksize: two blocks per row (the store's), one block per row, unsplit small blocks (one wave)
    (64, 8192, 8192),
    (40, 4096, 8192),
    (20, 96, 64),
]


def kernel_chunks(ctx, rng, sc, vc, bs, fmt):
    """5 chunks: 3 compressed (shuffled), 1 memcpyed, 1 unshuffled (split when the blocks are) -> (raw [n, sc, vc, 2],
    device buffer, offsets)"""
    cn = sc * vc * 2
    raw = genotype_bytes(rng, 4 * cn)
    raw[3 * cn:] = rng.integers(-128, 128, cn, dtype=np.int8)                # incompressible: stored memcpyed
    src = torch.from_numpy(raw.view(np.uint8)).to(ctx.device)
    dst, off, total = ctx.compress(src, cn, typesize=2, blocksize=bs, fmt=fmt)
    off = off.cpu().numpy().astype(np.int64)
    buf = dst[:total].cpu().numpy()
    assert buf[off[3] + 2] & 0x2 and not buf[off[0] + 2] & 0x2
    extra_raw = genotype_bytes(rng, cn)
    extra = raw_blosc1(extra_raw.view(np.uint8), 2, bs, split=(bs // 2 >= 128))
    allb = np.concatenate([buf, extra])
    off = np.append(off, off[-1] + extra.size)
    d = torch.from_numpy(allb).to(ctx.device)
    return np.concatenate([raw, extra_raw]).reshape(5, sc, vc, 2), d, off


def random_count_sel(rng, d, off, sc, vc, bs, n, n_out):
    parts, vb = vc * 2 // bs, bs // 2
    sel = np.zeros(n, COUNT_SEL_DTYPE)
    for j in range(n):
        i, p = int(rng.integers(len(off) - 1)), int(rng.integers(parts))
        mask = int(rng.integers(0, 1 << 63)) | (int(rng.integers(0, 2)) << 63)
        if j % 5 == 0:
            mask = (1 << sc) - 1                                          # every row
        mask &= (1 << sc) - 1
        lo, hi = (0, vb) if j % 3 == 0 else sorted(int(x) for x in rng.choice(vb + 1, 2, replace=False))
        sel[j] = (d.data_ptr() + int(off[i]), int(off[i + 1] - off[i]), mask, int(rng.integers(0, n_out - (hi - lo) + 1)),
                  p, lo, hi, 0)
    return sel


def expected(raw, off_ptr0, sel, sc, vc, bs, n_out):
    want = np.zeros((n_out, 4), np.int64)
    vb = bs // 2
    for s in sel:
        i = int(np.searchsorted(off_ptr0, int(s["src_ptr"])))
        rows = [r for r in range(sc) if int(s["row_mask"]) >> r & 1]
        v0 = int(s["part"]) * vb
        if rows:
            g = raw[i, rows, v0 + int(s["lo"]):v0 + int(s["hi"])]
            want[int(s["out_row"]):int(s["out_row"]) + int(s["hi"] - s["lo"])] += np_counts(g)
    return want


@pytest.mark.parametrize("fmt", [dev.BLOSC1, dev.BLOSC2])
@pytest.mark.parametrize("sc,vc,bs", GEOMS)
def test_kernel_counts_match_numpy(ctx, fmt, sc, vc, bs):
    rng = np.random.default_rng(sc * 7 + vc + bs + fmt)
    raw, d, off = kernel_chunks(ctx, rng, sc, vc, bs, fmt)
    n_out = 3 * bs
    sel = random_count_sel(rng, d, off, sc, vc, bs, 60, n_out)
    ptrs = d.data_ptr() + off[:-1]
    want = expected(raw, ptrs, sel, sc, vc, bs, n_out)
    counts, bad = ctx.count_alleles(sel, sc, vc, n_out=n_out, blocksize=bs)
    assert bad == 0 and counts.dtype == torch.int32 and tuple(counts.shape) == (n_out, 4)
    assert np.array_equal(counts.cpu().numpy(), want)
    # every chunk kind, whole rows: the memcpyed chunk (3) and the unshuffled one (4) included
    for i in range(5):
        s = np.zeros(vc * 2 // bs, COUNT_SEL_DTYPE)
        for p in range(len(s)):
            s[p] = (d.data_ptr() + int(off[i]), int(off[i + 1] - off[i]), (1 << sc) - 1, p * (bs // 2), p, 0, bs // 2, 0)
        c, bad = ctx.count_alleles(s, sc, vc, n_out=vc, blocksize=bs)
        assert bad == 0 and np.array_equal(c.cpu().numpy(), np_counts(raw[i])), i
    # a second call adds into the same buffer
    half = len(sel) // 2
    acc = torch.zeros((n_out, 4), dtype=torch.int32, device=ctx.device)
    ctx.count_alleles(sel[:half], sc, vc, blocksize=bs, counts=acc)
    _, bad = ctx.count_alleles(sel[half:], sc, vc, blocksize=bs, counts=acc)
    assert bad == 0 and np.array_equal(acc.cpu().numpy(), want)
    ctx.count_alleles(sel, sc, vc, blocksize=bs, counts=acc)
    assert np.array_equal(acc.cpu().numpy(), 2 * want)


def test_bad_selections_counted(ctx):
    sc, vc, bs = 64, 8192, 8192
    rng = np.random.default_rng(11)
    raw, d, off = kernel_chunks(ctx, rng, sc, vc, bs, dev.BLOSC1)
    n_out = 2 * bs
    sel = random_count_sel(rng, d, off, sc, vc, bs, 20, n_out)
    good = expected(raw, d.data_ptr() + off[:-1], sel, sc, vc, bs, n_out)
    extra = np.zeros(5, COUNT_SEL_DTYPE)
    size0 = int(off[1] - off[0])
    extra[0] = (d.data_ptr(), size0 - 100, 1, 0, 0, 0, 10, 0)                 # truncated chunk
    extra[1] = (d.data_ptr(), size0, 1, 0, 2, 0, 10, 0)                       # part past the row's blocks
    extra[2] = (d.data_ptr(), size0, 1, 0, 0, 5, 5, 0)                        # lo == hi
    extra[3] = (d.data_ptr(), size0, 1, 0, 0, 0, bs // 2 + 1, 0)              # hi past the block
    extra[4] = (d.data_ptr(), size0, 1, n_out - 5, 0, 0, 10, 0)               # past the end of d_counts
    counts, bad = ctx.count_alleles(np.concatenate([sel[:7], extra, sel[7:]]), sc, vc, n_out=n_out, blocksize=bs)
    assert bad == 5
    assert np.array_equal(counts.cpu().numpy(), good)      # bad selections with a bad header or bounds add nothing


def test_unsupported_geometry(ctx):
    sel = np.zeros(1, COUNT_SEL_DTYPE)
    for kw in (dict(sc=64, vc=8192, typesize=3, blocksize=8190), dict(sc=64, vc=8192, typesize=2, blocksize=6000),
               dict(sc=65, vc=8192, typesize=2, blocksize=8192), dict(sc=64, vc=16384, typesize=2, blocksize=16384)):
        counts = torch.zeros((16, 4), dtype=torch.int32, device=ctx.device)
        with pytest.raises(HhgtError) as e:
            ctx.count_alleles(sel, kw["sc"], kw["vc"], typesize=kw["typesize"], blocksize=kw["blocksize"], counts=counts)
        assert e.value.code == -1 and "count_alleles" in str(e.value)


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
    return dict(paths=[direct, exported, conv.store_path], tab=tab, bits=bits.transpose(1, 0, 2).copy(), tmp=tmp)


def test_store_allele_counts(ctx, cohort):
    from haplohyped_varawareml_amd.store import GenotypeStore
    g, G = f"chr_{CHROM3}", cohort["bits"]                                        # G: [S, V, 2]
    rng = np.random.default_rng(9)
    sub = np.sort(rng.choice(S3, 37, replace=False))
    names = synth.sample_names(S3)
    queries = [(None, 0, V3), (sub, 0, V3), ([S3 - 1], 0, V3), ([names[i] for i in sub], 4000, 12500),
               (None, 4095, 4097), (None, 8191, 8193), (sub, 16383, V3), (None, 7, 7), ([], 0, V3)]
    for path in cohort["paths"]:
        st = GenotypeStore(path, ctx=ctx)
        assert (st.meta["sc"], st.meta["vc"]) == (64, 8192)
        for samples, a, b in queries:
            c = st.allele_counts(g, samples, a, b)
            assert c.is_cuda and c.dtype == torch.int32 and tuple(c.shape) == (b - a, 4)
            idx = np.arange(S3) if samples is None else np.array([st._sample_index(x) for x in samples], np.int64)
            want = np_counts(G[idx, a:b]) if len(idx) else np.zeros((b - a, 4), np.int64)
            assert np.array_equal(c.cpu().numpy(), want), (path, a, b)
            f = st.allele_frequencies(g, samples, a, b).cpu().numpy()
            with np.errstate(divide="ignore", invalid="ignore"):
                wf = (want[:, AC] / want[:, AN]).astype(np.float32)
            assert f.dtype == np.float32 and np.array_equal(np.isnan(f), want[:, AN] == 0)
            assert np.array_equal(f[want[:, AN] > 0], wf[want[:, AN] > 0])
        # blocks: every selected row of every touched block column, once
        st.stats.update(count_blocks=0)
        st.allele_counts(g)
        assert st.stats["count_blocks"] == S3 * 5              # 20 000 variants = 2 + 2 + 1 blocks of 4096 per row
        st.close()


def test_store_counts_deterministic_and_slabbed(ctx, cohort):
    from haplohyped_varawareml_amd.store import GenotypeStore
    g = f"chr_{CHROM3}"
    st = GenotypeStore(cohort["paths"][0], ctx=ctx)
    a = st.allele_counts(g).cpu().numpy()
    b = st.allele_counts(g).cpu().numpy()
    assert np.array_equal(a, b)
    n = st.stats["count_compressed_bytes_read"]
    c = st.allele_counts(g, slab_bytes=300_000).cpu().numpy()     # many slabs: a few chunks each
    assert np.array_equal(a, c)
    assert st.stats["count_compressed_bytes_read"] - n == (n // 2)   # the same chunks read, once each, per call
    st.close()


def test_count_leaves_read_cache_alone(ctx, cohort):
    from haplohyped_varawareml_amd.store import GenotypeStore
    g = f"chr_{CHROM3}"
    for path in cohort["paths"]:
        st = GenotypeStore(path, ctx=ctx)
        batch = [(g, s, 1000 * s % 15000, 1000 * s % 15000 + 3000) for s in (3, 70, 500, 999)]
        first = [r.cpu().numpy() for r in st.read_windows(batch)]
        keys, used, n = list(st._cache), st._cache_used, st.stats["chunks_read"]
        st.allele_counts(g)
        assert list(st._cache) == keys and st._cache_used == used
        again = [r.cpu().numpy() for r in st.read_windows(batch)]
        assert st.stats["chunks_read"] == n                      # served from the cache: nothing read from the file
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        # cached chunks are used by the count, not read again
        m = st.stats["count_compressed_bytes_read"]
        st.allele_counts(g, v_lo=0, v_hi=100, samples=[3])
        assert st.stats["count_compressed_bytes_read"] == m
        st.close()


def test_reader_allele_frequencies(ctx, cohort):
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    tab, G = cohort["tab"], cohort["bits"]
    start0 = tab["pos"].astype(np.int64) - 1
    names = synth.sample_names(S3)
    donors = [names[i] for i in (0, 5, 64, 999)]
    for path in cohort["paths"][:2]:
        r = VCFH5Reader(path, ctx=ctx)
        for a, e, ds in ((None, None, None), (int(start0[4000]), int(start0[8300]) + 1, donors), (5, 5, None),
                         (int(start0[-10]), None, donors[:1])):
            rec = r.allele_frequencies(CHROM3, a, e, donor_ids=ds)
            m = np.ones(V3, bool)
            if a is not None:
                m &= start0 >= a
            if e is not None:
                m &= start0 < e
            idx = np.arange(S3) if ds is None else np.array([names.index(x) for x in ds])
            want = np_counts(G[idx][:, m])
            assert np.array_equal(rec["start"], start0[m]) and np.array_equal(rec["stop"], start0[m] + 1)
            assert np.array_equal(rec["ref"], tab["ref"][m].view("S1"))
            assert np.array_equal(rec["alt"], tab["alt"][m].view("S1"))
            assert (rec["chrom"] == f"chr{CHROM3}".encode()).all()
            for f, col in (("an", AN), ("ac", AC), ("het", HET), ("hom_alt", HOM_ALT)):
                assert np.array_equal(rec[f], want[:, col]), f
            with np.errstate(divide="ignore", invalid="ignore"):
                wf = (want[:, AC] / want[:, AN]).astype(np.float32)
            assert np.array_equal(np.isnan(rec["af"]), want[:, AN] == 0)
            assert np.array_equal(rec["af"][want[:, AN] > 0], wf[want[:, AN] > 0])
        for chrom, ds in ((6, None), (CHROM3, ["nobody"])):
            with pytest.raises(KeyError) as e1:
                r.allele_frequencies(chrom, donor_ids=ds)
            with pytest.raises(KeyError) as e2:
                r.fetch_genotypes((ds or [names[0]])[0], chrom)
            assert str(e1.value) == str(e2.value)
        r.close()


def test_cli_tsv(ctx, cohort):
    from click.testing import CliRunner
    from haplohyped_varawareml_amd.allele_freq import HEADER, format_rows, main
    tab, G, tmp = cohort["tab"], cohort["bits"], cohort["tmp"]
    names = synth.sample_names(S3)
    pick = [names[i] for i in range(0, S3, 7)]
    (tmp / "pick.txt").write_text("\n".join(pick) + "\n")
    pos = tab["pos"].astype(np.int64)
    for args, idx, m in (
            ([], np.arange(S3), np.ones(V3, bool)),
            (["--sample_list", str(tmp / "pick.txt"), "--region", f"chr{CHROM3}:{pos[100]}-{pos[9000]}"],
             np.arange(0, S3, 7), (pos >= pos[100]) & (pos <= pos[9000])),
            (["--chromosome", str(CHROM3)], np.arange(S3), np.ones(V3, bool))):
        out = tmp / "freq.tsv"
        res = CliRunner().invoke(main, ["--h5", cohort["paths"][0], "--out", str(out)] + args)
        assert res.exit_code == 0, res.output
        want = HEADER + format_rows(np.full(int(m.sum()), f"chr{CHROM3}"), pos[m], tab["ref"][m], tab["alt"][m],
                                    np_counts(G[idx][:, m]))
        assert out.read_text() == want


# ---- the encoder's multi-allelic mode ----------------------------------------------------------------------------------
def test_counts_of_encoded_mixed_vcf(ctx):
    """C4-style text (missing, half-missing and multi-allelic calls) encoded with set_keep_multiallelic(True), compressed,
    counted: against the generator's own calls"""
    S, V, seed = 130, 12_000, 43
    t = synth.mixed_table(seed, V, S)
    kept = np.nonzero(t["kept"] | (t["n_alt"] > 1))[0]                 # keep mode: every SNP site, multi-allelic too
    text, n, _ = ctx.synth_mixed("chr4", t, S, seed=seed)
    lay = dev.make_layout(S, len(kept), sc=64, vc=8192)
    ctx.set_keep_multiallelic(True)
    try:
        res = ctx.encode_text(text[:n], S, region="chr4", layout=lay)
    finally:
        ctx.set_keep_multiallelic(False)
    assert res.n_kept == len(kept)
    want_G = synth.mixed_expected_G(seed, t, S, kept)                       # [S, n_kept, 2]
    assert (want_G >= 2).any() and (want_G == -9).any()
    assert ((want_G[..., 0] == -9) != (want_G[..., 1] == -9)).any()       # half-missing calls
    cn = 64 * 8192 * 2
    dst, off, total = ctx.compress(res.G, cn, typesize=2, blocksize=8192, fmt=dev.BLOSC1)
    off = off.cpu().numpy().astype(np.int64)
    n_sc = -(-S // 64)
    rng = np.random.default_rng(1)
    for samples in (np.arange(S), np.sort(rng.choice(S, 50, replace=False))):
        plan = plan_counts(samples, S, 64, 8192, len(kept), 0, len(kept))
        sel = np.zeros(len(plan), COUNT_SEL_DTYPE)
        cid = plan["vcol"] * n_sc + plan["scol"]
        sel["src_ptr"] = dst.data_ptr() + off[cid]
        sel["src_bytes"] = off[cid + 1] - off[cid]
        for f in ("row_mask", "out_row", "part", "lo", "hi"):
            sel[f] = plan[f]
        counts, bad = ctx.count_alleles(sel, 64, 8192, n_out=len(kept), blocksize=8192)
        assert bad == 0
        assert np.array_equal(counts.cpu().numpy(), np_counts(want_G[samples]))
