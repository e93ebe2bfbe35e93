"""-m gpu: the device chunk decoder (decode.hip: blosc_header, decode_block_lds, lz4_wave_decode, unshuffle_range) on
streams our encoder never writes, judged by independent decoders: liblz4 on hand-built boundary streams
(tests/lz4_streams.py, itself pinned against liblz4 by tests/test_lz4_streams.py) and c-blosc 1.21 on its own lz4 / lz4hc
chunks.  Every case runs through hhgt_decompress_chunks with many chunks per launch and 0xA5 guards around d_dst, and
through hhgt_decompress_blocks over random byte ranges; the allele counter reads c-blosc lz4hc chunks on its three
paths.  n_bad is pinned to its definition: 1 per refused chunk header, 1 per corrupt block, 1 per bad selection."""
import gzip
import os

import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd._lib import HhgtError
from oracle import oracle
from tests import extlibs
from tests import lz4_streams as L
from tests.test_gpu_allele_counts import expected as expected_counts, random_count_sel
from tests.test_gpu_window_read import genotype_like, random_selections

pytestmark = pytest.mark.gpu

need_lz4 = pytest.mark.skipif(not extlibs.have_lz4(), reason="liblz4 not loadable (independent leg absent)")
need_blosc = pytest.mark.skipif(not extlibs.have_blosc(), reason="c-blosc not loadable (independent leg absent)")

GUARD = 4096


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def pack(chunks):
    off = np.zeros(len(chunks) + 1, np.int64)
    off[1:] = np.cumsum([c.size for c in chunks])
    return np.concatenate(chunks), off


def decode_all(ctx, chunks, cn, ts, bs):
    """one hhgt_decompress_chunks launch over all chunks, d_dst between 0xA5 guards -> (out [n, cn], n_bad, src, off)"""
    flat, off = pack(chunks)
    src, n = to_dev(flat), len(chunks)
    buf = torch.full((2 * GUARD + n * cn,), 0xA5, dtype=torch.uint8, device="cuda")
    _, bad = ctx.decompress(src, to_dev(off), n, cn, typesize=ts, blocksize=bs, dst=buf[GUARD:GUARD + n * cn])
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD] == 0xA5) and np.all(h[-GUARD:] == 0xA5), "write outside d_dst"
    return h[GUARD:-GUARD].reshape(n, cn), bad, src, off


def gather(ctx, rng, src, off, cn, ts, bs, want, bad=lambda i, b: False, n=40):
    """random [lo, hi) selections through hhgt_decompress_blocks: a selection of a bad (chunk, block) counts once, every
    other one equals want[i]; the destination's guards stay intact"""
    sel, rows, size = random_selections(rng, src, off, cn, bs, n, aligned=8)
    buf = torch.full((size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    _, nbad = ctx.decompress_blocks(sel, cn, typesize=ts, blocksize=bs, dst=buf[GUARD:GUARD + size])
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD] == 0xA5) and np.all(h[-GUARD:] == 0xA5), "write outside d_dst"
    o = h[GUARD:-GUARD]
    assert nbad == sum(1 for i, b, *_ in rows if bad(i, b))
    for i, b, lo, hi, d in rows:
        if not bad(i, b):
            assert np.array_equal(o[d:d + hi - lo], want[i][b * bs + lo:b * bs + hi]), (i, b, lo, hi)


def lz4_ref(stream, n):
    out = extlibs.lz4_decompress(stream, n)
    assert out.size == n
    return out


# ---- (a) boundary streams, valid ----------------------------------------------------------------------------------------
@need_lz4
@pytest.mark.parametrize("n", [32768, 65536])
def test_boundary_streams_typesize1(ctx, n):
    """one boundary stream per chunk (one block of n bytes, typesize 1), the two header formats alternating"""
    table = [(name, s) for name, s, kind in L.boundary_streams(n) if kind == "valid"]
    chunks = [L.frame([[s]], 1, n, n, fmt=1 + k % 2, shuffle=False) for k, (_, s) in enumerate(table)]
    want = [lz4_ref(s, n) for _, s in table]
    out, bad, src, off = decode_all(ctx, chunks, n, 1, n)
    assert bad == 0
    for k, (name, _) in enumerate(table):
        assert np.array_equal(out[k], want[k]), name
    gather(ctx, np.random.default_rng(n), src, off, n, 1, n, want, n=60)


@need_lz4
def test_boundary_streams_typesize2_split(ctx):
    """typesize 2, split: the two planes of a block are different boundary streams; the chunk decodes to the interleave
    of liblz4's outputs"""
    bs = 32768
    table = [(name, s) for name, s, kind in L.boundary_streams(bs // 2, seed=5) if kind == "valid"]
    chunks, want = [], []
    for k in range(len(table)):
        (n0, s0), (n1, s1) = table[k], table[(k + 7) % len(table)]
        chunks.append(L.frame([[s0, s1]], 2, bs, bs, fmt=1 + k % 2))
        w = np.empty(bs, np.uint8)
        w[0::2], w[1::2] = lz4_ref(s0, bs // 2), lz4_ref(s1, bs // 2)
        want.append(w)
    out, bad, src, off = decode_all(ctx, chunks, bs, 2, bs)
    assert bad == 0
    for k in range(len(table)):
        assert np.array_equal(out[k], want[k]), (table[k][0], table[(k + 7) % len(table)][0])
    gather(ctx, np.random.default_rng(2), src, off, bs, 2, bs, want, n=60)


@need_lz4
@pytest.mark.parametrize("ts", [1, 2])
def test_one_byte_last_block(ctx, ts):
    """chunks of 32 KiB + 1 byte: a boundary-stream block, then a 1-byte block (stored, csize == 1)"""
    bs, cn = 32768, 32769
    table = [s for _, s, kind in L.boundary_streams(bs, seed=9) if kind == "valid"][::7]
    if ts == 2:
        half = [s for _, s, kind in L.boundary_streams(bs // 2, seed=9) if kind == "valid"][::7]
    chunks, want = [], []
    for k, s in enumerate(table):
        tail = np.array([k * 37 % 256], np.uint8)
        if ts == 1:
            chunks.append(L.frame([[s], [tail]], 1, bs, cn, fmt=1 + k % 2, shuffle=False))
            w = lz4_ref(s, bs)
        else:
            s0, s1 = half[k % len(half)], half[(k + 3) % len(half)]
            chunks.append(L.frame([[s0, s1], [tail]], 2, bs, cn, fmt=1 + k % 2))
            w = np.empty(bs, np.uint8)
            w[0::2], w[1::2] = lz4_ref(s0, bs // 2), lz4_ref(s1, bs // 2)
        want.append(np.concatenate([w, tail]))
    out, bad, src, off = decode_all(ctx, chunks, cn, ts, bs)
    assert bad == 0
    for k in range(len(chunks)):
        assert np.array_equal(out[k], want[k]), k
    gather(ctx, np.random.default_rng(3), src, off, cn, ts, bs, want)


# ---- (b) malformed streams ----------------------------------------------------------------------------------------------
@need_lz4
def test_malformed_streams_flagged_per_block(ctx, record_property):
    """Malformed streams in one block of a chunk, between valid chunks, in one launch.  n_bad = 1 per corrupt block
    exactly; the other blocks of those chunks and every neighbour decode exactly; the guards stay.  Streams that only
    break LZ4's end-of-block rules: the device either flags the block or equals the plain interpreter (recorded)."""
    bs, cn, ts = 4096, 4 * 4096 + 1000, 1
    nblocks = 5
    rng = np.random.default_rng(11)
    good = [s for _, s, kind in L.boundary_streams(bs, seed=12) if kind == "valid"]
    good_tail = [s for _, s, kind in L.boundary_streams(1000, seed=13) if kind == "valid"]
    pick = lambda: good[int(rng.integers(len(good)))]  # noqa: E731
    bad_streams = L.malformed_streams(bs)
    eob = [(name, s) for name, s, kind in L.boundary_streams(bs, seed=14) if kind == "eob"]
    chunks, want, bad_blocks, eob_blocks = [], [], set(), {}

    def valid_blocks():
        return [[pick()] for _ in range(4)] + [[good_tail[int(rng.integers(len(good_tail)))]]]

    def expect_of(blocks, skip):
        return np.concatenate([(L.interpret(b[0], bs if k < 4 else 1000) if k not in skip else
                                np.zeros(bs if k < 4 else 1000, np.uint8)) for k, b in enumerate(blocks)])

    def push(blocks, fmt, skip=()):
        chunks.append(L.frame(blocks, ts, bs, cn, fmt=fmt, shuffle=False))
        want.append(expect_of(blocks, skip))
        return len(chunks) - 1

    push(valid_blocks(), 1)
    for k, (name, s) in enumerate(bad_streams):            # one malformed stream per chunk, in block k % 4
        blocks = valid_blocks()
        blocks[k % 4] = [s]
        i = push(blocks, 1 + k % 2, skip=(k % 4,))
        bad_blocks.add((i, k % 4))
        push(valid_blocks(), 2 - k % 2)
    blocks = valid_blocks()                                  # two corrupt blocks in one chunk: counted twice
    blocks[1], blocks[3] = [bad_streams[0][1]], [bad_streams[1][1]]
    i = push(blocks, 1, skip=(1, 3))
    bad_blocks |= {(i, 1), (i, 3)}
    # stream-table corruption: csize 0, csize > neblock, a bstart past the end (patched after framing)
    for what in ("csize0", "csize_gt_neblock", "bstart_past_end"):
        blocks = valid_blocks()
        b = {"csize0": 2, "csize_gt_neblock": 0, "bstart_past_end": 3}[what]
        i = push(blocks, 1, skip=(b,))
        ck = chunks[i]
        hl = 16
        bstart = int(ck[hl + 4 * b:hl + 4 * b + 4].view("<u4")[0])
        if what == "bstart_past_end":
            ck[hl + 4 * b:hl + 4 * b + 4] = np.array([ck.size + 8], "<u4").view(np.uint8)
        else:
            ck[bstart:bstart + 4] = np.array([0 if what == "csize0" else bs + 1], "<u4").view(np.uint8)
        bad_blocks.add((i, b))
        push(valid_blocks(), 2)
    for k, (name, s) in enumerate(eob):
        blocks = valid_blocks()
        blocks[k % 4] = [s]
        i = push(blocks, 1 + k % 2)                          # expectation: the interpreter's bytes
        eob_blocks[(i, k % 4)] = name
    out, bad, src, off = decode_all(ctx, chunks, cn, ts, bs)
    flagged = {}
    for (i, b), name in eob_blocks.items():
        blk = out[i, b * bs:(b + 1) * bs]
        same = np.array_equal(blk, want[i][b * bs:(b + 1) * bs])
        assert same or np.all(blk == 0xA5), name               # flagged: the block is not written at all
        flagged[name] = not same
    record_property("end_of_block_streams_flagged", flagged)
    print("end-of-block-rule streams, flagged by the device:", flagged)
    assert bad == len(bad_blocks) + sum(flagged.values())
    for i in range(len(chunks)):
        for b in range(nblocks):
            if (i, b) in bad_blocks or ((i, b) in eob_blocks and flagged[eob_blocks[(i, b)]]):
                continue
            a, e = b * bs, min(cn, (b + 1) * bs)
            assert np.array_equal(out[i, a:e], want[i][a:e]), (i, b)
    is_bad = lambda i, b: (i, b) in bad_blocks or ((i, b) in eob_blocks and flagged[eob_blocks[(i, b)]])  # noqa: E731
    gather(ctx, np.random.default_rng(12), src, off, cn, ts, bs, want, bad=is_bad, n=120)


# ---- (c) c-blosc 1.21 chunks --------------------------------------------------------------------------------------------
NB = 70001                        # two blocks of c-blosc's 64 KiB split blocks (the second short), many of smaller ones


def sample_data(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "genotype":
        return genotype_like(rng, n)
    if kind == "onehot":
        rows = np.zeros((n // 4 + 1, 4), np.uint8)
        rows[np.arange(rows.shape[0]), rng.integers(0, 4, rows.shape[0])] = 1
        return rows.reshape(-1)[:n].copy()
    if kind == "text":
        text = gzip.open(os.path.join(os.path.dirname(__file__), "golden", "chr22.filtered.vcf.gz"), "rb").read()
        return np.frombuffer((text * (n // len(text) + 1))[:n], np.uint8).copy()
    return rng.integers(0, 256, n, dtype=np.uint8)         # random: c-blosc stores it memcpyed (tight destination)


def blosc_chunk(data, ts, bs, clevel, shuffle, cname, tight=False):
    ck = extlibs.blosc1_compress(data, ts, bs, clevel, shuffle, cname, tight=tight)
    assert np.array_equal(extlibs.blosc1_decompress(ck, data.size), data)
    return ck


def decode_groups(ctx, items, nbytes, label):
    """items: [(typesize, chunk, data)] -> one launch (and one gather) per (typesize, header blocksize); blocks over
    64 KiB must be refused by the host.  Returns the number of chunks decoded on the device."""
    groups = {}
    for ts, ck, data in items:
        groups.setdefault((ts, int(ck[8:12].view("<u4")[0])), {})[ck.tobytes()] = data
    done = 0
    for (ts, hbs), chunks in sorted(groups.items()):
        cks = [np.frombuffer(k, np.uint8) for k in chunks]
        if hbs > 65536:
            with pytest.raises(HhgtError, match="does not fit LDS"):
                decode_all(ctx, cks, nbytes, ts, hbs)
            continue
        want = list(chunks.values())
        out, bad, src, off = decode_all(ctx, cks, nbytes, ts, hbs)
        assert bad == 0, (label, ts, hbs)
        for k in range(len(cks)):
            assert np.array_equal(out[k], want[k]), (label, ts, hbs, k, cks[k][:4])
        gather(ctx, np.random.default_rng(ts * 7 + hbs), src, off, nbytes, ts, hbs, want, n=24)
        done += len(cks)
    return done


@need_blosc
def test_cblosc_sweep(ctx):
    """c-blosc 1.21 lz4 and lz4hc, clevels 1 / 5 / 9, shuffle off / on, typesizes 1 .. 35, requested blocksizes 1 .. 32
    KiB (c-blosc widens split blocks to 64 KiB or more: the header says which), four kinds of data"""
    data = {k: sample_data(k, NB, 1) for k in ("genotype", "onehot", "text", "random")}
    items = []
    for ts in (1, 2, 3, 4, 8, 16, 17, 35):
        for bs in (1024, 2048, 4096, 8192, 16384, 32768):
            for cname in (b"lz4", b"lz4hc"):
                for clevel in (1, 5, 9):
                    for shuffle in (0, 1):
                        for kind, d in data.items():
                            if clevel != 5 and kind in ("onehot", "random"):
                                continue
                            items.append((ts, blosc_chunk(d, ts, bs, clevel, shuffle, cname, kind == "random"), d))
    flags = {int(ck[2]) for _, ck, _ in items}
    assert any(f & L.MEMCPYED for f in flags) and any(f & L.DONT_SPLIT for f in flags)
    assert any(not f & (L.DONT_SPLIT | L.MEMCPYED) for f in flags)
    assert decode_groups(ctx, items, NB, "sweep") > 100


@need_blosc
def test_cblosc_never_split(ctx):
    """splitmode NEVER: c-blosc keeps the requested blocksize and writes one stream per block, typesizes 2 .. 16"""
    data = {k: sample_data(k, NB, 2) for k in ("genotype", "text")}
    items = []
    with extlibs.splitmode(extlibs.BLOSC_NEVER_SPLIT):
        for ts in (2, 3, 4, 8, 16):
            for bs in (1024, 2048, 4096, 8192, 16384, 32768):
                for cname in (b"lz4", b"lz4hc"):
                    for shuffle in (0, 1):
                        for kind, d in data.items():
                            ck = blosc_chunk(d, ts, bs, 5, shuffle, cname)
                            assert ck[2] & L.DONT_SPLIT and int(ck[8:12].view("<u4")[0]) == bs - bs % ts
                            items.append((ts, ck, d))
    assert decode_groups(ctx, items, NB, "never-split") == len(items)


@need_lz4
def test_liblz4_levels_framed(ctx):
    """liblz4 HC levels 1 .. 12 and fast accelerations 1 .. 16 on the byte planes, framed split, both header formats"""
    bs, cn = 8192, 3 * 8192 + 1400
    coders = [("hc", lv) for lv in range(1, 13)] + [("fast", a) for a in range(1, 17)]
    chunks, want = [], []
    for k, (kind, lv) in enumerate(coders):
        data = sample_data("genotype" if k % 3 else "text", cn, 100 + k)
        comp = (lambda b: extlibs.lz4_compress_hc(b, lv)) if kind == "hc" else (lambda b: extlibs.lz4_compress_fast(b, lv))
        blocks = []
        for b in range(-(-cn // bs)):
            sh = oracle.shuffle(data[b * bs:(b + 1) * bs], 2)
            parts = [sh[:bs // 2], sh[bs // 2:]] if sh.size == bs else [sh]
            blocks.append([c if (c := comp(p)).size < p.size else p for p in parts])
        chunks.append(L.frame(blocks, 2, bs, cn, fmt=1 + k % 2))
        if k % 2 == 0 and extlibs.have_blosc():
            assert np.array_equal(extlibs.blosc1_decompress(chunks[-1], cn), data)
        want.append(data)
    out, bad, src, off = decode_all(ctx, chunks, cn, 2, bs)
    assert bad == 0
    for k in range(len(chunks)):
        assert np.array_equal(out[k], want[k]), coders[k]
    gather(ctx, np.random.default_rng(4), src, off, cn, 2, bs, want, n=60)


# ---- (d) refusals -------------------------------------------------------------------------------------------------------
@need_blosc
def test_refused_chunks_counted_once(ctx):
    """bitshuffle, blosclz / zlib / zstd, and headers whose typesize / nbytes / cbytes / blocksize differ from the call's:
    each chunk counts once (each selection of it once), valid neighbours decode exactly"""
    bs, cn, ts = 8192, 3 * 8192 + 1400, 2
    data = [sample_data("genotype" if k % 2 else "text", cn, 200 + k) for k in range(24)]
    chunks, want, refused = [], [], set()

    def good(d, k):
        if k % 3 == 0:      # c-blosc's own lz4 streams, re-framed behind a Blosc2 header
            hdr, blocks = L.streams_of(blosc_chunk(d, ts, bs, 5, 1, b"lz4"))
            return L.frame(blocks, ts, bs, cn, fmt=2, split=not hdr["flags"] & L.DONT_SPLIT)
        return blosc_chunk(d, ts, bs, 5, k % 2, b"lz4hc")

    with extlibs.splitmode(extlibs.BLOSC_NEVER_SPLIT):
        bads = [blosc_chunk(data[0], ts, bs, 5, 2, b"lz4"),          # bitshuffle
                blosc_chunk(data[1], ts, bs, 5, 1, b"blosclz"),
                blosc_chunk(data[2], ts, bs, 5, 1, b"zlib"),
                blosc_chunk(data[3], ts, bs, 5, 1, b"zstd")]
        assert bads[0][2] & L.DOBITSHUFFLE and [(c[2] >> 5) & 7 for c in bads[1:]] == [0, 3, 4]
        assert not any(c[2] & L.MEMCPYED for c in bads)
        for field, val in ((3, None), (4, cn + 2), (8, bs // 2), (12, None)):
            ck = blosc_chunk(data[4 + field], ts, bs, 5, 1, b"lz4hc").copy()
            if field == 3:
                ck[3] = 4
            elif field == 12:
                ck[12:16] = np.array([ck.size + 1], "<u4").view(np.uint8)
            else:
                ck[field:field + 4] = np.array([val], "<u4").view(np.uint8)
            bads.append(ck)
        for k in range(len(bads)):
            chunks.append(good(data[10 + k], k))
            want.append(data[10 + k])
            chunks.append(bads[k])
            want.append(np.zeros(cn, np.uint8))
            refused.add(len(chunks) - 1)
        chunks.append(good(data[23], 1))
        want.append(data[23])
    out, bad, src, off = decode_all(ctx, chunks, cn, ts, bs)
    assert bad == len(refused)
    for i in range(len(chunks)):
        if i not in refused:
            assert np.array_equal(out[i], want[i]), i
    gather(ctx, np.random.default_rng(5), src, off, cn, ts, bs, want, bad=lambda i, b: i in refused, n=80)


@need_blosc
def test_automatic_blocksize_refused_on_host(ctx):
    """the reference's filter settings (lz4hc, clevel 5, shuffle, blocksize 0): c-blosc picks blocks far over 64 KiB;
    both decode entry points raise before launching anything"""
    cn = 2 * 1024 * 1024
    data = sample_data("genotype", cn, 6)
    ck = blosc_chunk(data, 2, 0, 5, 1, b"lz4hc")
    hbs = int(ck[8:12].view("<u4")[0])
    assert hbs > 65536
    src = to_dev(ck)
    off = to_dev(np.array([0, ck.size], np.int64))
    dst = torch.full((cn,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(HhgtError, match="does not fit LDS"):
        ctx.decompress(src, off, 1, cn, typesize=2, blocksize=hbs, dst=dst)
    sel, _, size = random_selections(np.random.default_rng(6), src, np.array([0, ck.size]), cn, hbs, 4, aligned=0)
    with pytest.raises(HhgtError, match="does not fit LDS"):
        ctx.decompress_blocks(sel, cn, typesize=2, blocksize=hbs, dst=dst)
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all())


@pytest.mark.parametrize("ts,bs", [(2, 128), (2, 64), (4, 256), (16, 1024), (2, 8192), (4, 4096)])
def test_split_small_blocks_served(ctx, ts, bs):
    """Split headers, shuffled and not.  Blocks of fewer than 128 elements (c-blosc and our encoder store those unsplit,
    another writer may not): one wave per stream, decoded exactly.  Split blocks without shuffle (c-blosc 1.21 writes them
    for shuffle 0; stream j = bytes [j n, (j + 1) n) of the block): a regression case, the un-shuffle step once read
    them as one contiguous stream"""
    cn = 7 * bs + bs // 2 + 3
    rng = np.random.default_rng(ts * bs)
    chunks, want = [], []
    for k in range(12):
        d = genotype_like(rng, cn) if k % 4 else rng.integers(0, 256, cn, dtype=np.uint8)
        shuffle = k % 3 != 0
        blocks = []
        for b in range(-(-cn // bs)):
            sh = oracle.shuffle(d[b * bs:(b + 1) * bs], ts) if shuffle else d[b * bs:(b + 1) * bs]
            n = sh.size // ts if sh.size == bs else sh.size
            parts = [sh[j * n:(j + 1) * n] for j in range(sh.size // n)]
            blocks.append([c if (c := oracle.lz4_compress(p)).size < p.size else p for p in parts])
        chunks.append(L.frame(blocks, ts, bs, cn, fmt=1 + k % 2, shuffle=shuffle))
        want.append(d)
        assert np.array_equal(oracle.blosc_decompress(chunks[-1]), d)
        if k % 2 == 0 and bs // ts >= 128 and extlibs.have_blosc():    # (c-blosc reads small split blocks as one stream)
            assert np.array_equal(extlibs.blosc1_decompress(chunks[-1], cn), d)
    out, bad, src, off = decode_all(ctx, chunks, cn, ts, bs)
    assert bad == 0
    for k in range(len(chunks)):
        assert np.array_equal(out[k], want[k]), k
    gather(ctx, np.random.default_rng(7), src, off, cn, ts, bs, want)


# ---- (e) allele counts on c-blosc lz4hc chunks ---------------------------------------------------------------------------
def genotype_calls(rng, n):
    """int8 0 / 1 / 2 / -9"""
    g = (rng.random(n) < 0.1).astype(np.int8)
    g[rng.random(n) < 0.02] = 2
    g[rng.random(n) < 0.02] = -9
    return g


@need_blosc
@pytest.mark.parametrize("sc,vc", [(1, 4096), (16, 4096), (64, 128)])
def test_count_alleles_on_cblosc_lz4hc(ctx, sc, vc):
    """typesize 2, blocks of min(8 KiB, a row): split (only a one-row chunk of one block: c-blosc widens the split blocks
    of larger chunks past 8 KiB), splitmode NEVER, shuffle 0 -- the three read paths of k_count_alleles -- and refused
    codecs counted once per selection"""
    cn = sc * vc * 2
    bs = min(8192, vc * 2)
    rng = np.random.default_rng(sc + vc)
    chunks, raws, refused = [], [], set()
    kinds = [("split", 1, b"lz4hc"), ("never", 1, b"lz4hc"), ("never", 0, b"lz4hc"), ("split", 0, b"lz4hc"),
             ("never", 1, b"blosclz"), ("never", 1, b"zstd")]
    for rep in range(3):
        for mode, shuffle, cname in kinds:
            if mode == "split" and cn != bs:
                continue
            g = genotype_calls(rng, cn)
            if mode == "never":
                with extlibs.splitmode(extlibs.BLOSC_NEVER_SPLIT):
                    ck = blosc_chunk(g.view(np.uint8), 2, bs, 5, shuffle, cname)
            else:
                ck = blosc_chunk(g.view(np.uint8), 2, bs, 5, shuffle, cname)
            assert int(ck[8:12].view("<u4")[0]) == bs and not ck[2] & L.MEMCPYED
            assert bool(ck[2] & L.DONT_SPLIT) == (mode == "never")
            if cname != b"lz4hc":
                refused.add(len(chunks))
            chunks.append(ck)
            raws.append(g)
    flat, off = pack(chunks)
    d = to_dev(flat)
    raw = np.stack(raws).reshape(len(chunks), sc, vc, 2)
    n_out = 3 * (bs // 2)
    sel = random_count_sel(rng, d, off, sc, vc, bs, 90, n_out)
    ptrs = d.data_ptr() + off[:-1]
    idx = np.searchsorted(ptrs, sel["src_ptr"].astype(np.int64))
    ok = np.array([i not in refused for i in idx])
    want = expected_counts(raw, ptrs, sel[ok], sc, vc, bs, n_out)
    counts, bad = ctx.count_alleles(sel, sc, vc, n_out=n_out, typesize=2, blocksize=bs)
    assert bad == int((~ok).sum()) and bad > 0
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), want)
