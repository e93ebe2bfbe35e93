"""-m gpu: k_frame_write (csrc/frame.hip) — every framed chunk parsed strictly, field by field, and decoded.

The kernel requests a block's metadata in one level and, on the genotype path (typesize 2, 8 KiB blocks), the first 512 bytes
of both streams before it knows their sizes; the rest of a stream is requested by exact size, and the last 1-15 bytes go out
as 8 / 4 / 2 / 1-byte stores.  So the stream sizes are crafted around 16, 512 and 1024, and the output is held against an
independent statement of the layout (the parser below), against tools/sim/gapenc_ref.c for the stream bytes, against the
oracle's decoder and against the device decoder.

Sizes of 15, 16 and 17 bytes do not exist for a plane of 4096 positions: gapenc_ref's smallest stream — the empty plane —
has 26 bytes (test A asserts that it is above 17).  What those three sizes stand for, a last piece of 15 bytes, a stream
that ends with a full 16-byte piece, and a last piece of one byte, is taken at the smallest sizes the reference does
produce with the same remainders mod 16.  And a 0/1 plane of density 0.5 is not stored: the byte-wise encoder brings it to
about 2.4 KB, which reaches the 4 KiB pass all the same; a plane of random bytes beside it gives the stored 4096-byte stream."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import oracle
from haplohyped_varawareml_amd import device as dev
from haplohyped_varawareml_amd._lib import HhgtError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096                 # positions of a plane = bytes of a stream's source (blocksize 8192, typesize 2)
BS = 2 * N
ERR_CAPACITY = -3        # include/hhgt.h HHGT_ERR_CAPACITY
POOL_SEED, POOL_PLANES = 7, 3000
SIZES_ASKED = [511, 512, 513, 527, 528, 1023, 1024, 1025]


# ---- an independent statement of the chunk layout -----------------------------------------------------------------------------
def parse_chunk(chunk, nbytes, typesize, blocksize, fmt):
    """chunk bytes -> (memcpyed, [[stream bytes of block b] ...]); asserts every header field, every bstart, that the streams
    lie back to back and that the last one ends where the header's cbytes says"""
    chunk = np.asarray(chunk, np.uint8)
    hl = 16 if fmt == dev.BLOSC1 else 32
    split = 2 <= typesize <= 16 and blocksize // typesize >= 128
    nblocks = -(-nbytes // blocksize)
    h = chunk[:hl]
    flags = int(h[2])
    memcpyed = bool(flags & 0x2)
    want_flags = (1 << 5) | (0x1 if typesize > 1 else 0) | (0 if split else 0x10) | (0x2 if memcpyed else 0)
    want = np.zeros(hl, np.uint8)
    if fmt == dev.BLOSC1:
        want[0], want[1], want[2] = 2, 1, want_flags
    else:
        want[0], want[1], want[2] = 5, 1, want_flags | 0x1 | 0x4
        want[16 + 5] = 1 if typesize > 1 else 0
    want[3] = typesize
    want[4:16] = np.array([nbytes, blocksize, chunk.size], "<u4").view(np.uint8)
    assert np.array_equal(h, want), f"header {h.tolist()} != {want.tolist()}"
    if memcpyed:
        assert chunk.size == nbytes + hl
        return True, chunk[hl:]
    bst = chunk[hl:hl + 4 * nblocks].view("<u4")
    p = hl + 4 * nblocks
    blocks = []
    for b in range(nblocks):
        assert int(bst[b]) == p, f"bstart[{b}] = {int(bst[b])}, streams in front end at {p}"
        leftover = nbytes - b * blocksize < blocksize
        streams = []
        for _ in range(typesize if split and not leftover else 1):
            cs = int(chunk[p:p + 4].copy().view("<u4")[0])
            assert 0 < cs and p + 4 + cs <= chunk.size, f"block {b}: stream of {cs} bytes at {p} leaves the chunk of {chunk.size}"
            streams.append(chunk[p + 4:p + 4 + cs])
            p += 4 + cs
        blocks.append(streams)
    assert p == chunk.size, f"streams end at {p}, cbytes is {chunk.size}"
    return False, blocks


def chunks_of(dst, off, total):
    """-> the chunks, after checking that they are packed from 0 to total"""
    off = off.cpu().numpy()
    assert off[0] == 0 and off[-1] == total and np.all(np.diff(off) > 0)
    d = dst[:total].cpu().numpy()
    return [d[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)], off


def check_decodes(ctx, dst, off, total, raw, nbytes, typesize, blocksize):
    chunks, _ = chunks_of(dst, off, total)
    for i, ch in enumerate(chunks):
        assert np.array_equal(oracle.blosc_decompress(ch), raw[i * nbytes:(i + 1) * nbytes]), f"chunk {i}: oracle decode"
    back, n_bad = ctx.decompress(dst, off, len(chunks), nbytes, typesize=typesize, blocksize=blocksize)
    assert n_bad == 0 and np.array_equal(back.cpu().numpy(), raw), "device decode"


# ---- test A's input: planes with crafted stream sizes, from a CPU pool ---------------------------------------------------------
@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("gapenc") / "libgapenc.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "sim", "gapenc_ref.c")])
    L = C.CDLL(so)
    L.gapenc_ref.restype = C.c_int
    L.gapenc_ref.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]

    def encode(plane):                 # depth 2 = the default effort (clevel 5)
        out = np.zeros(N + 64, np.uint8)
        n = L.gapenc_ref(plane.ctypes.data, N, out.ctypes.data, 2)
        return None if n < 0 else out[:n].copy()
    return encode


NBLK, NCHUNK, RANDOM_CHUNKS = 5, 7, (1, 4)     # five blocks per chunk: 35 blocks in all, no multiple of four
CHUNK = NBLK * BS


@pytest.fixture(scope="module")
def crafted(ref):
    """-> dict(raw, planes [chunk][2 * NBLK], want: the sizes placed, dense / stored: (chunk, plane) of the two long streams)"""
    rng = np.random.default_rng(POOL_SEED)
    by_size, pool = {}, []
    for _ in range(POOL_PLANES):
        pl = np.zeros(N, np.uint8)
        pl[rng.choice(N, int(rng.integers(0, 601)), replace=False)] = 1
        e = ref(pl)
        assert e is not None and e.size < N       # at most 600 ones: always bit-plane coded
        by_size.setdefault(e.size, pl)
        pool.append(pl)
    sizes = sorted(by_size)
    assert sizes[0] > 17, "the reference now yields streams of 17 bytes or less: ask for 15, 16 and 17 themselves"
    tails = [min((s for s in sizes if s % 16 == r), default=None) for r in (15, 0, 1)]
    want = [sizes[0]] + tails + SIZES_ASKED + [sizes[-1]]
    missing = [s for s in want if s not in by_size]
    assert not missing, f"the pool holds no plane of size {missing}"
    assert all(t < 64 for t in tails) and 1025 < sizes[-1] < N
    comp = [c for c in range(NCHUNK) if c not in RANDOM_CHUNKS]
    planes = {c: [pool[int(rng.integers(0, len(pool)))] for _ in range(2 * NBLK)] for c in comp}
    # the crafted sizes: spread over the compressible chunks, as first and as second stream of a block, first block included
    slots = [(c, k) for k in (0, 1, 4, 7, 9) for c in comp][:len(want)]
    for (c, k), s in zip(slots, want):
        planes[c][k] = by_size[s]
    # streams of the 4 KiB pass, each in an otherwise sparse chunk: a 0/1 plane of density 0.5 (the byte-wise encoder still
    # finds matches in it: about 2.4 KB) and a plane of random bytes, which is stored as its 4096 bytes
    dense, stored = (comp[-1], 5), (comp[-2], 6)
    assert dense not in slots and stored not in slots
    planes[dense[0]][dense[1]] = (rng.random(N) < 0.5).astype(np.uint8)
    planes[stored[0]][stored[1]] = rng.integers(0, 256, N).astype(np.uint8)
    raw = np.empty((NCHUNK, NBLK, N, 2), np.uint8)
    for c in range(NCHUNK):
        if c in RANDOM_CHUNKS:
            raw[c] = rng.integers(0, 256, (NBLK, N, 2))
        else:
            raw[c, :, :, 0] = np.stack(planes[c][0::2])
            raw[c, :, :, 1] = np.stack(planes[c][1::2])
    return dict(raw=raw.reshape(-1), planes=planes, want=want, placed=dict(zip(slots, want)), dense=dense, stored=stored)


@pytest.fixture(scope="module")
def framed(ctx, crafted):
    """the crafted input framed once (16-byte header form): (chunk bytes of the whole call, offsets, total)"""
    dst, off, total = ctx.compress(torch.from_numpy(crafted["raw"]).cuda(), CHUNK, typesize=2, blocksize=BS, fmt=dev.BLOSC1)
    return dst[:total].cpu().numpy().copy(), off.cpu().numpy().copy(), total


def test_crafted_stream_sizes_parse_strictly(ctx, ref, crafted, framed):
    d, off, total = framed
    assert off[0] == 0 and off[-1] == total == d.size
    seen = {}
    for c in range(NCHUNK):
        ch = d[int(off[c]):int(off[c + 1])]
        memcpyed, blocks = parse_chunk(ch, CHUNK, 2, BS, dev.BLOSC1)    # (cbytes == off[c + 1] - off[c]: the header check)
        assert memcpyed == (c in RANDOM_CHUNKS), f"chunk {c}"
        if memcpyed:
            assert np.array_equal(blocks, crafted["raw"][c * CHUNK:(c + 1) * CHUNK])
            continue
        for b, streams in enumerate(blocks):
            assert len(streams) == 2
            for h, got in enumerate(streams):
                pl = crafted["planes"][c][2 * b + h]
                if (c, 2 * b + h) == crafted["stored"]:
                    assert got.size == N and np.array_equal(got, pl), "the plane of random bytes is stored"
                    continue
                if (c, 2 * b + h) == crafted["dense"]:
                    assert 1024 < got.size < N and np.array_equal(oracle.lz4_decompress(got, N), pl), "the dense plane"
                    continue
                want = ref(pl)
                assert np.array_equal(got, want), f"chunk {c} block {b} stream {h}: {got.size} bytes, gapenc_ref has {want.size}"
                seen[(c, 2 * b + h)] = got.size
    for slot, s in crafted["placed"].items():
        assert seen[slot] == s, f"the plane crafted for {s} bytes came out with {seen[slot]}"
    dst, offt = torch.from_numpy(d).cuda(), torch.from_numpy(off).cuda()
    check_decodes(ctx, dst, offt, total, crafted["raw"], CHUNK, 2, BS)


# ---- test B: a memcpyed chunk between / in front of compressible ones ---------------------------------------------------------
@pytest.mark.parametrize("fmt", [dev.BLOSC1, dev.BLOSC2])
def test_memcpyed_chunk_int8(ctx, fmt):
    rng = np.random.default_rng(31)
    raw = (rng.random((3, CHUNK)) < 0.02).astype(np.uint8)
    raw[1] = rng.integers(0, 256, CHUNK)
    raw = raw.reshape(-1)
    dst, off, total = ctx.compress(torch.from_numpy(raw).cuda(), CHUNK, typesize=2, blocksize=BS, fmt=fmt)
    chunks, offs = chunks_of(dst, off, total)
    hl = 16 if fmt == dev.BLOSC1 else 32
    kinds = []
    for c, ch in enumerate(chunks):
        memcpyed, body = parse_chunk(ch, CHUNK, 2, BS, fmt)
        kinds.append(memcpyed)
        if memcpyed:
            assert np.array_equal(body, raw[c * CHUNK:(c + 1) * CHUNK])
    assert kinds == [False, True, False]
    assert offs[2] - offs[1] == CHUNK + hl and offs[1] < CHUNK // 4 and offs[3] - offs[2] < CHUNK // 4
    check_decodes(ctx, dst, off, total, raw, CHUNK, 2, BS)


def tile_major(planes):
    """byte planes [2 rows][4096] of ONE chunk column (plane 2r = haplotype 0 of sample row r) -> the column's plane bytes as
    include/hhgt.h lays them out ([tile][kind-plane][row][32 B]: two planes of ones, two of exceptions — a missing call is a
    one with the exception bit, any other byte a zero with it, and its value stays in the int8 matrix), and the int8 bytes"""
    planes = np.asarray(planes, np.uint8)
    rows = planes.shape[0] // 2
    P = np.zeros((16, 4, rows, 32), np.uint8)
    for h in range(2):
        pl = planes[h::2].reshape(rows, 16, 256)
        P[:, h] = np.packbits((pl == 1) | (pl == 0xF7), axis=2, bitorder="little").transpose(1, 0, 2)
        P[:, 2 + h] = np.packbits(pl > 1, axis=2, bitorder="little").transpose(1, 0, 2)
    raw = np.empty((rows, N, 2), np.uint8)
    raw[:, :, 0], raw[:, :, 1] = planes[0::2], planes[1::2]
    return P.reshape(-1), raw.reshape(-1)


def test_memcpyed_chunk_planes(ctx):
    """the planes path (hhgt_compress_planes), 64 sample rows, two chunk columns.  Every plane of the first chunk is dense in
    calls that no match covers — nine in ten are allele bytes beyond 0 / 1 / missing, whose values the int8 matrix supplies,
    the rest 0, 1 and missing (a 0/1 plane of density 0.5 still compresses to 2.4 KB and would not do) — so the chunk's bytes
    are generated from planes and matrix behind a memcpyed header, and the second chunk starts right behind them"""
    rng = np.random.default_rng(32)
    S = 64
    hard = rng.integers(2, 121, (2 * S, N)).astype(np.uint8)
    few = rng.random((2 * S, N)) < 0.1
    hard[few] = rng.choice(np.array([0, 1, 0xF7], np.uint8), int(few.sum()))
    cols = [hard, (rng.random((2 * S, N)) < 0.01).astype(np.uint8)]
    P, raw = zip(*(tile_major(c) for c in cols))
    P, raw = np.concatenate(P), np.concatenate(raw)
    lay = dev.make_layout(S, 2 * N, sc=S, vc=N)
    res = dev.EncodeResult(torch.from_numpy(raw).cuda(), lay, None, None, None, None, 0, {}, [], torch.from_numpy(P).cuda())
    assert np.array_equal(ctx.planes_expand(res).cpu().numpy(), raw), "the planes built here do not say what raw says"
    nbytes = S * BS
    for fmt in (dev.BLOSC1, dev.BLOSC2):
        dst, off, total = ctx.compress_planes(res, fmt=fmt)
        chunks, offs = chunks_of(dst, off, total)
        hl = 16 if fmt == dev.BLOSC1 else 32
        m0, body = parse_chunk(chunks[0], nbytes, 2, BS, fmt)
        m1, blocks = parse_chunk(chunks[1], nbytes, 2, BS, fmt)
        assert m0 and not m1 and offs[1] == nbytes + hl
        assert np.array_equal(body, raw[:nbytes])
        assert len(blocks) == S and all(len(b) == 2 for b in blocks)
        check_decodes(ctx, dst, off, total, raw, nbytes, 2, BS)


# ---- test C: nothing outside [dst, dst + off[n]) ------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [1, 7, 15])
def test_nothing_written_outside(ctx, crafted, framed, lead):
    d, off, total = framed
    src = torch.from_numpy(crafted["raw"]).cuda()
    slack = 4096
    buf = torch.full((lead + total + slack,), 0xA5, dtype=torch.uint8, device="cuda")
    dst, off2, total2 = ctx.compress(src, CHUNK, typesize=2, blocksize=BS, fmt=dev.BLOSC1, dst=buf[lead:])
    got = buf.cpu().numpy()
    assert total2 == total and np.array_equal(off2.cpu().numpy(), off)
    assert np.array_equal(got[lead:lead + total], d), "the chunks differ from those framed at an aligned dst"
    assert np.all(got[:lead] == 0xA5) and np.all(got[lead + total:] == 0xA5)
    # one byte short, synchronous form: the error, and nothing behind dst_cap (the last chunk is the one that does not fit)
    buf.fill_(0xA5)
    with pytest.raises(HhgtError) as e:
        ctx.compress(src, CHUNK, typesize=2, blocksize=BS, fmt=dev.BLOSC1, dst=buf[lead:lead + total - 1])
    assert e.value.code == ERR_CAPACITY
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[:lead] == 0xA5) and np.all(got[lead + total - 1:] == 0xA5)
    fit = int(off[-2])
    assert np.array_equal(got[lead:lead + fit], d[:fit]), "the chunks that fit are written"


# ---- test D: the other paths --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typesize,blocksize,nbytes", [
    (1, 4096, 2 * 4096 + 1000),          # no split: one stream per block, and a leftover block
    (4, 2048, 3 * 2048 + 512),           # four streams per block; the leftover block has one
    (35, 2240, 3 * 2240 + 350),          # typesize beyond 16: never split
    (2, 512, 4 * 512 + 100),             # two streams in slots of 288 bytes: no early load may be taken
    (2, 8192, 2 * 8192 + 4096),          # the genotype geometry with a leftover block
])
@pytest.mark.parametrize("fmt", [dev.BLOSC1, dev.BLOSC2])
def test_other_geometries(ctx, typesize, blocksize, nbytes, fmt):
    rng = np.random.default_rng(typesize * 1000 + blocksize)
    n_chunks = 3
    raw = (rng.random(n_chunks * nbytes) < 0.05).astype(np.uint8) * rng.integers(1, 4, n_chunks * nbytes).astype(np.uint8)
    dst, off, total = ctx.compress(torch.from_numpy(raw).cuda(), nbytes, typesize=typesize, blocksize=blocksize, fmt=fmt)
    chunks, _ = chunks_of(dst, off, total)
    for ch in chunks:
        memcpyed, blocks = parse_chunk(ch, nbytes, typesize, blocksize, fmt)
        assert not memcpyed and len(blocks[-1]) == 1
    assert total < raw.size
    for i, ch in enumerate(chunks):
        assert np.array_equal(oracle.blosc_decompress(ch), raw[i * nbytes:(i + 1) * nbytes]), f"chunk {i}: oracle decode"
