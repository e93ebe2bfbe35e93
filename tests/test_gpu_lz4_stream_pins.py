"""-m gpu: the byte-wise LZ4 coder's streams (csrc/lz4.hip), held to the bytes the coder wrote before it was cut into phases
(DESIGN.md §3.1).  The format leaves an encoder freedom, the other LZ4 tests only ask "decodes to the input" and a ratio; this
one pins every stream's size and SHA-256 (streams stored verbatim included) to tests/golden/lz4_bytewise_streams.json, written
by tests/golden/make_lz4_stream_pins.py from this module's case list.  Every case also decodes with the oracle.

Each case runs at clevel 1, 5 and 9, so all nine instantiations of k_lz4_blocks are reached:
  typesize 1, one stream per chunk                      <8,5,false> <7,6,false> <7,7,false>
  typesize 4 / 16 / 2 from an unaligned source          <0,*,false> (and the two-wave ones through the general shuffle)
  typesize 2, 8 KiB blocks from int8: scan mode         the two-wave ones beside the bit-plane coder; pinned are the streams
                                                        that coder leaves (a byte above 1, more than 636 nonzero bytes)
  the same from the bit-plane form                      <8,5,true> <7,6,true> <7,7,true>; some calls are 2, so their byte comes
                                                        from the int8 matrix
A null entry of the fixture is a stream on which two recording processes disagreed (none so far)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from haplohyped_varawareml_amd import device as dev
from tests.gpu_util import split_chunks
from tests.test_gpu_lz4_bitplanes import N, bench_like, run_planes, streams_of
from tests.test_gpu_lz4_patterns import sparse

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4_bytewise_streams.json")
CLEVELS = (1, 5, 9)


def to_dev_at(a, shift):
    """a on the device, `shift` bytes past an aligned address"""
    t = torch.zeros(a.size + 32, dtype=torch.uint8, device="cuda")
    t[shift:shift + a.size] = torch.from_numpy(a.copy())
    return t[shift:shift + a.size]


def chunk_streams(ck, typesize, blocksize):
    """the streams of one Blosc-1 chunk in block order; a memcpyed chunk counts as one stream, its payload"""
    nbytes, cbytes = int(ck[4:8].view("<u4")[0]), int(ck[12:16].view("<u4")[0])
    if ck[2] & 0x2:
        return [ck[16:16 + nbytes]]
    nblocks = -(-nbytes // blocksize)
    split = 2 <= typesize <= 16 and blocksize // typesize >= 128
    bstarts = ck[16:16 + 4 * nblocks].view("<u4")
    out, used = [], 16 + 4 * nblocks
    for b in range(nblocks):
        whole = min(blocksize, nbytes - b * blocksize) == blocksize
        p = int(bstarts[b])
        for _ in range(typesize if split and whole else 1):
            cs = int(ck[p:p + 4].view("<u4")[0])
            out.append(ck[p + 4:p + 4 + cs])
            p += 4 + cs
            used += 4 + cs
    assert used == cbytes == ck.size, (used, cbytes, ck.size)
    return out


def coded(ctx, data, chunk_nbytes, typesize, blocksize, shift=0):
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    dst, off, total = ctx.compress(to_dev_at(data, shift), chunk_nbytes, typesize=typesize, blocksize=blocksize, fmt=dev.BLOSC1)
    out = []
    for i, ck in enumerate(split_chunks(dst, off, total)):
        assert np.array_equal(oracle.blosc_decompress(ck), data[i * chunk_nbytes:(i + 1) * chunk_nbytes]), f"chunk {i}: oracle decode differs"
        out += chunk_streams(ck, typesize, blocksize)
    return out


def t1(ctx, rows, n):
    """rows of n bytes, typesize 1, one block and one stream per row"""
    return coded(ctx, np.concatenate([np.asarray(r, np.uint8) for r in rows]), n, 1, max(n, 16))


# ---- typesize 1: the patterns of tests/test_gpu_lz4_patterns.py ----------------------------------------------------------------
def case_sparse(ctx):
    out = []
    for seed, p in enumerate((0.002, 0.01, 0.03, 0.1, 0.3)):
        rng = np.random.default_rng(100 + seed)
        out += t1(ctx, [sparse(rng, 4096, p, missing=0.002) for _ in range(8)], 4096)
    return out


def case_gaps(ctx):
    rows = []
    for gap in (5, 6, 19, 20, 21, 36, 63, 64, 65, 300):
        for phase in (0, 1, gap // 2):
            a = np.zeros(4096, np.uint8)
            a[phase::gap] = 1
            rows.append(a)
    return t1(ctx, rows, 4096)


def case_motifs(ctx):
    rows, n = [], 8192
    for period in (1, 3, 19, 20, 21, 64, 65, 257):
        rng = np.random.default_rng(period)
        a = np.tile(rng.integers(0, 4, period, dtype=np.uint8), n // period + 1)[:n].copy()
        rows.append(a.copy())
        a[::1000] ^= 0x55
        rows.append(a)
    return t1(ctx, rows, n)


def case_tails(ctx):
    rows, n = [], 1000
    for tail in range(20):
        a = np.zeros(n, np.uint8)
        b = np.tile(np.array([3, 1, 4, 1, 5, 9, 2, 6], np.uint8), n // 8 + 1)[:n].copy()
        if tail:
            a[n - tail:] = np.arange(1, tail + 1, dtype=np.uint8)
            b[n - tail] ^= 0xFF
        rows += [a, b]
    return t1(ctx, rows, n)


def case_run_boundaries(ctx):
    rows, n = [], 2048
    for edge in (64, 128, 192, 256):
        for d in (-2, -1, 0, 1, 2):
            for v in (0, 1, 0xF7):
                a = np.full(n, v, np.uint8)
                a[edge + d] = v ^ 1
                a[edge + d + 40] = v ^ 1
                rows.append(a)
    return t1(ctx, rows, n)


def case_queue(ctx):
    rng = np.random.default_rng(7)
    n = 16384
    a = np.zeros(n, np.uint8)
    a[::5] = rng.integers(1, 256, a[::5].size, dtype=np.uint8)
    b = np.zeros(n, np.uint8)
    for s0 in range(0, n - 200, 200):
        b[s0:s0 + 40 + (s0 // 200) % 60] = rng.integers(0, 256, 40 + (s0 // 200) % 60, dtype=np.uint8)
    return t1(ctx, [a, b], n)


def case_lengths(ctx):
    out = []
    for n in list(range(1, 40)) + [63, 64, 65, 255, 256, 257]:
        rng = np.random.default_rng(n)
        out += t1(ctx, [np.zeros(n, np.uint8), np.ones(n, np.uint8), sparse(rng, n, 0.1), sparse(rng, n, 0.5),
                        np.tile(np.array([1, 0, 0], np.uint8), n // 3 + 1)[:n], rng.integers(0, 256, n, dtype=np.uint8)], n)
    return out


# ---- more than two waves per workgroup, leftover blocks, a source that is not 16-byte aligned -----------------------------
def case_ts4_leftover(ctx):
    rng = np.random.default_rng(41)
    chunk = 2 * 16384 + 1234
    m = 2 * chunk // 4 + 1
    v = (sparse(rng, m, 0.05).astype("<u4") * rng.integers(1, 70000, m, dtype=np.uint32)).astype("<u4")
    return coded(ctx, v.view(np.uint8)[:2 * chunk], chunk, 4, 16384, shift=1)


def case_ts16(ctx):
    rng = np.random.default_rng(42)
    m = 2 * 8192 * 2 // 16                                            # two chunks of two blocks
    rec = np.stack([sparse(rng, m, 0.5 ** (j % 8 + 1), missing=0.002) for j in range(16)], axis=1)
    return coded(ctx, rec, 2 * 8192, 16, 8192, shift=3)


def case_ts2_general(ctx):
    rng = np.random.default_rng(43)
    return coded(ctx, sparse(rng, 2 * 6000, 0.03, missing=0.002), 6000, 2, 2000, shift=1)


# ---- scan mode: typesize 2, 8 KiB blocks; the byte-wise coder takes what the bit-plane coder leaves marked ----------------------
def scan_planes(rng):
    planes = bench_like(rng, 16)
    planes[3, 100] = 0xF7
    planes[4, rng.integers(0, N, 300)] = 0xF7
    planes[7] = rng.integers(0, 2, N)
    planes[10] = rng.integers(0, 256, N)
    return planes


def case_scan_int8(ctx):
    planes = scan_planes(np.random.default_rng(9))
    got, _ = run_planes(ctx, planes)
    return [got[k] for k, pl in enumerate(planes) if (pl > 1).any() or np.count_nonzero(pl) > 636]


def planes_and_calls(planes):
    """byte planes [2 rows][4096] -> (tile-major plane bytes of one chunk column, the int8 bytes) as include/hhgt.h has the
    layout; a call beyond 0 / 1 / missing has its one-bit clear and its exception bit set, its byte comes from the matrix"""
    planes = np.asarray(planes, np.uint8)
    rows = planes.shape[0] // 2
    P = np.zeros((16, 4, rows, 32), np.uint8)                      # [tile][kind-plane][row][32 B]
    for h in range(2):
        pl = planes[h::2]
        one = np.packbits(((pl == 1) | (pl == 0xF7)).reshape(rows, 16, 256), axis=2, bitorder="little")
        exc = np.packbits((pl > 1).reshape(rows, 16, 256), axis=2, bitorder="little")
        P[:, h] = one.transpose(1, 0, 2)
        P[:, 2 + h] = exc.transpose(1, 0, 2)
    raw = np.empty((rows, N, 2), np.uint8)
    raw[:, :, 0] = planes[0::2]
    raw[:, :, 1] = planes[1::2]
    return P.reshape(-1), raw.reshape(-1)


def case_scan_planes(ctx):
    rng = np.random.default_rng(10)
    planes = scan_planes(rng)
    for k in (1, 5, 12):                                             # calls of value 2, few and many
        planes[k, rng.integers(0, N, 3 if k == 1 else 200)] = 2
    rows = len(planes) // 2
    P, raw = planes_and_calls(planes)
    lay = dev.make_layout(rows, N, sc=rows, vc=N)
    res = dev.EncodeResult(torch.from_numpy(raw).cuda(), lay, None, None, None, None, 0, {}, [], torch.from_numpy(P).cuda())
    assert np.array_equal(ctx.planes_expand(res).cpu().numpy(), raw)
    dst, off, total = ctx.compress_planes(res, fmt=dev.BLOSC1)
    chunk = dst[:total].cpu().numpy()
    assert np.array_equal(oracle.blosc_decompress(chunk), raw), "chunk does not decode to the input"
    got = streams_of(chunk, 2, 8192, raw.size)
    return [got[k] for k, pl in enumerate(planes) if ((pl > 1) & (pl != 0xF7)).any() or np.count_nonzero(pl) > 636]


CASES = {"sparse": case_sparse, "gaps": case_gaps, "motifs": case_motifs, "tails": case_tails, "run_boundaries": case_run_boundaries,
         "queue": case_queue, "lengths": case_lengths, "ts4_leftover": case_ts4_leftover, "ts16": case_ts16,
         "ts2_general": case_ts2_general, "scan_int8": case_scan_int8, "scan_planes": case_scan_planes}


def case_pins(ctx, name, clevel):
    """-> [[size, sha256 hex], ...] of the case's streams at this effort"""
    ctx.set_clevel(clevel)
    try:
        streams = CASES[name](ctx)
    finally:
        ctx.set_clevel(5)
    return [[int(s.size), hashlib.sha256(s.tobytes()).hexdigest()] for s in streams]


@pytest.fixture(scope="module")
def pins():
    return json.load(open(FIXTURE))


@pytest.mark.parametrize("clevel", CLEVELS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_streams_are_the_recorded_ones(ctx, pins, name, clevel):
    want = pins[f"{name}@{clevel}"]
    got = case_pins(ctx, name, clevel)
    assert len(got) == len(want) and len(got) > 0
    diff = [(k, g[0], w[0]) for k, (g, w) in enumerate(zip(got, want)) if w is not None and g != w]
    assert not diff, f"{name} at clevel {clevel}: {len(diff)} of {len(want)} streams differ; (stream, bytes, recorded bytes): {diff[:8]}"
