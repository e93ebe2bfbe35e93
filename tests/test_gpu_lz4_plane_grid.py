"""-m gpu: which workgroup of k_lz4_bitplanes_uni codes which plane, and where its stream lands (csrc/lz4bits.hip: one
workgroup per plane, dealt in groups of 128 = 64 blocks so that the eight blocks an XCD takes are consecutive and both
planes of a block stay on it; the grid is rounded up to whole groups).  Through compress_planes at clevel 5 (two
candidates per one), every stream is compared byte for byte with tools/sim/gapenc_ref.c and every chunk is decoded by the
oracle — over block counts on both sides of 64 and 128, sample rows that split the four rows of a 128-byte line across
groups, padded rows, blocks whose two planes take different paths (plain / exception-aware / left to the byte-wise coder),
and calls of different sizes behind each other on one context."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import oracle
from haplohyped_varawareml_amd import device as dev
from tests.test_gpu_lz4_bitplanes import N, bench_like, streams_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# blocks of a call = columns x padded sample rows x (vc / 4096): (samples, sc, vc, columns); sc = 0: one chunk of all rows
SHAPES = {
    1: (1, 0, 4096, 1),
    7: (7, 0, 4096, 1),
    8: (4, 4, 8192, 1),
    9: (3, 0, 4096, 3),
    63: (7, 0, 4096, 9),
    64: (5, 8, 8192, 4),       # 3 padded rows per column
    65: (65, 0, 4096, 1),
    127: (127, 0, 4096, 1),
    128: (65, 64, 4096, 1),    # 64 + 1 rows: the second chunk is one row and 63 padded ones
    129: (43, 0, 4096, 3),
    200: (5, 0, 8192, 20),
}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("gapenc") / "libgapenc.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "sim", "gapenc_ref.c")])
    L = C.CDLL(so)
    L.gapenc_ref.restype = C.c_int
    L.gapenc_ref.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]

    def encode(plane):                 # depth 2 = clevel 5
        plane = np.ascontiguousarray(plane)
        out = np.zeros(N + 64, np.uint8)
        n = L.gapenc_ref(plane.ctypes.data, N, out.ctypes.data, 2)
        return None if n < 0 else out[:n].copy()
    return encode


def layout_of(shape):
    S, sc, vc, cols = shape
    lay = dev.make_layout(S, cols * vc, sc=sc, vc=vc)
    s_pad = -(-S // sc) * sc if sc else S
    return lay, s_pad, vc // N


def random_planes(rng, shape, frac=0.0):
    """byte planes [column][padded row][block of the row][haplotype][4096]: bench-like ones, a fraction of all positions a
    missing call (0xF7), padded rows zero"""
    S, sc, vc, cols = shape
    _, s_pad, bpr = layout_of(shape)
    pl = bench_like(rng, cols * s_pad * bpr * 2).reshape(cols, s_pad, bpr, 2, N)
    if frac:
        pl[rng.random(pl.shape) < frac] = 0xF7
    pl[:, S:] = 0
    return pl


def to_tile_major(pl):
    """-> (the plane bytes as include/hhgt.h lays them out: [column][tile][kind-plane][row][32 B], the int8 bytes they stand for)"""
    cols, s_pad, bpr = pl.shape[:3]
    P = np.zeros((cols, 16 * bpr, 4, s_pad, 32), np.uint8)
    for h in range(2):
        rows = pl[:, :, :, h].reshape(cols, s_pad, 16 * bpr, 256)
        P[:, :, h] = np.packbits(rows != 0, axis=3, bitorder="little").transpose(0, 2, 1, 3)
        P[:, :, 2 + h] = np.packbits(rows == 0xF7, axis=3, bitorder="little").transpose(0, 2, 1, 3)
    return P.reshape(-1), np.ascontiguousarray(pl.transpose(0, 1, 2, 4, 3)).reshape(-1)


def compress(ctx, shape, pl):
    """-> the streams of the call, in block order (stream 2 b + h: haplotype h of block b); every chunk decoded by the oracle"""
    lay, s_pad, bpr = layout_of(shape)
    P, raw = to_tile_major(pl)
    res = dev.EncodeResult(None, lay, None, None, None, None, 0, {}, [], torch.from_numpy(P).cuda())
    dst, off, total = ctx.compress_planes(res, fmt=dev.BLOSC1)
    d, offs = dst[:total].cpu().numpy(), off.cpu().numpy()
    chunk_nbytes = (shape[1] or shape[0]) * shape[2] * 2
    assert len(offs) - 1 == raw.size // chunk_nbytes and int(offs[-1]) == total
    out = []
    for i in range(len(offs) - 1):
        chunk = d[int(offs[i]):int(offs[i + 1])]
        assert np.array_equal(oracle.blosc_decompress(chunk), raw[i * chunk_nbytes:(i + 1) * chunk_nbytes]), f"chunk {i} does not decode to the input"
        out += streams_of(chunk, 2, 8192, chunk_nbytes)
    assert len(out) == raw.size // N
    return out


def check(ctx, ref, shape, pl, what=""):
    got = compress(ctx, shape, pl)
    flat = pl.reshape(-1, N)
    n_ref = 0
    for k, plane in enumerate(flat):
        want = ref(plane)
        back = got[k] if got[k].size == N else oracle.lz4_decompress(got[k], N)
        assert np.array_equal(back, plane), f"{what}stream {k} (block {k // 2}, plane {k % 2}) does not decode to its plane"
        if want is None or want.size >= N:        # left to the byte-wise coder / stored verbatim
            continue
        n_ref += 1
        assert np.array_equal(got[k], want), f"{what}stream {k} (block {k // 2}, plane {k % 2}) differs from gapenc_ref ({got[k].size} vs {want.size} bytes)"
    return n_ref


@pytest.mark.parametrize("n_blocks", sorted(SHAPES))
def test_every_plane_of_the_grid_matches_the_reference(ctx, ref, n_blocks):
    shape = SHAPES[n_blocks]
    _, s_pad, bpr = layout_of(shape)
    assert shape[3] * s_pad * bpr == n_blocks
    ctx.set_clevel(5)
    pl = random_planes(np.random.default_rng(1000 + n_blocks), shape)
    assert check(ctx, ref, shape, pl) == 2 * n_blocks


@pytest.mark.parametrize("n_blocks", [9, 65, 128])
def test_missing_calls_in_some_planes_of_the_grid(ctx, ref, n_blocks):
    """every third plane holds missing calls: neighbouring workgroups take different paths, in every position of a group"""
    shape = SHAPES[n_blocks]
    ctx.set_clevel(5)
    rng = np.random.default_rng(2000 + n_blocks)
    pl = random_planes(rng, shape)
    flat = pl.reshape(-1, N)
    for k in range(0, len(flat), 3):
        flat[k][rng.random(N) < 0.02] = 0xF7
    pl[:, shape[0]:] = 0
    assert check(ctx, ref, shape, pl) >= 2 * n_blocks - 2


@pytest.mark.parametrize("exc_plane", [0, 1])
def test_one_block_one_plane_with_missing_calls(ctx, ref, exc_plane):
    """the exception-aware and the plain path are taken per workgroup: one plane of the block with missing calls, its
    sibling without"""
    shape = SHAPES[1]
    ctx.set_clevel(5)
    rng = np.random.default_rng(31 + exc_plane)
    pl = random_planes(rng, shape)
    pl[0, 0, 0, exc_plane][rng.random(N) < 0.025] = 0xF7
    assert (pl[0, 0, 0, exc_plane] == 0xF7).any() and not (pl[0, 0, 0, 1 - exc_plane] == 0xF7).any()
    assert check(ctx, ref, shape, pl) == 2


@pytest.mark.parametrize("dense_plane", [0, 1])
def test_one_block_one_plane_too_dense(ctx, ref, dense_plane):
    """more than 636 ones: the single-wave workgroup marks the stream and raises flags[0], the byte-wise coder codes it;
    the sibling plane is the bit-plane coder's"""
    shape = SHAPES[1]
    ctx.set_clevel(5)
    rng = np.random.default_rng(41 + dense_plane)
    pl = random_planes(rng, shape)
    pl[0, 0, 0, dense_plane] = 0
    pl[0, 0, 0, dense_plane][rng.choice(N, 700, replace=False)] = 1
    assert ref(pl[0, 0, 0, dense_plane]) is None and ref(pl[0, 0, 0, 1 - dense_plane]) is not None
    assert check(ctx, ref, shape, pl) == 1


def test_calls_of_different_sizes_on_one_context(ctx, ref):
    """a large call, a small one, the large one again: no stream size or slot of an earlier call shows through"""
    ctx.set_clevel(5)
    rng = np.random.default_rng(51)
    big, small = SHAPES[129], SHAPES[7]
    pl_big, pl_small = random_planes(rng, big), random_planes(rng, small)
    assert check(ctx, ref, big, pl_big, "first call: ") == 2 * 129
    assert check(ctx, ref, small, pl_small, "second call: ") == 2 * 7
    assert check(ctx, ref, big, pl_big[::-1].copy(), "third call: ") == 2 * 129
