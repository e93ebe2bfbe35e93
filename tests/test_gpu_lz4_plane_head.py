"""The head of k_lz4_bitplanes_uni's wave (csrc/lz4bits.hip, DESIGN.md §3.2 "The head of a plane's wave"): from the
workgroup index to the plane's lines without a division (planes_block32 / planes_lane_bytes, csrc/common.h), and the
stream of an all-zero plane written without coding it.

-m gpu: through compress_planes, every stream is compared byte for byte with tools/sim/gapenc_ref.c and every chunk is
decoded by the oracle (the helpers of tests/test_gpu_lz4_plane_grid.py).  Block counts: 1, 63, 64, 65 and D - 1, D, D + 1,
2 D + 1 with D = AHEAD / 2 blocks, the counts at which a workgroup AHEAD further on is missing, is the last one, and lies
in another chunk column and sample row.  The warm-ahead these counts were chosen for was measured and NOT built
(profiles/r12_head_split.txt); AHEAD stays here as the smallest look-ahead of that sweep — the counts are cases of the
mapping like any other.  The same with a first column > 0 and fewer columns than the buffer holds, and with one and two
blocks per sample row (vc 4096 / 8192).

CPU: tests/lz4_plane_head_check.cpp, a program of its own under AddressSanitizer / UBSan, walks every workgroup of these
geometries and of the flagship's and holds the division-free mapping to planes_block and every load to the planes buffer."""
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import oracle
from haplohyped_varawareml_amd import device as dev
from tests.test_gpu_lz4_bitplanes import LAZY, N, ref, streams_of   # noqa: F401  (ref: the fixture, with a depth argument)
from tests.test_gpu_lz4_plane_grid import check, layout_of, random_planes, to_tile_major

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

AHEAD = 256          # workgroups; D = AHEAD / 2 blocks (no look-ahead in the kernel: see above)
D = AHEAD // 2

# blocks of a call = columns x padded sample rows x (vc / 4096): (samples, sc, vc, columns of the buffer); sc = 0: one chunk
# of all rows.  tests/lz4_plane_head_check.cpp walks the same geometries.
SHAPES = {
    1: (1, 0, 4096, 1),
    63: (7, 0, 4096, 9),
    64: (5, 8, 8192, 4),         # 3 padded rows per column
    65: (65, 0, 4096, 1),
    D - 1: (127, 0, 4096, 1),
    D: (65, 64, 4096, 1),        # 64 + 1 rows: the second chunk is one row and 63 padded ones
    D + 1: (43, 0, 4096, 3),
    2 * D + 1: (257, 0, 4096, 1),
}
# two blocks per sample row: 66, D, 2 D + 2 blocks
SHAPES_BPR2 = {66: (11, 0, 8192, 3), D: (16, 0, 8192, 4), 2 * D + 2: (43, 0, 8192, 3)}
# (shape, first column, columns of the call): 63, 64, D + 1 and D blocks out of a larger buffer
PARTIAL = [((7, 0, 4096, 12), 2, 9), ((5, 8, 8192, 6), 1, 4), ((43, 0, 4096, 5), 1, 3), ((65, 64, 4096, 3), 2, 1)]


def ref_at(ref, depth):
    return lambda plane: ref(np.ascontiguousarray(plane), depth)


def check_cols(ctx, ref2, shape, pl, col0, n_cols):
    """tests/test_gpu_lz4_plane_grid.py's compress + check for the column slots [col0, col0 + n_cols) of the planes"""
    lay, s_pad, bpr = layout_of(shape)
    P, raw = to_tile_major(pl)
    res = dev.EncodeResult(None, lay, None, None, None, None, 0, {}, [], torch.from_numpy(P).cuda())
    dst, off, total = ctx.compress_planes(res, col0=col0, n_cols=n_cols, fmt=dev.BLOSC1)
    d, offs = dst[:total].cpu().numpy(), off.cpu().numpy()
    chunk_nbytes = (shape[1] or shape[0]) * shape[2] * 2
    col_nbytes = s_pad * shape[2] * 2
    raw = raw[col0 * col_nbytes:(col0 + n_cols) * col_nbytes]
    assert len(offs) - 1 == raw.size // chunk_nbytes and int(offs[-1]) == total
    got = []
    for i in range(len(offs) - 1):
        chunk = d[int(offs[i]):int(offs[i + 1])]
        assert np.array_equal(oracle.blosc_decompress(chunk), raw[i * chunk_nbytes:(i + 1) * chunk_nbytes]), f"chunk {i} does not decode to the input"
        got += streams_of(chunk, 2, 8192, chunk_nbytes)
    flat = pl[col0:col0 + n_cols].reshape(-1, N)
    assert len(got) == len(flat)
    n_ref = 0
    for k, plane in enumerate(flat):
        want = ref2(plane)
        back = got[k] if got[k].size == N else oracle.lz4_decompress(got[k], N)
        assert np.array_equal(back, plane), f"stream {k} does not decode to its plane"
        if want is None or want.size >= N:
            continue
        n_ref += 1
        assert np.array_equal(got[k], want), f"stream {k} (block {k // 2}, plane {k % 2}) differs from gapenc_ref ({got[k].size} vs {want.size} bytes)"
    return n_ref


@gpu
@pytest.mark.parametrize("n_blocks", sorted(SHAPES))
def test_block_counts_around_the_look_ahead(ctx, ref, n_blocks):
    shape = SHAPES[n_blocks]
    _, s_pad, bpr = layout_of(shape)
    assert shape[3] * s_pad * bpr == n_blocks
    ctx.set_clevel(5)
    pl = random_planes(np.random.default_rng(3000 + n_blocks), shape)
    assert check(ctx, ref_at(ref, 2), shape, pl) == 2 * n_blocks


@gpu
@pytest.mark.parametrize("n_blocks", sorted(SHAPES_BPR2))
def test_two_blocks_per_sample_row(ctx, ref, n_blocks):
    shape = SHAPES_BPR2[n_blocks]
    _, s_pad, bpr = layout_of(shape)
    assert bpr == 2 and shape[3] * s_pad * bpr == n_blocks
    ctx.set_clevel(5)
    pl = random_planes(np.random.default_rng(3100 + n_blocks), shape)
    assert check(ctx, ref_at(ref, 2), shape, pl) == 2 * n_blocks


@gpu
@pytest.mark.parametrize("shape,col0,n_cols", PARTIAL)
def test_first_column_and_fewer_columns_than_the_buffer(ctx, ref, shape, col0, n_cols):
    """the call's block 0 is the first block of column slot col0, and the columns behind the call stay untouched"""
    _, s_pad, bpr = layout_of(shape)
    ctx.set_clevel(5)
    pl = random_planes(np.random.default_rng(3200 + col0 + shape[0]), shape)
    assert check_cols(ctx, ref_at(ref, 2), shape, pl, col0, n_cols) == 2 * n_cols * s_pad * bpr


# ---- empty planes ------------------------------------------------------------------------------------------------------
# clevel -> gapenc_ref's depth: no candidates at all, the default, and twelve with the lazy rule (twelve WITHOUT it is no
# clevel's: clevel 9 has run with the lazy rule since round 4)
EFFORTS = [(1, 0), (5, 2), (9, 12 | LAZY)]
EMPTY_STREAM = bytes([0x1F, 0, 1, 0] + [0xFF] * 15 + [0xF6, 0x50, 0, 0, 0, 0, 0])


def test_the_empty_stream_is_the_reference_s(ref):
    """the 26 bytes k_lz4_bitplanes_uni writes for an all-zero plane are gapenc_ref's at every depth the kernel is built for"""
    for depth in (0, 1, 2, 4, 8, 12, 16, 2 | LAZY, 12 | LAZY):
        assert ref(np.zeros(N, np.uint8), depth).tobytes() == EMPTY_STREAM, depth
    assert np.array_equal(oracle.lz4_decompress(np.frombuffer(EMPTY_STREAM, np.uint8), N), np.zeros(N, np.uint8))


def at_effort(ctx, clevel, fn):
    ctx.set_clevel(clevel)
    try:
        return fn()
    finally:
        ctx.set_clevel(5)


@gpu
@pytest.mark.parametrize("clevel,depth", EFFORTS)
def test_an_all_zero_call(ctx, ref, clevel, depth):
    shape = SHAPES[65]
    pl = np.zeros_like(random_planes(np.random.default_rng(1), shape))
    assert at_effort(ctx, clevel, lambda: check(ctx, ref_at(ref, depth), shape, pl)) == 2 * 65


@gpu
@pytest.mark.parametrize("clevel,depth", EFFORTS)
def test_empty_planes_among_ordinary_ones_and_in_padded_rows(ctx, ref, clevel, depth):
    """S = 70 in chunks of 64 rows: 58 padded rows, all empty; of the others every third plane is emptied, so that empty
    and ordinary planes alternate inside a block and inside a group of workgroups"""
    shape = (70, 64, 4096, 2)
    _, s_pad, bpr = layout_of(shape)
    assert s_pad - shape[0] == 58
    pl = random_planes(np.random.default_rng(3300 + clevel), shape)
    pl.reshape(-1, N)[::3] = 0
    assert at_effort(ctx, clevel, lambda: check(ctx, ref_at(ref, depth), shape, pl)) == 2 * shape[3] * s_pad * bpr


@gpu
@pytest.mark.parametrize("clevel,depth", EFFORTS)
def test_nearly_empty_planes(ctx, ref, clevel, depth):
    """a plane whose only nonzero byte is a missing call is not empty (it goes to the exception-aware path), nor is one
    with a single 1 at position 0 or 4095; their siblings and neighbours are empty"""
    shape = (8, 0, 4096, 1)
    pl = np.zeros_like(random_planes(np.random.default_rng(1), shape))
    flat = pl.reshape(-1, N)
    flat[1][777] = 0xF7
    flat[2][0] = 0xF7
    flat[4][N - 1] = 0xF7
    flat[6][0] = 1
    flat[9][N - 1] = 1
    flat[11][0] = flat[11][N - 1] = 1
    flat[12][2048] = 1
    flat[13][2048] = 0xF7
    assert at_effort(ctx, clevel, lambda: check(ctx, ref_at(ref, depth), shape, pl)) == 2 * 8


# ---- the mapping on the CPU --------------------------------------------------------------------------------------------
def test_mapping_program_under_sanitizers(tmp_path):
    """tests/lz4_plane_head_check.cpp: host code only, nothing preloaded; never where a device is visible"""
    if torch.cuda.is_available():
        pytest.skip("a sanitized program must not open a device: this test runs on CPU-only hosts")
    from haplohyped_varawareml_amd.build import _hipcc
    exe = str(tmp_path / "lz4_plane_head_check")
    subprocess.check_call([_hipcc(), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "lz4_plane_head_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "Sanitizer" not in r.stderr, r.stdout + r.stderr
