"""CPU: store_plan.plan_regions — the tables of hhgt_region_sums — against a brute-force statement: the union of a region's
pieces is exactly the bit positions of its variants inside the window plus the padding between them, in order, cut every
REGION_SPAN words counted from the word of the region's own first position; a region of one piece is direct, one of several
owns consecutive slots and a run.  And the ctypes declaration of hhgt_region_sums against the header's prototype."""
import ctypes
import os
import re

import numpy as np
import pytest

from haplohyped_varawareml_amd.store_plan import (PIECE_DIRECT, PIECE_FIELDS, PIECE_HI, PIECE_LO, PIECE_OUT, PIECE_SLOT,
                                                  REGION_MAX_COLS, REGION_SPAN, RUN_FIELDS, RUN_OUT, RUN_PIECES, RUN_SLOT,
                                                  mask_words_per_block, plan_regions, plane_positions)
from tests.test_grm_stats import header_prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_pieces(lo, hi, a, b, blocksize, block0):
    """the pieces of one region [lo, hi) in the window [a, b), one position at a time -> list of (p_lo, p_hi)"""
    lo, hi = max(lo, a), min(hi, b)
    if lo >= hi:
        return []
    pos = plane_positions(a, b, blocksize, block0)[lo - a:hi - a]
    covered = list(range(int(pos[0]), int(pos[-1]) + 1))              # the variants' positions and the padding between them
    w0 = covered[0] // 32
    pieces = {}
    for p in covered:
        pieces.setdefault((p // 32 - w0) // REGION_SPAN, []).append(p)
    return [(ps[0], ps[-1] + 1) for _, ps in sorted(pieces.items())]


def check_plan(regions, a, b, blocksize, block0=None):
    regions = np.asarray(regions, np.int64).reshape(-1, 2)
    pieces, runs, n_slots = plan_regions(regions, a, b, blocksize, block0)
    assert pieces.dtype == np.int64 and pieces.ndim == 2 and pieces.shape[1] == PIECE_FIELDS
    assert runs.dtype == np.int64 and runs.ndim == 2 and runs.shape[1] == RUN_FIELDS
    b0 = a // (blocksize // 2) if block0 is None else block0
    want, want_runs, slot = [], [], 0
    for r, (lo, hi) in enumerate(regions):
        mine = brute_pieces(int(lo), int(hi), a, b, blocksize, b0)
        if len(mine) > 1:
            want_runs.append((r, slot, len(mine)))
        for k, (p_lo, p_hi) in enumerate(mine):
            assert 0 < -(-p_hi // 32) - p_lo // 32 <= REGION_SPAN
            want.append((p_lo, p_hi, r, slot + k if len(mine) > 1 else PIECE_DIRECT))
        slot += len(mine) if len(mine) > 1 else 0
    assert pieces.tolist() == [list(x) for x in want]
    assert runs.tolist() == [list(x) for x in want_runs]
    assert n_slots == slot
    # what the kernel relies on: pieces inside the rows, slots used once, a region named by one run or one direct piece
    row_bits = ((b - 1) // (blocksize // 2) - b0 + 1) * 32 * mask_words_per_block(blocksize) if b > a else 0
    assert (pieces[:, PIECE_LO] >= 0).all() and (pieces[:, PIECE_HI] <= row_bits).all()
    slots = pieces[pieces[:, PIECE_SLOT] != PIECE_DIRECT, PIECE_SLOT]
    assert sorted(slots.tolist()) == list(range(n_slots))
    direct = pieces[pieces[:, PIECE_SLOT] == PIECE_DIRECT, PIECE_OUT].tolist()
    assert len(set(direct) | set(runs[:, RUN_OUT].tolist())) == len(direct) + len(runs)
    return pieces, runs, n_slots


def test_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "hhgt.h")).read()
    value = lambda name: int(re.search(rf"^#define {name} \(?(-?\d+)\)?\s*$", src, re.M).group(1))
    assert value("HHGT_REGION_SPAN") == REGION_SPAN == 64 and value("HHGT_REGION_MAX_COLS") == REGION_MAX_COLS == 16
    got = [value("HHGT_PIECE_" + n) for n in ("LO", "HI", "OUT", "SLOT", "FIELDS", "DIRECT")]
    assert got == [PIECE_LO, PIECE_HI, PIECE_OUT, PIECE_SLOT, PIECE_FIELDS, PIECE_DIRECT]
    assert [value("HHGT_RUN_" + n) for n in ("OUT", "SLOT", "PIECES", "FIELDS")] == [RUN_OUT, RUN_SLOT, RUN_PIECES, RUN_FIELDS]


def test_small_regions_in_one_block():
    bs = 2 * 4096                                           # 4096 variants a block: 128 words, no padding
    edge = [(5, 5), (9, 3), (7, 8), (0, 32), (0, 33), (31, 33), (32, 64), (100, 100 + 32 * REGION_SPAN),
            (100, 101 + 32 * REGION_SPAN), (96, 96 + 32 * REGION_SPAN), (96, 97 + 32 * REGION_SPAN), (0, 4096), (4095, 4096)]
    pieces, runs, n_slots = check_plan(edge, 0, 4096, bs)
    by_out = lambda r: pieces[pieces[:, PIECE_OUT] == r]
    assert len(by_out(0)) == len(by_out(1)) == 0                                  # empty regions give no piece
    assert by_out(2).tolist() == [[7, 8, 2, PIECE_DIRECT]]                        # one variant
    assert len(by_out(3)) == len(by_out(4)) == len(by_out(5)) == 1                # on and off a word's end
    assert len(by_out(7)) == 2 and len(by_out(8)) == 2 and len(by_out(9)) == 1 and len(by_out(10)) == 2
    assert by_out(7)[:, PIECE_HI].tolist() == [96 + 32 * REGION_SPAN, 100 + 32 * REGION_SPAN]      # cut from ITS first word
    assert len(by_out(11)) == 2 and n_slots == 8 and len(runs) == 4


def test_padding_between_blocks_stays_inside_a_region():
    bs = 200                                                # 100 variants a block in 4 words: 28 bits of padding each
    assert mask_words_per_block(bs) == 4
    regions = [(90, 110), (0, 700), (99, 100), (100, 101), (99, 101), (250, 650)]
    pieces, _, _ = check_plan(regions, 0, 700, bs)
    assert pieces[0].tolist() == [90, 128 + 10, 0, PIECE_DIRECT]                  # variants 90..99, 28 bits of padding, 100..109
    assert pieces[pieces[:, PIECE_OUT] == 4].tolist() == [[99, 129, 4, PIECE_DIRECT]]
    # a window that begins inside the group, at a block and inside one, with the rows' first block given
    check_plan(regions, 200, 700, bs)
    check_plan(regions, 250, 630, bs)
    check_plan(regions, 250, 630, bs, block0=1)
    with pytest.raises(IndexError):
        plan_regions(regions, 250, 630, bs, block0=3)


@pytest.mark.parametrize("words", [REGION_SPAN, REGION_SPAN + 1, 2 * REGION_SPAN, 2 * REGION_SPAN + 1])
def test_long_regions_are_cut_every_span(words):
    bs = 2 * 32 * 512                                       # one block of 512 words
    for first in (0, 1, 31, 32, 77):
        regions = [(first, first + 32 * words), (first, first + 32 * words - 31), (first, first + 32 * words + 1)]
        pieces, runs, _ = check_plan(regions, 0, 32 * 512, bs)
        n = [int((pieces[:, PIECE_OUT] == r).sum()) for r in range(3)]
        touched = lambda lo, hi: -(-hi // 32) - lo // 32
        assert n == [-(-touched(lo, hi) // REGION_SPAN) for lo, hi in regions]
        assert runs[:, RUN_PIECES].tolist() == [k for k in n if k > 1]


def test_regions_in_any_order_overlapping_duplicated_and_outside():
    rng = np.random.default_rng(5)
    bs, n_var = 2 * 1024, 9000                              # 32 words a block
    lo = rng.integers(-500, n_var + 500, 300)
    regions = np.stack([lo, lo + rng.integers(-50, 5000, 300)], axis=1)
    regions[10] = regions[11] = regions[12]                                       # duplicates, adjacent and not
    regions[200] = regions[12]
    regions[20] = (2000, 4000)
    regions[21] = (2500, 3000)                                                    # nested
    regions[22] = (-100, 0)
    regions[23] = (n_var, n_var + 10)                                             # outside the group
    for a, b in ((0, n_var), (1024, 5000), (3000, 3001), (4096, 4096), (100, 8999)):
        pieces, runs, n_slots = check_plan(regions, a, b, bs)
        outside = np.maximum(regions[:, 0], a) >= np.minimum(regions[:, 1], b)      # no variant of it in the window
        assert not np.isin(pieces[:, PIECE_OUT], np.nonzero(outside)[0]).any()
        assert set(pieces[:, PIECE_OUT].tolist()) == set(np.nonzero(~outside)[0].tolist())
        # a region's pieces are the same alone and among others, but for its output and its slots
        for r in (10, 12, 20, 21, 150, 200, 299):
            alone, alone_runs, k = plan_regions(regions[r:r + 1], a, b, bs)
            among = pieces[pieces[:, PIECE_OUT] == r]
            assert alone[:, :PIECE_OUT].tolist() == among[:, :PIECE_OUT].tolist()
            assert k == (len(alone) if len(alone) > 1 else 0) == len(alone_runs) * len(alone)
        same = [pieces[pieces[:, PIECE_OUT] == r][:, :PIECE_OUT].tolist() for r in (10, 11, 12, 200)]
        assert same[0] == same[1] == same[2] == same[3]
    none = plan_regions(np.zeros((0, 2), np.int64), 0, n_var, bs)
    assert none[0].shape == (0, PIECE_FIELDS) and none[1].shape == (0, RUN_FIELDS) and none[2] == 0


def test_lib_declares_hhgt_region_sums_as_the_header_does():
    from haplohyped_varawareml_amd import _lib, build
    build.build()
    L = _lib.load()
    args = header_prototype("hhgt_region_sums")
    assert args == ["hhgt_ctx *ctx", "const uint32_t *d_planes", "uint64_t n_rows", "uint64_t row_words", "const double *d_w",
                    "uint32_t n_cols", "const int64_t *d_pieces", "uint64_t n_pieces", "const int64_t *d_runs", "uint64_t n_runs",
                    "uint64_t n_slots", "uint64_t n_regions", "double *d_sums", "uint64_t *n_bad", "void *stream"]
    scalar = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    want = [ctypes.POINTER(ctypes.c_uint64) if a == "uint64_t *n_bad" else ctypes.c_void_p if "*" in a else scalar[a.split()[0]]
            for a in args]
    assert list(L.hhgt_region_sums.argtypes) == want and L.hhgt_region_sums.restype == ctypes.c_int
