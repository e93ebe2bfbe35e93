"""hhgt_region_sums (the f64 MFMA over genotype planes, cut at the boundaries of regions) against numpy and against
hhgt_score_sums over one-hot region columns: every row count around a wave's 16 rows and a workgroup's 128, rows of a few
words and around one and two pieces' length, column counts around the one column tile; regions that are empty, of one bit,
across a word's end, the whole row, its last bit, identical, nested, longer than one and than two pieces."""
import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd._lib import HhgtError
from haplohyped_varawareml_amd.store_plan import (PIECE_DIRECT, REGION_MAX_COLS, REGION_SPAN,
                                                  plan_regions)
from tests.test_gpu_assoc import guarded, unpack
from tests.test_gpu_ld import random_vplanes
from tests.test_gpu_score import CLASS_OF_PLANE, device_planes

pytestmark = pytest.mark.gpu

SPAN = REGION_SPAN
ROWS = [1, 15, 16, 17, 127, 128, 129, 257]                 # around a wave's 16 rows and a workgroup's 128
WORDS = [1, 2, 3, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 1]  # the first few, around one and two pieces
COLS = [1, 15, 16]


def regions_of(rng, words, n_random=40):
    """about 40 random bit ranges of a row of `words` words and the edge set -> int64 [R, 2]"""
    bits = 32 * words
    lo = rng.integers(0, bits, n_random)
    length = np.where(rng.random(n_random) < 0.5, rng.integers(0, 40, n_random), rng.integers(0, bits + 1, n_random))
    out = [(int(a), int(min(a + n, bits))) for a, n in zip(lo, length)]
    out += [(5, 5), (3, 4), (0, bits), (bits - 1, bits), (2, bits - 1), (2, bits - 1), (1, bits), (4, bits // 2 + 1)]     # nested in the last
    if words >= 2:
        out += [(31, 33), (32, 64), (0, 32)]                # bit 31 of a word and bit 0 of the next; whole words
    if words > SPAN:
        out += [(7, 32 * SPAN + 8), (33, 32 * (SPAN + 1)), (32, 32 * (SPAN + 1) + 1)]          # SPAN + 1, SPAN and SPAN + 1 words
    if words > 2 * SPAN:
        out += [(50, 32 * 2 * SPAN + 40), (31, 32 * 2 * SPAN + 1)]                             # three pieces
    return np.array(out, np.int64)


def plan(regions, words):
    """the tables of regions given as bit ranges of a row of `words` words: one block of 32 words variants, no padding"""
    return plan_regions(regions, 0, 32 * words, 2 * 32 * words)


def np_regions(planes, w, regions):
    """uint32 [3, n, words], float64 [3, 32 words, C], [R, 2] -> float64 [n, R, C]"""
    bits = unpack(planes)
    out = np.zeros((planes.shape[1], len(regions), w.shape[2]))
    for r, (lo, hi) in enumerate(regions):
        if lo < hi:
            out[:, r] = sum(bits[k][:, lo:hi] @ w[c, lo:hi] for k, c in enumerate(CLASS_OF_PLANE))
    return out


def run(ctx, planes, w, regions, sums=None, **kw):
    words = planes.shape[2]
    pieces, runs, n_slots = plan(regions, words)
    return ctx.region_sums(device_planes(ctx, planes), torch.from_numpy(w).to(ctx.device), pieces, runs, n_slots, len(regions),
                           sums=sums, **kw)


@pytest.mark.parametrize("words", WORDS)
def test_kernel_is_exact_on_quarters(ctx, words):
    """quarters in [-2, 2]: every partial sum is representable, and the sums, which ADD to what the tensor holds, are exact;
    nothing outside the table is touched"""
    for i, n_rows in enumerate(ROWS):
        n_cols = COLS[(i + WORDS.index(words)) % len(COLS)]
        rng = np.random.default_rng(1000 * words + n_rows)
        regions = regions_of(rng, words)
        w = rng.integers(-8, 9, (3, 32 * words, n_cols)) / 4.0
        planes, _ = random_vplanes(rng, n_rows, words)       # (H, M, A: the planes overlap, and all of them count)
        start = rng.integers(-8, 9, (n_rows, len(regions), n_cols)) / 4.0
        buf, view = guarded(ctx, start.shape)
        view.copy_(torch.from_numpy(start))
        got = run(ctx, planes, w, regions, sums=view)
        assert got is view
        host = buf.cpu().numpy()
        assert np.isnan(host[:1024]).all() and np.isnan(host[-1024:]).all()
        assert np.array_equal(host[1024:-1024].reshape(start.shape), start + np_regions(planes, w, regions)), (n_rows, n_cols)


@pytest.mark.parametrize("n_rows, words, n_cols", [(129, 2 * SPAN + 1, 16), (17, 3, 1), (16, SPAN + 1, 15)])
def test_weights_outside_the_regions_are_not_read(ctx, n_rows, words, n_cols):
    rng = np.random.default_rng(n_rows)
    bits = 32 * words
    regions = regions_of(rng, words)
    # positions 8 .. 13 belong to no region, with a region that ends at the hole and one that begins behind it in its word
    regions = np.concatenate([regions[(regions[:, 0] >= 14) | (regions[:, 1] <= 8)], [(3, 8), (14, bits)]])
    covered = np.zeros(bits, bool)
    for lo, hi in regions:
        covered[lo:hi] = True
    assert covered[3:8].all() and not covered[8:14].any() and covered[14:].all()
    w = rng.integers(-8, 9, (3, bits, n_cols)) / 4.0
    planes, _ = random_vplanes(rng, n_rows, words)
    holes = w.copy()
    holes[:, ~covered] = np.nan
    assert np.array_equal(run(ctx, planes, holes, regions).cpu().numpy(), np_regions(planes, w, regions))


@pytest.mark.parametrize("n_rows, words, n_cols", [(130, 2 * SPAN + 1, 13), (65, SPAN + 1, 16), (17, 3, 1)])
def test_kernel_error_bound_and_determinism_on_real_weights(ctx, n_rows, words, n_cols):
    """an entry that sums m values is within m 2^-52 sum |w| of numpy's float64 sum: hhgt_region_sums' first-order bound
    (m - 1) 2^-53 sum |w|, doubled for the second-order terms and for numpy's own summation (hhgt_score_sums' test derives
    the same).  And a region gives the same bits on two calls, alone, among others and with the table's regions permuted"""
    rng = np.random.default_rng(n_rows)
    regions = regions_of(rng, words)
    w = rng.normal(size=(3, 32 * words, n_cols))
    planes, _ = random_vplanes(rng, n_rows, words)
    want, total = np_regions(planes, w, regions), np_regions(planes, np.abs(w), regions)
    ones = np.ones((3, 32 * words, 1))
    m = np_regions(planes, ones, regions)                                                # values summed per (row, region)
    got, again = run(ctx, planes, w, regions), run(ctx, planes, w, regions)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))
    err, bound = np.abs(got.cpu().numpy() - want), m * 2.0 ** -52 * total
    print(f"region_sums {n_rows} x {32 * words} x {n_cols}: largest error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
    assert (err <= bound).all()
    perm = rng.permutation(len(regions))
    permuted = run(ctx, planes, w, regions[perm])
    assert torch.equal(permuted.view(torch.int64), got[:, torch.from_numpy(perm).to(ctx.device)].view(torch.int64))
    longest = int(np.argmax(regions[:, 1] - regions[:, 0]))
    for r in (0, longest, len(regions) - 1):
        alone = run(ctx, planes, w, regions[r:r + 1])
        assert torch.equal(alone[:, 0].view(torch.int64), got[:, r].view(torch.int64)), r


@pytest.mark.parametrize("n_rows, words", [(129, 2 * SPAN + 1), (16, 2)])
def test_kernel_agrees_with_score_sums_over_one_hot_columns(ctx, n_rows, words):
    """the second device route: column r of hhgt_score_sums' weights carries the region's weights inside region r and
    zeros outside.  Quarters: both are exact"""
    rng = np.random.default_rng(words)
    regions = regions_of(rng, words)[-64:]
    w = rng.integers(-8, 9, (3, 32 * words, 3)) / 4.0
    planes, _ = random_vplanes(rng, n_rows, words)
    got = run(ctx, planes, w, regions)
    inside = np.zeros((32 * words, len(regions)))
    for r, (lo, hi) in enumerate(regions):
        inside[lo:hi, r] = 1.0
    for c in range(w.shape[2]):
        one_hot = np.ascontiguousarray(w[:, :, c:c + 1] * inside[None])
        other = ctx.score_sums(device_planes(ctx, planes), torch.from_numpy(one_hot).to(ctx.device))
        assert torch.equal(other, got[:, :, c]), c


def test_no_bit_and_every_bit(ctx):
    n_rows, words, n_cols = 130, 2 * SPAN + 1, 5
    rng = np.random.default_rng(3)
    regions = regions_of(rng, words)
    w = rng.integers(-8, 9, (3, 32 * words, n_cols)) / 4.0
    totals = np.stack([w[:, lo:hi].sum(axis=(0, 1)) for lo, hi in regions])              # the class totals of each region
    for fill, want in ((0, np.zeros_like(totals)), (-1, totals)):
        full = np.full((3, n_rows, words), fill, np.int32).view(np.uint32)
        assert np.array_equal(run(ctx, full, w, regions).cpu().numpy(), np.broadcast_to(want, (n_rows,) + want.shape))
    # no piece, and no row: nothing is touched
    planes, _ = random_vplanes(rng, n_rows, words)
    nan = torch.full((n_rows, 2, n_cols), float("nan"), dtype=torch.float64, device=ctx.device)
    assert torch.isnan(run(ctx, planes, w, np.array([(5, 5), (9, 2)]), sums=nan)).all()
    assert tuple(run(ctx, planes[:, :0], w, regions).shape) == (0, len(regions), n_cols)


def test_kernel_arguments(ctx):
    dev = ctx.device
    planes = torch.zeros((3, 5, 2), dtype=torch.int32, device=dev)
    w = torch.ones((3, 64, 3), dtype=torch.float64, device=dev)
    pieces, runs, n_slots = plan(np.array([(0, 64), (3, 40)]), 2)
    args = dict(planes=planes, w=w, pieces=pieces, runs=runs, n_slots=n_slots, n_regions=2)
    assert tuple(ctx.region_sums(**args).shape) == (5, 2, 3)
    for n_cols in (0, REGION_MAX_COLS + 1):
        with pytest.raises(HhgtError, match="columns"):
            ctx.region_sums(**{**args, "w": torch.ones((3, 64, n_cols), dtype=torch.float64, device=dev)})
    # the tables are checked on the device: a piece past the row, the wrong way round, longer than a piece may be, of a
    # region or a slot that does not exist, and a run past the slots — none of them touches the sums
    long_planes = torch.zeros((3, 5, SPAN + 2), dtype=torch.int32, device=dev)
    long_w = torch.ones((3, 32 * (SPAN + 2), 3), dtype=torch.float64, device=dev)
    for bad_piece, extra in (((0, 65, 0, PIECE_DIRECT), {}), ((40, 3, 0, PIECE_DIRECT), {}), ((-1, 3, 0, PIECE_DIRECT), {}),
                             ((0, 64, 2, PIECE_DIRECT), {}), ((0, 64, -1, PIECE_DIRECT), {}), ((0, 64, 0, 0), {}), ((0, 64, 0, -2), {}),
                             ((0, 32 * SPAN + 1, 0, PIECE_DIRECT), dict(planes=long_planes, w=long_w)),
                             ((31, 32 * SPAN + 32, 0, PIECE_DIRECT), dict(planes=long_planes, w=long_w))):
        sums = torch.full((5, 2, 3), 7.0, dtype=torch.float64, device=dev)
        with pytest.raises(HhgtError, match="pieces or runs"):
            ctx.region_sums(**{**args, **extra, "pieces": np.array([bad_piece], np.int64), "runs": np.zeros((0, 3), np.int64),
                               "n_slots": 0, "sums": sums})
        assert (sums == 7.0).all(), bad_piece
    two = np.array([(0, 32, 0, 0), (32, 64, 0, 1)], np.int64)
    for bad_run in ((0, 1, 2), (2, 0, 2), (0, -1, 1), (0, 0, 3)):
        with pytest.raises(HhgtError, match="pieces or runs"):
            ctx.region_sums(**{**args, "pieces": two, "runs": np.array([bad_run], np.int64), "n_slots": 2})
    ones = torch.full_like(planes, -1)                      # every bit of three planes under weights of 1: 3 x 64
    assert ctx.region_sums(**{**args, "planes": ones, "pieces": two, "runs": np.array([(1, 0, 2)], np.int64), "n_slots": 2})[:, 1].eq(192.0).all()
    d_pieces = torch.from_numpy(pieces).to(dev)
    for kw in (dict(w=w.float()), dict(w=w[:, :63]), dict(w=w[:2]), dict(w=w.cpu()), dict(w=w[:, :, 0]),
               dict(w=torch.ones((3, 64, 6), dtype=torch.float64, device=dev)[:, :, ::2]),
               dict(planes=planes.float()), dict(planes=planes[:2]), dict(planes=planes[:, :, :1]),
               dict(pieces=pieces.astype(np.int32)), dict(pieces=pieces[:, :3]), dict(pieces=d_pieces.cpu()), dict(pieces=d_pieces.int()),
               dict(runs=np.zeros((0, 4), np.int64)), dict(runs=torch.zeros((0, 3), dtype=torch.int32, device=dev)),
               dict(sums=torch.zeros((5, 2, 3), dtype=torch.float32, device=dev)),
               dict(sums=torch.zeros((5, 3, 3), dtype=torch.float64, device=dev)),
               dict(sums=torch.zeros((5, 2, 3), dtype=torch.float64)),
               dict(sums=torch.zeros((5, 2, 6), dtype=torch.float64, device=dev)[:, :, ::2])):
        with pytest.raises(ValueError):
            ctx.region_sums(**{**args, **kw})
    # device tables are taken as they are; without the wait the call is asynchronous and gives the same sums
    a = ctx.region_sums(**{**args, "pieces": d_pieces, "runs": torch.from_numpy(runs).to(dev), "wait": False})
    assert torch.equal(a, ctx.region_sums(**args))
