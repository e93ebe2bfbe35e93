"""-m gpu: LD between nearby variants.  hhgt_variant_planes (the bit transposition) against numpy unpackbits / transpose, in
one tile of 256 plane rows and in up to three, between sentinel words;
hhgt_ld_counts (32 x 32 tiles of the band, popcounts of ANDs) against the numpy restatement on random planes — tile edges,
windows across one and several tiles, calls accumulating, the samples split over two buffers; hhgt_ld_prune (decisions, then
the walk of one wave) against the numpy walk, in one tile and in three with carry-in; GenotypeStore.ld_counts / ld_r2 /
ld_prune on stores written from a known matrix in three geometries (one with padded blocks), directory and exported .h5 —
sample lists, sub-ranges, MAF masks, seams in every block, the read cache untouched, the pruned mask fed to pair_counts;
VCFH5Reader.ld_prune and the ld_prune CLI.  Windows past 65 up to the limit of 1024: hhgt_ld_counts with up to 33 tile rows, hhgt_ld_prune with
4, 8 and 16 register words on the long-range recipe of tests/test_ld_plan.py (far_genotypes), its decisions at counts up to
2^30 against exact integers and at exact ties, and the store with a window wider than its plane windows and tiles."""
import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd import device as dev
from haplohyped_varawareml_amd._lib import HhgtError
from haplohyped_varawareml_amd.store import (LD_HM, LD_MH, GenotypeStore, StoreWriter, export_h5, ld_exceeds, plan_planes,
                                             plane_rows)
from tests.test_gpu_sample_counts import np_variant_mask
from tests.test_ld_plan import (FAR_V, FAR_WINDOWS, check_r2, exact_decisions, far_cohort, ld_genotypes, np_exceeds,
                                np_ld_table, np_products, np_prune, np_r2, scaled_entries, tie_entries, walk_words)
from tests.test_pair_count_plan import np_pair_table

pytestmark = pytest.mark.gpu


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


def to_dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(ctx.device)


# ---- hhgt_variant_planes ---------------------------------------------------------------------------------------------------

def np_transpose(planes, w_lo, w_hi):
    """uint32 [3, n, W] (HET, REF, ALT) -> uint32 [3, 32 (w_hi - w_lo), ceil(n / 32)] (HET, COMPLETE, ALT)"""
    n = planes.shape[1]
    src = np.stack([planes[0], planes[0] | planes[1] | planes[2], planes[2]])[:, :, w_lo:w_hi]
    bits = np.unpackbits(np.ascontiguousarray(src).view(np.uint8), axis=2, bitorder="little")      # [3, n, 32 words]
    sw = -(-n // 32)
    t = np.zeros((3, bits.shape[2], sw * 32), np.uint8)
    t[:, :, :n] = bits.transpose(0, 2, 1)
    return np.packbits(t, axis=2, bitorder="little").view(np.uint32).reshape(3, bits.shape[2], sw)


@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 64, 65, 130])
@pytest.mark.parametrize("row_words", [1, 3, 33])
def test_variant_planes_match_numpy(ctx, n_rows, row_words):
    rng = np.random.default_rng(n_rows * 100 + row_words)
    cls = rng.integers(0, 5, (n_rows, row_words * 32))                       # 3, 4: not complete; classes are disjoint
    planes = np.stack([np.packbits(cls == k, axis=1, bitorder="little").view(np.uint32) for k in range(3)])
    d = to_dev(ctx, planes)
    W = row_words
    for w_lo, w_hi in {(0, W), (0, 0), (W - 1, W), (W // 3, max(W // 3, W - 1))}:
        sw = -(-n_rows // 32)
        out = torch.full((3, 32 * (w_hi - w_lo), sw), -1, dtype=torch.int32, device=ctx.device)    # pre-filled with ones
        assert ctx.variant_planes(d, w_lo, w_hi, vplanes=out) is out
        got, want = as_u32(out), np_transpose(planes, w_lo, w_hi)
        assert got.shape == want.shape and np.array_equal(got, want), (w_lo, w_hi)
        if w_hi > w_lo:
            assert np.array_equal(got[1], np_transpose(np.stack([planes[0] | planes[1] | planes[2]] * 3), w_lo, w_hi)[0])
            if n_rows % 32:
                assert not (got[:, :, -1] >> (n_rows % 32)).any()           # bits past n_rows
    assert np.array_equal(as_u32(ctx.variant_planes(d)), np_transpose(planes, 0, W))
    for w_lo, w_hi in ((2, 1), (0, W + 1)):
        with pytest.raises(HhgtError, match="variant_planes"):
            ctx.variant_planes(d, w_lo, w_hi, vplanes=torch.zeros((3, 32 * max(w_hi - w_lo, 0), -(-n_rows // 32)),
                                                                  dtype=torch.int32, device=ctx.device))
    with pytest.raises(ValueError):
        ctx.variant_planes(d, 0, W, vplanes=torch.zeros((3, 32 * W, 99), dtype=torch.int32, device=ctx.device))


GUARD = 1024        # sentinel words on either side of the output


@pytest.mark.parametrize("n_rows", [255, 256, 257, 288, 289, 511, 513, 600])
@pytest.mark.parametrize("row_words", [1, 9, 17])
def test_variant_planes_past_one_row_tile(ctx, n_rows, row_words):
    """k_variant_planes beyond its tile of 256 plane rows x 8 words: all four waves with rows, blockIdx.y up to 2, a last
    tile of one row, of one output word (288: `s0 + 1 < sw` cuts the upper half of a wave's mask in the second tile) and of
    an odd number of them; word ranges of one and of several tiles of 8 words, from a start that is no multiple of 8,
    ending inside a tile.  Guards a wave or a row tile left out or stored to another's words, and a store past the output:
    the output is a view between two stretches of sentinel words that must come back as they were."""
    rng = np.random.default_rng(n_rows * 100 + row_words)
    cls = rng.integers(0, 5, (n_rows, row_words * 32))                       # 3, 4: not complete; classes are disjoint
    planes = np.stack([np.packbits(cls == k, axis=1, bitorder="little").view(np.uint32) for k in range(3)])
    d = to_dev(ctx, planes)
    W, sw = row_words, -(-n_rows // 32)
    ranges = {(0, W), (W - 1, W)} | ({(3, min(W, 12)), (2, 7), (1, W - 2)} if W >= 9 else set())
    for w_lo, w_hi in sorted(ranges):
        size = 3 * 32 * (w_hi - w_lo) * sw
        buf = torch.full((GUARD + size + GUARD,), 0x5a5a5a5a, dtype=torch.int32, device=ctx.device)
        out = buf[GUARD:GUARD + size].view(3, 32 * (w_hi - w_lo), sw)
        out.fill_(-1)                                                        # pre-filled with ones
        assert ctx.variant_planes(d, w_lo, w_hi, vplanes=out) is out
        host = as_u32(buf)
        assert (host[:GUARD] == 0x5a5a5a5a).all() and (host[GUARD + size:] == 0x5a5a5a5a).all(), (w_lo, w_hi)
        got, want = host[GUARD:GUARD + size].reshape(3, 32 * (w_hi - w_lo), sw), np_transpose(planes, w_lo, w_hi)
        assert np.array_equal(got, want), (w_lo, w_hi, np.argwhere(got != want)[:4])
        assert np.array_equal(got[1], np_transpose(np.stack([planes[0] | planes[1] | planes[2]] * 3), w_lo, w_hi)[0])
        if n_rows % 32:
            assert not (got[:, :, -1] >> (n_rows % 32)).any()               # bits past n_rows


# ---- hhgt_ld_counts --------------------------------------------------------------------------------------------------------

def random_vplanes(rng, n_var, sw):
    """disjoint variant-major planes H, M, A-like: per variant its own class mix -> (uint32 [3, n_var, sw], classes)"""
    p = rng.dirichlet(np.ones(4), n_var)                                     # HOM_REF, HET, HOM_ALT, not complete
    u = rng.random((n_var, sw * 32))
    cls = (u[:, :, None] > np.cumsum(p, axis=1)[:, None, :]).sum(2)          # 0..3 (4 by rounding: not complete)
    h, a = cls == 1, cls == 2
    m = cls <= 2
    pack = lambda x: np.packbits(x, axis=1, bitorder="little").view(np.uint32)
    return np.stack([pack(h), pack(m), pack(a)]), (m, h, a)


def np_ld_from_classes(m, h, a, window):
    n = m.shape[0]
    t = np.zeros((n, window, 8), np.int64)
    for d in range(min(window, n - 1)):
        u = np.arange(n - 1 - d)
        v = u + 1 + d
        for c, x in enumerate([m[u] & m[v], h[u] & m[v], a[u] & m[v], m[u] & h[v], m[u] & a[v], h[u] & h[v],
                               (h[u] & a[v]) | (a[u] & h[v]), a[u] & a[v]]):
            t[u, d, c] = x.sum(1)
    return t


@pytest.mark.parametrize("n_var", [1, 2, 63, 64, 65, 200])
@pytest.mark.parametrize("window", [1, 7, 64, 65])
def test_ld_counts_match_numpy(ctx, n_var, window):
    for sw in (1, 3, 80):
        rng = np.random.default_rng(n_var * 1000 + window * 10 + sw)
        vp, (m, h, a) = random_vplanes(rng, n_var, sw)
        want = np_ld_from_classes(m, h, a, window)
        if n_var >= 63:
            assert (want[..., LD_HM] != want[..., LD_MH]).any()              # a swapped (u, v) would show
        d = to_dev(ctx, vp)
        table = ctx.ld_counts(d, window)
        assert table.dtype == torch.int32 and tuple(table.shape) == (n_var, window, 8)
        got = table.cpu().numpy()
        assert np.array_equal(got, want), (n_var, window, sw)
        k, dd = np.arange(n_var)[:, None], np.arange(window)[None, :]
        assert not got[(k + 1 + dd >= n_var)].any()                          # past the end
        assert ctx.ld_counts(d, window, table=table) is table                # a second call adds
        assert np.array_equal(table.cpu().numpy(), 2 * want)
        if sw > 1:                                                           # the samples split over two buffers
            half = sw // 2
            t2 = ctx.ld_counts(to_dev(ctx, vp[:, :, :half]), window)
            ctx.ld_counts(to_dev(ctx, vp[:, :, half:]), window, table=t2)
            assert np.array_equal(t2.cpu().numpy(), want)


WIDE = [(w, n) for w in (66, 96, 97, 128, 129, 1000, 1024)
        for n in sorted({40, w, w + 1, w + 33} | ({1100} if w == 1024 else set()))]


@pytest.mark.parametrize("window,n_var", WIDE)
def test_ld_counts_wide_windows(ctx, window, n_var):
    """hhgt_ld_counts with 4 to 33 tile rows in blockIdx.y: the ownership cut j - i > window where the window is no
    multiple of 32, fewer variants than the window, the entry addressing (i * window + d) * 2 at wide rows.  Guards
    `d < window` off by one (an entry at distance window + 1 written, or the one at distance window left out) and a pair
    owned by two workgroups or by none.  Exact, into a table pre-filled with a pattern: what the call does not own it does
    not touch."""
    k, dd = np.arange(n_var)[:, None], np.arange(window)[None, :]
    past = k + 1 + dd >= n_var
    pattern = (np.arange(n_var * window * 8, dtype=np.int64) % 1009 + 1).astype(np.int32).reshape(n_var, window, 8)
    for sw in (1, 3):
        rng = np.random.default_rng(n_var * 1000 + window * 10 + sw)
        vp, (m, h, a) = random_vplanes(rng, n_var, sw)
        want = np_ld_from_classes(m, h, a, window)
        assert (want[..., LD_HM] != want[..., LD_MH]).any() and past.any() and not want[past].any()
        d = to_dev(ctx, vp)
        table = torch.from_numpy(pattern).to(ctx.device)
        assert ctx.ld_counts(d, window, table=table) is table
        got = table.cpu().numpy()
        assert np.array_equal(got[past], pattern[past])                      # past the end: untouched
        assert np.array_equal(got, pattern + want), (n_var, window, sw)
        assert ctx.ld_counts(d, window, table=table) is table                # a second call adds
        assert np.array_equal(table.cpu().numpy(), pattern + 2 * want)
        assert np.array_equal(ctx.ld_counts(d, window).cpu().numpy(), want)  # the default table: zeros
        if sw > 1:                                                           # the samples split over two buffers
            half = sw // 2
            t2 = ctx.ld_counts(to_dev(ctx, vp[:, :, :half]), window)
            ctx.ld_counts(to_dev(ctx, vp[:, :, half:]), window, table=t2)
            assert np.array_equal(t2.cpu().numpy(), want)


def test_ld_counts_constant_planes_and_bad_windows(ctx):
    n_var, window, sw = 70, 40, 3
    zeros = torch.zeros((3, n_var, sw), dtype=torch.int32, device=ctx.device)
    assert not ctx.ld_counts(zeros, window).any()
    ones = torch.full((3, n_var, sw), -1, dtype=torch.int32, device=ctx.device)
    got = ctx.ld_counts(ones, window).cpu().numpy()
    k, d = np.arange(n_var)[:, None], np.arange(window)[None, :]
    inside = k + 1 + d < n_var
    assert (got[inside] == 32 * sw).all() and not got[~inside].any()         # every column, the OR of column 6 included
    for bad in (0, 1025):
        with pytest.raises(HhgtError, match="ld_counts"):
            ctx.ld_counts(zeros, bad)
    with pytest.raises(ValueError):
        ctx.ld_counts(zeros, window, table=torch.zeros((n_var, window + 1, 8), dtype=torch.int32, device=ctx.device))


# ---- hhgt_ld_prune ---------------------------------------------------------------------------------------------------------

S, V = 130, 600


@pytest.fixture(scope="module")
def recipe():
    """the correlated genotypes, and per window their LD table (computed once, never changed)"""
    g = ld_genotypes(1, S, V)
    return dict(g=g, tables={w: np_ld_table(g, w) for w in (1, 7, 50, 64, 65)})


def padded(table, window, a, b):
    """rows [a - window, b) of an LD table as hhgt_ld_prune takes a tile: zeros before the first variant"""
    out = np.zeros((window + b - a, window, 8), np.int32)
    lo = max(a - window, 0)
    out[window - (a - lo):] = table[lo:b]
    return out


@pytest.mark.parametrize("window", [1, 7, 50, 64, 65])
def test_ld_prune_kernel_matches_numpy_walk(ctx, recipe, window):
    table = recipe["tables"][window]
    r2 = np_r2(table)
    assert np.isnan(r2[:V - window]).any() and (r2 == 1.0).any()             # (a duplicate lies right behind its original)
    # the data decide something: at 0.2 between 20 % and 80 % stay, a higher threshold keeps more, and at 0.999999 only
    # the exact duplicates go (one lies one place on, one three places on: window 1 does not reach the second)
    n_kept = [int(np_prune(table, t).sum()) for t in (0.2, 0.8, 0.999999)]
    assert 0.2 * V <= n_kept[0] <= 0.8 * V and n_kept[0] < n_kept[1] < n_kept[2] == (V - 2 if window >= 3 else V - 1), n_kept
    for t in (0.2, 0.8, 0.999999):
        want = np_prune(table, t)
        assert np.array_equal(ld_exceeds(to_dev(ctx, table.astype(np.int32)), t).cpu().numpy(), np_exceeds(table, t))
        keep = ctx.ld_prune(to_dev(ctx, padded(table, window, 0, V)), t)
        assert keep.dtype == torch.uint8 and tuple(keep.shape) == (window + V,)
        got = keep.cpu().numpy()
        assert not got[:window].any() and set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got[window:].astype(bool), want), (window, t)
        # three tiles, the flags of the last `window` variants carried in
        flags = np.zeros(window, np.uint8)
        parts = []
        for a, b in ((0, 130), (130, 131), (131, V)):
            buf = torch.from_numpy(np.concatenate([flags, np.full(b - a, 7, np.uint8)])).to(ctx.device)
            out = ctx.ld_prune(to_dev(ctx, padded(table, window, a, b)), t, keep=buf).cpu().numpy()
            assert np.array_equal(out[:window], flags)
            parts.append(out[window:])
            flags = np.concatenate([flags, out[window:]])[-window:]
        assert np.array_equal(np.concatenate(parts).astype(bool), want), (window, t)


@pytest.fixture(scope="module")
def far():
    """the long-range cohort and its table at window 1024 (tests/test_ld_plan.py proves on the CPU that it bites)"""
    return far_cohort()


def prune_in_tiles(ctx, table, window, t, cuts):
    """hhgt_ld_prune over the tiles [cuts[i], cuts[i + 1]), the flags of the last `window` variants carried in -> bool"""
    flags = np.zeros(window, np.uint8)
    parts = []
    for a, b in zip(cuts, cuts[1:]):
        buf = torch.from_numpy(np.concatenate([flags, np.full(b - a, 7, np.uint8)])).to(ctx.device)
        out = ctx.ld_prune(to_dev(ctx, padded(table, window, a, b)), t, keep=buf).cpu().numpy()
        assert np.array_equal(out[:window], flags) and set(np.unique(out[window:])) <= {0, 1}
        parts.append(out[window:])
        flags = np.concatenate([flags, out[window:]])[-window:]
    return np.concatenate(parts).astype(bool)


@pytest.mark.parametrize("window", FAR_WINDOWS)
def test_ld_prune_wide_registers(ctx, far, window):
    """k_ld_walk<2>, <4>, <8>, <16> (and k_ld_exceeds with as many words per variant) on the recipe whose every register
    word decides alone: guards an upper register word dropped or its carry K[q - 1] >> 63 lost, the initial load of the
    upper words from carried flags, the padded bits of a register wider than the window, and `d < window` off by one (a copy
    at distance window goes, one at window + 1 stays).  In one tile and in four, one of them shorter than the window and one
    cut between u and v of the chain, so that v stays because of a carried flag of 0 far back."""
    table = far["table"][:, :window]
    u0, u, v = far["chains"][window]
    cuts = [0, window + 70, window + 71, max(u + 1, window + 200), FAR_V]
    assert cuts == sorted(set(cuts)) and u < cuts[3] <= v
    n_in_reach = sum(D <= window for D, _, _ in far["dups"])
    assert walk_words(window) == {128: 2, 129: 4, 256: 4, 300: 8, 512: 8, 513: 16, 1024: 16}[window]
    dev_table = to_dev(ctx, table)
    whole = to_dev(ctx, padded(table, window, 0, FAR_V))
    for t in (0.5, 0.999999):
        want = np_prune(table, t)
        assert (want[u0], want[u], want[v]) == (True, False, True) and (~want).sum() >= n_in_reach
        assert np.array_equal(ld_exceeds(dev_table, t).cpu().numpy(), np_exceeds(table, t))
        got = ctx.ld_prune(whole, t).cpu().numpy()
        assert not got[:window].any() and set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got[window:].astype(bool), want), (window, t, np.nonzero(got[window:] != want)[0])
        assert np.array_equal(prune_in_tiles(ctx, table, window, t, cuts), want), (window, t)


@pytest.mark.parametrize("window", FAR_WINDOWS)
def test_ld_prune_carried_flags_of_ones(ctx, far, window):
    """the initial load K[q] = ballot(d < window && keep[window - 1 - d]) in every word: carried flags of 1 over table rows of
    zeros prune nothing; a single carried variant at distance exactly `window` — the last bit in reach — prunes its
    duplicate iff its flag is 1; one at window + 1 is not seen.  Guards `d < window` off by one and an upper word not
    loaded."""
    table = far["table"][:, :window]
    n = 70
    keep = torch.from_numpy(np.concatenate([np.ones(window, np.uint8), np.full(n, 7, np.uint8)])).to(ctx.device)
    out = ctx.ld_prune(torch.zeros((window + n, window, 8), dtype=torch.int32, device=ctx.device), 0.5, keep=keep)
    assert out.cpu().numpy().tolist() == [1] * (window + n)
    by_distance = {D: (orig, copy) for D, orig, copy in far["dups"]}
    orig, copy = by_distance[window]
    tile = to_dev(ctx, padded(table, window, copy, copy + 1))           # row 0 is the original, `window` places back
    assert copy - orig == window and np_exceeds(table, 0.5)[orig, window - 1]
    one, rest = np.zeros(window, np.uint8), np.ones(window, np.uint8)
    one[0], rest[0] = 1, 0
    for flags, kept in ((one, 0), (np.zeros(window, np.uint8), 1), (rest, 1), (np.ones(window, np.uint8), 0)):
        buf = torch.from_numpy(np.concatenate([flags, np.full(1, 7, np.uint8)])).to(ctx.device)
        out = ctx.ld_prune(tile, 0.5, keep=buf).cpu().numpy()
        assert np.array_equal(out[:window], flags) and out[window] == kept, (window, flags[:2], kept)
    orig, copy = by_distance[window + 1]                                # out of reach: nothing in the tile's rows exceeds
    buf = torch.from_numpy(np.concatenate([np.ones(window, np.uint8), np.full(1, 7, np.uint8)])).to(ctx.device)
    assert ctx.ld_prune(to_dev(ctx, padded(table, window, copy, copy + 1)), 0.5, keep=buf).cpu().numpy()[window] == 1


def device_decisions(ctx, entries, t, window=64):
    """exceeds of each entry [n, 8] as hhgt_ld_prune decides it, one by one: blocks of one variant whose table row holds
    `window` of the entries, followed by `window` variants whose rows are zeros — the first is kept (the rows before it
    decide nothing), follower j is pruned iff entry j - 1 of the row exceeds, and lane d of a wave decides entry d
    -> bool [n]"""
    e = np.asarray(entries).reshape(-1, 8)
    n, blocks = len(e), -(-len(e) // window)
    assert e.min() >= 0 and e.max() < 1 << 30
    rows = np.zeros((blocks * window, 8), np.int32)
    rows[:n] = e
    tab = np.zeros((window + blocks * (window + 1), window, 8), np.int32)
    tab[window + np.arange(blocks) * (window + 1)] = rows.reshape(blocks, window, 8)
    keep = ctx.ld_prune(to_dev(ctx, tab), t).cpu().numpy()
    assert not keep[:window].any() and set(np.unique(keep)) <= {0, 1}
    keep = keep[window:].reshape(blocks, window + 1)
    assert keep[:, 0].all()
    return (keep[:, 1:] == 0).reshape(-1)[:n]


def test_ld_prune_decides_in_int64_at_large_counts(ctx):
    """ld_exceeds of csrc/ld.hip at counts up to 2^30 - 1, where N sxy passes 2^57: guards a 32-bit (or float32) product
    anywhere in n * sxy - sx * sy, which every table of 130 samples passes.  The decisions equal np_exceeds bit for bit,
    and the exact ones (Python integers, fractions.Fraction(t); tests/test_ld_plan.py checks np_exceeds against them)
    outside the near ties, which are at most 1 %.  With 8 register words too: the unit / nq, unit % nq split and the
    d < window cut inside a word."""
    small, big = scaled_entries()
    table = big.reshape(600, 7, 8)
    assert (np_products(big)[0] > 2.0 ** 100).any()
    for t in (0.0, 0.2, 0.5, 1.0):
        ex, near = exact_decisions(big, t)
        assert near.mean() <= 0.01 and np.array_equal(ex, exact_decisions(small, t)[0])
        want = np_exceeds(big, t)
        for window in (64, 300):
            got = device_decisions(ctx, big, t, window)
            assert np.array_equal(got, want), (t, window, np.nonzero(got != want)[0][:10])
            assert np.array_equal(got[~near], ex[~near]), (t, window)
        assert np.array_equal(ld_exceeds(to_dev(ctx, big.astype(np.int32)), t).cpu().numpy(), want)
        keep = ctx.ld_prune(to_dev(ctx, padded(table, 7, 0, 600)), t).cpu().numpy()[7:].astype(bool)
        assert np.array_equal(keep, np_prune(table, t)) and np.array_equal(keep, np_prune(small.reshape(600, 7, 8), t))
        assert keep.all() == (t == 1.0)


def test_ld_prune_ties_and_the_ends_of_the_range(ctx, far):
    """the contract says >: guards `>=` in place of `>`.  An entry whose r^2 is exactly t (1/4 or 1, at small counts and
    near 2^30) does not exceed, one ulp below t it does; at 0 every entry with num != 0 exceeds and none with num = 0; at 1
    nothing exceeds, and the walk keeps every variant, duplicates included."""
    entries, r2 = tie_entries()
    below = lambda x: float(np.nextafter(x, 0.0))
    for window in (64, 129):
        dec = lambda t: device_decisions(ctx, entries, t, window)
        assert not dec(1.0).any() and np.array_equal(dec(below(1.0)), r2 == 1.0)
        assert np.array_equal(dec(0.25), r2 == 1.0) and dec(below(0.25)).all()
        assert np.array_equal(dec(float(np.nextafter(0.25, 1.0))), r2 == 1.0) and dec(0.0).all()
    small, big = scaled_entries()
    every = np.concatenate([entries, small, big])
    num_is_0 = np_products(every)[0] == 0
    assert num_is_0.any() and not num_is_0.all()
    assert np.array_equal(device_decisions(ctx, every, 0.0), ~num_is_0)
    assert not device_decisions(ctx, every, 1.0).any()
    table = far["table"][:, :129]
    assert (np_r2(table) == 1.0).sum() >= sum(D <= 129 for D, _, _ in far["dups"]) >= 9
    assert ctx.ld_prune(to_dev(ctx, padded(table, 129, 0, FAR_V)), 1.0).cpu().numpy()[129:].all()


def test_ld_prune_kernel_refuses(ctx):
    table = torch.zeros((10, 4, 8), dtype=torch.int32, device=ctx.device)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(HhgtError, match="ld_prune"):
            ctx.ld_prune(table, bad)
    with pytest.raises(ValueError):
        ctx.ld_prune(table, 0.2, keep=torch.zeros(9, dtype=torch.uint8, device=ctx.device))
    with pytest.raises(ValueError):
        ctx.ld_prune(torch.zeros((3, 4, 8), dtype=torch.int32, device=ctx.device), 0.2)
    assert ctx.ld_prune(table, 0.2).cpu().numpy().tolist() == [0] * 4 + [1] * 6      # nothing exceeds: all kept


# ---- the store -------------------------------------------------------------------------------------------------------------

GROUP = "chr_7"
GEOMS = [(64, 128, 1500), (64, 8192, 9000), (64, 100, 700)]                 # sc, vc, V; the last: 100 variants in 4 words
PICK = [5, 129, 70, 5, 3, 64]                                               # chunk rows 0, 1, 2; sample 5 twice
SPARSE = [5, 129, 5, 3]                                                     # chunk rows 0 and 2 only: plane rows are compacted


def write_store(ctx, path, g, sc, vc):
    """a directory store of int8 [S, V, 2] in chunks of sc x vc, compressed on the device"""
    n_s, n_v = g.shape[:2]
    n_vcol, n_scol = -(-n_v // vc), -(-n_s // sc)
    raw = np.zeros((n_vcol, n_scol, sc, vc, 2), np.int8)
    for vi in range(n_vcol):
        for si in range(n_scol):
            sub = g[si * sc:(si + 1) * sc, vi * vc:(vi + 1) * vc]
            raw[vi, si, :sub.shape[0], :sub.shape[1]] = sub
    src = torch.from_numpy(raw.reshape(-1).view(np.uint8)).to(ctx.device)
    dst, off, total = ctx.compress(src, sc * vc * 2, typesize=2, blocksize=min(vc * 2, 8192), fmt=dev.BLOSC1)
    w = StoreWriter(path, [f"d{i:03d}" for i in range(n_s)], sc, vc, cohort_name="c", chunk_format="blosc1")
    w.begin_group(GROUP)
    w.add_chunks(dst[:total].cpu().numpy(), off.cpu().numpy().astype(np.uint64), raw.size)
    w.add_variants(np.arange(n_v, dtype=np.uint32) * 3 + 10, np.full(n_v, ord("A"), np.uint8), np.full(n_v, ord("G"), np.uint8))
    w.add_chrom_runs([(0, "chr7")])
    w.end_group()
    w.close()


@pytest.fixture(scope="module")
def stores(ctx, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ld")
    out = []
    for sc, vc, n_v in GEOMS:
        g = ld_genotypes(vc, 130, n_v)
        d = str(tmp / f"c{vc}.hhgt")
        write_store(ctx, d, g, sc, vc)
        out.append(dict(g=g, sc=sc, vc=vc, V=n_v, paths=[d, export_h5(d, str(tmp / f"c{vc}.h5"))]))
    return dict(geoms=out, tmp=tmp)


_EXPECTED = {}


def check_store(st, g, window, t, samples, a, b, mask_arg=None, mask=None, **kw):
    """ld_counts, ld_r2 and ld_prune of one query against the restatement -> the expected keep mask over [a, b)"""
    ii = np.arange(g.shape[0]) if samples is None else np.array([st._sample_index(x) for x in samples], np.int64)
    counted = np.ones(b - a, bool) if mask is None else mask
    key = (id(g), window, t, tuple(ii), a, b, counted.tobytes())
    if key not in _EXPECTED:                                        # computed once, shared by the paths and the budgets
        table = np_ld_table(g[:, a:b], window, samples=ii, variants=counted)
        _EXPECTED[key] = (table, np_prune(table, t))
    want, want_keep = _EXPECTED[key]
    table = st.ld_counts(GROUP, samples, a, b, variant_mask=mask_arg, window=window, **kw)
    assert table.is_cuda and table.dtype == torch.int32 and tuple(table.shape) == (int(counted.sum()), window, 8)
    assert np.array_equal(table.cpu().numpy(), want), (a, b, kw)
    r2 = st.ld_r2(GROUP, samples, a, b, variant_mask=mask_arg, window=window, **kw)
    assert r2.is_cuda and r2.dtype == torch.float64
    check_r2(r2.cpu().numpy(), np_r2(want))
    keep = st.ld_prune(GROUP, samples, a, b, variant_mask=mask_arg, window=window, r2=t,
                       **{k: v for k, v in kw.items() if k != "max_table_bytes"})
    assert keep.is_cuda and keep.dtype == torch.bool and tuple(keep.shape) == (b - a,)
    full = np.zeros(b - a, bool)
    full[counted] = want_keep
    assert np.array_equal(keep.cpu().numpy(), full), (a, b, kw)
    return full


@pytest.mark.parametrize("geom", range(len(GEOMS)))
def test_store_ld(ctx, stores, geom):
    c = stores["geoms"][geom]
    scols, rows = plane_rows(np.array(SPARSE), c["sc"])
    assert scols.tolist() == [0, 2] and rows.tolist() == [5, 65, 5, 3]      # 128 plane rows for 130 samples; 129 -> row 65
    g, n_v, vc = c["g"], c["V"], c["vc"]
    window, t = 50, 0.2
    cut = (vc // 2 + 5, n_v - 7) if vc < 8192 else (4000, 8300)              # inside blocks at both ends
    for path in c["paths"]:
        st = GenotypeStore(path, ctx=ctx)
        whole = check_store(st, g, window, t, None, 0, n_v)
        assert 0.2 * n_v <= whole.sum() <= 0.8 * n_v
        check_store(st, g, window, t, PICK, 0, n_v)                                        # a repeat, out of store order
        kept = check_store(st, g, window, t, SPARSE, 0, n_v)                               # a repeat, chunk row 1 left out
        assert 0.2 * n_v <= kept.sum() <= 0.8 * n_v
        check_store(st, g, 7, 0.8, [f"d{i:03d}" for i in SPARSE], *cut, plane_bytes=1)
        check_store(st, g, 7, 0.8, [f"d{i:03d}" for i in PICK], *cut)
        check_store(st, g, window, t, None, 11, 11)                                        # an empty range
        check_store(st, g, window, t, [], 0, 40)                                           # no sample: nothing exceeds
        vm = st.variant_mask(GROUP, PICK, *cut, min_maf=0.1)
        maf = np_variant_mask(g[np.unique(PICK), cut[0]:cut[1]], min_maf=0.1)
        assert np.array_equal(vm.cpu().numpy(), maf) and 50 < maf.sum() < len(maf)
        kept = check_store(st, g, 7, t, PICK, *cut, mask_arg=vm, mask=maf)                  # a device tensor
        check_store(st, g, 7, t, PICK, *cut, mask_arg=maf, mask=maf)                        # a host array
        assert not kept[~maf].any() and 0 < kept.sum() < maf.sum()
        # seams in every block, small slabs, both
        for kw in (dict(plane_bytes=1), dict(slab_bytes=3000), dict(plane_bytes=1, slab_bytes=3000)):
            check_store(st, g, window, t, None, 0, n_v, **kw)
            check_store(st, g, 65, 0.8, PICK, *cut, **kw)
        # the pruned set as the variant mask of another query
        keep = st.ld_prune(GROUP, PICK, window=window, r2=t)
        pairs = st.pair_counts(GROUP, PICK, variant_mask=keep)
        assert np.array_equal(pairs.cpu().numpy(), np_pair_table(g[np.array(PICK)][:, keep.cpu().numpy()]))
        # the counters
        st.stats.update(ld_plane_blocks=0, ld_pairs=0)
        st.ld_counts(GROUP, PICK, window=window)
        plan = plan_planes(np.array(PICK), 130, c["sc"], vc, n_v, 0, n_v, blocksize=st._blocksize())
        assert st.stats["ld_plane_blocks"] == sum(bin(int(m)).count("1") for m in plan["row_mask"]) > 0
        assert st.stats["ld_pairs"] == n_v * window - window * (window + 1) // 2
        st.ld_prune(GROUP, PICK, 0, 30, window=window)
        assert st.stats["ld_pairs"] == n_v * window - window * (window + 1) // 2 + 30 * 29 // 2
        with pytest.raises(ValueError, match="max_table_bytes"):
            st.ld_counts(GROUP, window=window, max_table_bytes=n_v * window * 32 - 1)
        for bad in (dict(window=0), dict(window=1025), dict(variant_mask=maf[:10])):
            with pytest.raises(ValueError):
                st.ld_counts(GROUP, **bad)
            with pytest.raises(ValueError):
                st.ld_prune(GROUP, **bad)
        with pytest.raises(ValueError):
            st.ld_prune(GROUP, r2=1.5)
        with pytest.raises(KeyError):
            st.ld_counts("chr_6")
        with pytest.raises(KeyError):
            st.ld_prune("chr_6")
        with pytest.raises(IndexError):
            st.ld_counts(GROUP, v_lo=5, v_hi=n_v + 1)
        st.close()


@pytest.fixture(scope="module")
def seam_store(ctx, stores):
    """the padded geometry (100 variants per Blosc block) with two more duplicates, 101 and 250 places behind their
    originals: whether they stay is decided across the seams of two or three plane windows"""
    c = stores["geoms"][2]
    g = c["g"].copy()
    dups = ((300, 401), (370, 620))
    for orig, copy in dups:
        g[:, copy] = g[:, orig]
    path = str(stores["tmp"] / "seam.hhgt")
    write_store(ctx, path, g, c["sc"], c["vc"])
    keep = {w: np_prune(np_ld_table(g, w), 0.2) for w in (50, 129, 300)}
    for w, seen in ((129, (True, False)), (300, (True, True))):         # a condition on the data: the wide window decides
        assert [bool(keep[50][copy] != keep[w][copy]) for _, copy in dups] == list(seen), w
    return dict(g=g, path=path, V=c["V"])


@pytest.mark.parametrize("window", [129, 300])
def test_store_ld_window_wider_than_plane_windows(ctx, seam_store, window):
    """GenotypeStore.ld_counts / ld_r2 / ld_prune with a carry longer than the new rows: at plane_bytes = 1 a plane window is
    one block of 100 variants and a tile 64, so `carry = buf[:, -window:]` spans two to three plane windows, `old` is
    restored over pairs carried more than once, and carry_keep holds flags of several tiles.  Guards a seam losing or
    double-counting pairs (or keep flags) when the carry is longer than the new rows."""
    g, n_v = seam_store["g"], seam_store["V"]
    st = GenotypeStore(seam_store["path"], ctx=ctx)
    pairs = GenotypeStore._ld_pairs(n_v, window)
    assert pairs == n_v * window - window * (window + 1) // 2
    for kw in (dict(plane_bytes=1), dict(), dict(slab_bytes=300_000), dict(plane_bytes=1, slab_bytes=3000)):
        st.stats["ld_pairs"] = 0
        kept = check_store(st, g, window, 0.2, None, 0, n_v, **kw)
        assert st.stats["ld_pairs"] == 3 * pairs                         # ld_counts, ld_r2, ld_prune: once each
        assert 0.1 * n_v <= kept.sum() <= 0.8 * n_v
    check_store(st, g, window, 0.2, PICK, 0, n_v, plane_bytes=1)
    check_store(st, g, window, 0.8, SPARSE, 55, n_v - 7, plane_bytes=1)                     # cut inside blocks at both ends
    st.close()


def test_store_ld_wide_window_under_a_mask_and_in_a_short_range(ctx, stores):
    """window 300 on 128-variant chunks: a variant mask keeping about half (a carried row is a counted variant up to ~600
    places back: four to five chunks), and a range shorter than the window (n < window: every pair of the range).  Guards
    the same seam logic under a mask, and _ld_pairs / the table's shape with fewer variants than the window."""
    c = stores["geoms"][0]
    g, n_v, window = c["g"], c["V"], 300
    mask = np.random.default_rng(5).random(n_v) < 0.5
    n = int(mask.sum())
    assert 0.4 * n_v < n < 0.6 * n_v
    for path in c["paths"]:
        st = GenotypeStore(path, ctx=ctx)
        for kw in (dict(), dict(plane_bytes=1)):
            st.stats["ld_pairs"] = 0
            kept = check_store(st, g, window, 0.2, None, 0, n_v, mask_arg=mask, mask=mask, **kw)
            assert st.stats["ld_pairs"] == 3 * (n * window - window * (window + 1) // 2) == 3 * GenotypeStore._ld_pairs(n, window)
            assert not kept[~mask].any() and 0 < kept.sum() < n
            st.stats["ld_pairs"] = 0
            kept = check_store(st, g, window, 0.2, PICK, 700, 900, **kw)
            assert st.stats["ld_pairs"] == 3 * (200 * 199 // 2) == 3 * GenotypeStore._ld_pairs(200, window)
            assert 0 < kept.sum() < 200
        st.close()


def test_store_ld_leaves_read_cache_alone(ctx, stores):
    c = stores["geoms"][0]
    for path in c["paths"]:
        st = GenotypeStore(path, ctx=ctx)
        a = st.ld_counts(GROUP, PICK).cpu().numpy()
        n = st.stats["count_compressed_bytes_read"]
        assert n > 0 and np.array_equal(st.ld_counts(GROUP, PICK, slab_bytes=3000).cpu().numpy(), a)
        assert st.stats["count_compressed_bytes_read"] == 2 * n      # the same chunks read, once each, per call
        batch = [(GROUP, s, 100 * s % 1000, 100 * s % 1000 + 300) for s in (3, 70, 129)]
        first = [r.cpu().numpy() for r in st.read_windows(batch)]
        keys, used, n = list(st._cache), st._cache_used, st.stats["chunks_read"]
        k = st.ld_prune(GROUP, PICK).cpu().numpy()
        assert np.array_equal(st.ld_counts(GROUP, PICK).cpu().numpy(), a)
        assert list(st._cache) == keys and st._cache_used == used
        again = [r.cpu().numpy() for r in st.read_windows(batch)]
        assert st.stats["chunks_read"] == n                          # served from the cache: nothing read from the file
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        m = st.stats["count_compressed_bytes_read"]
        assert np.array_equal(st.ld_prune(GROUP, [3], v_lo=300, v_hi=400).cpu().numpy(),    # cached chunks are used
                              np_prune(np_ld_table(c["g"][[3], 300:400], 50), 0.2))
        assert st.stats["count_compressed_bytes_read"] == m and k.any()
        st.close()


# ---- reader and CLI --------------------------------------------------------------------------------------------------------

def test_reader_ld_prune_and_cli(ctx, stores):
    from click.testing import CliRunner
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    from haplohyped_varawareml_amd.ld_prune import HEADER, main
    c, tmp = stores["geoms"][0], stores["tmp"]
    g, n_v = c["g"], c["V"]
    donors = [f"d{i:03d}" for i in PICK]
    (tmp / "ld_samples.txt").write_text("\n".join(donors) + "\n")
    idx = np.unique(PICK)
    maf = np_variant_mask(g[idx], min_maf=0.1)
    cases = [(dict(), None, np.ones(n_v, bool), 50, 0.2),
             (dict(donor_ids=donors, min_maf=0.1, window=7, r2=0.8), idx, maf, 7, 0.8),
             (dict(chromosomes=[7], donor_ids=donors), idx, np.ones(n_v, bool), 50, 0.2),
             (dict(donor_ids=donors, window=300, r2=0.5), idx, np.ones(n_v, bool), 300, 0.5)]     # wider than two chunks
    wants = []
    for path in c["paths"]:
        r = VCFH5Reader(path, ctx=ctx)
        for kw, ii, counted, window, t in cases:
            rec = r.ld_prune(**kw)
            keep = np.zeros(n_v, bool)
            keep[counted] = np_prune(np_ld_table(g, window, samples=ii, variants=counted), t)
            assert len(rec) == n_v and np.array_equal(rec["keep"], keep) and np.array_equal(rec["counted"], counted)
            assert set(rec["chrom"]) == {b"chr7"} and np.array_equal(rec["start"], np.arange(n_v) * 3 + 10)
            assert set(rec["ref"]) == {b"A"} and set(rec["alt"]) == {b"G"} and 0 < keep.sum() < counted.sum()
            wants.append(keep)
        with pytest.raises(KeyError):
            r.ld_prune(6)
        with pytest.raises(KeyError):
            r.ld_prune(7, donor_ids=["nobody"])
        r.close()
    out = tmp / "prune.tsv"
    text = lambda keep: HEADER + "".join(f"chr7\t{3 * v + 11}\tA\tG\n" for v in np.nonzero(keep)[0])
    for args, keep in (([], wants[0]),
                       (["--sample_list", str(tmp / "ld_samples.txt"), "--min_maf", "0.1", "--window", "7", "--r2", "0.8"], wants[1]),
                       (["--sample_list", str(tmp / "ld_samples.txt"), "--chromosome", "7"], wants[2])):
        res = CliRunner().invoke(main, ["--h5", c["paths"][1], "--out", str(out)] + args)
        assert res.exit_code == 0, res.output
        assert out.read_text() == text(keep), args
    assert CliRunner().invoke(main, ["--h5", c["paths"][1], "--out", str(out), "--window", "0"]).exit_code != 0
