"""GPU: LD clumping.  hhgt_ld_decisions against the numpy restatement of the link bits, hhgt_ld_clump on crafted bits and on
real tables against store_stats.clump_reference (tests/test_clump_plan.py holds that against a brute force on the CPU and
proves that the recipes bite), GenotypeStore.ld_clump on real stores against the reference on np_ld_table of the same
selection, and VCFH5Reader.clump with the clump command end to end.

k_clump_round and k_clump_owners are compiled at LPV = 2, 4, 8, 16 and 32 lanes per variant, the power of two >= 2 nq with nq =
ceil(window / 64).  The crafted cases run at every window of CLUMP_WINDOWS (tests/clump_cases.py), which reach
    LPV  2: 64 (nq 1)                LPV  4: 65, 128 (nq 2)           LPV  8: 129, 192 (nq 3: two idle lanes), 256 (nq 4)
    LPV 16: 257, 300 (nq 5), 448 (nq 7), 512 (nq 8: a full group)     LPV 32: 513 (nq 9), 960 (nq 15), 1000, 1024 (nq 16)
and at each of them every word on either side decides alone at least once: the strided paths have all their links in one
word q < nq — at its first and at its last usable bit — and every waiting variant has one blocker, behind it under the
identity ranking, ahead of it under the reversed one, for ten rounds (past the host's batch of eight); the gadgets have an
owner found only in word j, for every j of the 2 nq.  tests/test_clump_plan.py holds the expected owners to clump_reference
on the CPU and proves on the numpy round model that a dropped word, a narrower template or a wider group mask shows."""
import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd import store_stats as SS
from haplohyped_varawareml_amd._lib import HhgtError
from haplohyped_varawareml_amd.store import GenotypeStore, export_h5
from tests import clump_cases as CC
from tests.test_clump_plan import SEED, np_linked_back, np_rounds, pack_bits, random_p
from tests.test_gpu_ld import GEOMS, GROUP, PICK, SPARSE, padded, to_dev, write_store
from tests.test_gpu_sample_counts import np_variant_mask
from tests.test_ld_plan import FAR_V, FAR_WINDOWS, far_cohort, ld_genotypes, np_ld_table, np_prune, tie_entries

pytestmark = pytest.mark.gpu

S, V = 130, 600
GUARD = 64                      # sentinel words on either side of the link bits
SENTINEL = 0x5A5A5A5A5A5A5A5A
SENTINEL32 = 0x5A5A5A5A                                                 # around the owners (int32)


@pytest.fixture(scope="module")
def recipe():
    """the correlated genotypes' LD tables per window (computed once, never changed)"""
    g = ld_genotypes(1, S, V)
    return {w: np_ld_table(g, w) for w in (1, 7, 50, 64, 65)}


@pytest.fixture(scope="module")
def far():
    return far_cohort()


_LINKS = {}


def far_links(far, window, r2):
    """np_linked_back of the far recipe, once per (window, r2)"""
    if (window, r2) not in _LINKS:
        _LINKS[window, r2] = np_linked_back(far["table"][:, :window], r2)
    return _LINKS[window, r2]


def padded_pos(pos, window, a, b):
    """the positions of the rows [a - window, b) as hhgt_ld_decisions takes them: zeros before the first variant"""
    out = np.zeros(window + b - a, np.int64)
    lo = max(a - window, 0)
    out[window - (a - lo):] = pos[lo:b]
    return out


def decisions(ctx, table, window, a, b, r2, pos=None, max_dist=None):
    """hhgt_ld_decisions over the tile [a, b) of an LD table, into a buffer between sentinels -> int64 [b - a, nq], host"""
    n, nq = b - a, -(-window // 64)
    buf = torch.full((2 * GUARD + n * nq,), SENTINEL, dtype=torch.int64, device=ctx.device)
    bits = buf[GUARD:GUARD + n * nq].view(n, nq)
    pos_t = None if pos is None else torch.from_numpy(padded_pos(pos, window, a, b)).to(ctx.device)
    out = ctx.ld_decisions(to_dev(ctx, padded(table, window, a, b)), r2, pos_t, max_dist, bits=bits)
    assert out.data_ptr() == bits.data_ptr() and out.dtype == torch.int64 and tuple(out.shape) == (n, nq)
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n * nq:] == SENTINEL).all()
    return host[GUARD:GUARD + n * nq].reshape(n, nq)


def check_decisions(ctx, table, window, r2, want_lb, cuts, pos=None, max_dist=None):
    want = pack_bits(want_lb)
    n = len(table)
    for tiles in ([0, n], cuts):
        got = np.concatenate([decisions(ctx, table, window, a, b, r2, pos, max_dist) for a, b in zip(tiles, tiles[1:])])
        assert np.array_equal(got, want), (window, r2, max_dist, tiles, np.argwhere(got != want)[:5])
        if window % 64:                                                  # bits at or past `window` are 0
            assert not (got.view(np.uint64)[:, -1] >> np.uint64(window % 64)).any()


# ---- hhgt_ld_decisions -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", [1, 7, 50, 64, 65])
def test_ld_decisions_match_numpy(ctx, recipe, window):
    table = recipe[window]
    pos = np.cumsum(np.random.default_rng(3).integers(1, 9, V)).astype(np.int64) + (1 << 33)    # (past 32 bits)
    for r2 in (0.2, 0.5):
        lb = np_linked_back(table, r2)
        assert lb.any() and not lb.all()
        check_decisions(ctx, table, window, r2, lb, [0, 130, 131, V])
        # the distance cut is inclusive: at exactly the distance of the linked pair that lies farthest apart the pair
        # stays, one bp less and it goes; at 0 nothing is linked (no two positions are equal)
        k, d = np.nonzero(lb)
        dist = pos[k] - pos[k - 1 - d]
        D = int(dist.max())
        for max_dist in (0, D, D - 1):
            want = np_linked_back(table, r2, pos, max_dist)
            assert want.sum() == (dist <= max_dist).sum() and (max_dist != D or np.array_equal(want, lb))
            check_decisions(ctx, table, window, r2, want, [0, 130, 131, V], pos, max_dist)
        assert np_linked_back(table, r2, pos, D - 1).sum() < lb.sum() and not np_linked_back(table, r2, pos, 0).any()


@pytest.mark.parametrize("window", [129, 300, 1024])
def test_ld_decisions_wide_windows(ctx, far, window):
    """three to sixteen words per variant, nq = ceil(window / 64) and not the walk's power of two (300: 5 words, not 8); in
    one tile and in three, one of them a single variant, the carried rows `window` deep"""
    table = far["table"][:, :window]
    lb = far_links(far, window, 0.5)
    assert lb[:, window - 1].any() and lb[:, 0].any()                    # a copy at distance exactly `window`, and one at 1
    check_decisions(ctx, table, window, 0.5, lb, [0, window + 70, window + 71, FAR_V])


def test_ld_decisions_at_ties(ctx):
    """the contract says >: on entries whose r^2 is exactly 1/4 or 1 (at small counts and near 2^30) the bit is ld_exceeds
    of the entry — not set at a threshold equal to r^2, set one ulp below it"""
    entries, r2 = tie_entries()
    n, window = len(entries), len(entries)
    table = np.zeros((n + 1, window, 8), np.int64)
    table[0] = entries                                                   # entry d: the pair (variant 0, variant 1 + d)
    tile = to_dev(ctx, padded(table, window, 0, n + 1))
    for t in (1.0, float(np.nextafter(1.0, 0.0)), 0.25, float(np.nextafter(0.25, 0.0)), float(np.nextafter(0.25, 1.0)), 0.0):
        want = SS.ld_exceeds(entries, t)
        got = ctx.ld_decisions(tile, t).cpu().numpy().view(np.uint64)[:, 0]
        assert [int(got[1 + d] >> np.uint64(d)) & 1 for d in range(n)] == want.astype(int).tolist(), t
        assert sum(bin(int(x)).count("1") for x in got) == want.sum()
    assert not SS.ld_exceeds(entries, 0.25)[r2 == 0.25].any() and SS.ld_exceeds(entries, float(np.nextafter(0.25, 0.0))).all()


# ---- hhgt_ld_clump on crafted bits -------------------------------------------------------------------------------------------

def clump_words(ctx, words, window, rank, eligible, guarded=False):
    """hhgt_ld_clump on packed link words int64 [n, nq] -> (owner int64 [n], rounds); guarded: the owners go into a buffer
    between sentinels, and nothing outside them is written"""
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(ctx.device)                # noqa: E731
    n, buf, out = len(words), None, None
    if guarded:
        buf = torch.full((2 * GUARD + n,), SENTINEL32, dtype=torch.int32, device=ctx.device)
        out = buf[GUARD:GUARD + n]
    owner, rounds = ctx.ld_clump(dev(words, np.int64), window, dev(rank, np.int32), dev(eligible, np.uint8), owner=out)
    assert owner.dtype == torch.int32 and tuple(owner.shape) == (n,) and isinstance(rounds, int)
    if guarded:
        host = buf.cpu().numpy()
        assert owner.data_ptr() == out.data_ptr() and (host[:GUARD] == SENTINEL32).all() and (host[GUARD + n:] == SENTINEL32).all()
    return owner.cpu().numpy().astype(np.int64), rounds


def clump(ctx, lb, rank, eligible, guarded=False):
    """hhgt_ld_clump on the link bits of bool [n, window] -> (owner int64 [n], rounds)"""
    return clump_words(ctx, pack_bits(lb), lb.shape[1], rank, eligible, guarded)


def check_clump(ctx, lb, rank, eligible, guarded=False):
    """against clump_reference (p = rank, p1 = the eligible ones' largest) and the numpy rounds"""
    rank, eligible = np.asarray(rank), np.asarray(eligible, bool)
    p = np.where(eligible, rank, rank + 2.0 * len(rank)) / (4.0 * len(rank) + 1.0)     # not eligible: above p1, order kept
    want = SS.clump_reference(lb, p, (len(rank) + 0.5) / (4.0 * len(rank) + 1.0))
    got, rounds = clump(ctx, lb, rank, eligible, guarded)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    want_rounds = np_rounds(lb, rank, eligible)
    assert np.array_equal(want_rounds[0], want) and rounds == want_rounds[1]
    return got, rounds


def test_ld_clump_path_takes_n_rounds(ctx):
    """a path of 300 under the identity ranking: variant k decides in round k + 1 — the worst case of the bound — the
    same on a second call (double-buffered state: a round reads only the round before)"""
    n = 300
    lb = np.zeros((n, 1), bool)
    lb[1:, 0] = True
    for _ in range(2):
        owner, rounds = check_clump(ctx, lb, np.arange(n), np.ones(n))
        assert rounds == n and owner.tolist() == [k - k % 2 for k in range(n)]
    owner, rounds = check_clump(ctx, lb, np.arange(n)[::-1], np.ones(n))
    assert rounds == n and owner.tolist() == [k + 1 - k % 2 for k in range(n)]
    rng = np.random.default_rng(5)
    for _ in range(3):
        owner, rounds = check_clump(ctx, lb, rng.permutation(n), rng.random(n) < 0.8)
        assert 2 <= rounds < n


@pytest.mark.parametrize("window", CC.CLUMP_WINDOWS)
def test_ld_clump_star(ctx, window):
    """a centre with leaves at distances 1, 64, 65, 1023, 1024, window - 1 and window on both sides (those within the window):
    guards an upper word, the forward / backward transposition and d < window off by one; and a bit that points before
    variant 0"""
    c, n = 1050, 2100
    dists = sorted(D for D in {1, 64, 65, 1023, 1024, window - 1, window} if 1 <= D <= window)
    lb = np.zeros((n, window), bool)
    for D in dists:
        lb[c, D - 1] = lb[c + D, D - 1] = True
    lb[5, min(100, window - 1)] = True                                   # points before variant 0: ignored
    leaves = [c - D for D in dists] + [c + D for D in dists]
    rng = np.random.default_rng(window)
    rank = rng.permutation(n)
    low, high = np.argmin(rank), np.argmax(rank)
    for centre_rank, eligible_centre in ((rank[low], 1), (rank[high], 1), (rank[low], 0)):
        r = rank.copy()
        r[low if centre_rank == rank[low] else high], r[c] = r[c], centre_rank
        elig = np.ones(n, np.uint8)
        elig[c] = eligible_centre
        owner, rounds = check_clump(ctx, lb, r, elig)
        if eligible_centre and centre_rank == rank[low]:
            assert owner[c] == c and all(owner[x] == c for x in leaves) and rounds == 2
        else:
            first = min(leaves, key=lambda x: r[x])
            assert owner[c] == first and all(owner[x] == x for x in leaves)
        assert all(owner[x] == x for x in range(n) if x != c and x not in leaves)


def test_ld_clump_small_and_degenerate(ctx):
    both = np.array([[False], [True]])
    owner, rounds = clump(ctx, both, [0, 0], [1, 1])                    # equal ranks block neither way: no wait
    assert owner.tolist() == [0, 1] and rounds == 1
    owner, rounds = clump(ctx, both, [7, 7], [1, 0])                    # the owner of the other one all the same
    assert owner.tolist() == [0, 0] and rounds == 1
    lb = np_linked_back(np_ld_table(ld_genotypes(1, 40, 200), 7), 0.2)
    owner, rounds = clump(ctx, lb, np.arange(200), np.zeros(200))
    assert (owner == -1).all() and rounds == 0
    owner, rounds = clump(ctx, lb, np.zeros(200, np.int64), np.ones(200))      # all ranks equal: every variant an index
    assert owner.tolist() == list(range(200)) and rounds == 1
    for window in (1, 64, 1024):
        owner, rounds = clump(ctx, np.zeros((0, window), bool), [], [])
        assert owner.shape == (0,) and rounds == 0
        owner, rounds = clump(ctx, np.ones((1, window), bool), [0], [1])
        assert owner.tolist() == [0] and rounds == 1
        owner, rounds = clump(ctx, np.ones((1, window), bool), [0], [0])
        assert owner.tolist() == [-1] and rounds == 0


# ---- hhgt_ld_clump at every lane-group width: one word at a time, the owners' minimum, batch and workgroup boundaries ----------

def run_case(ctx, case, guarded=False):
    """a case of tests/clump_cases.py on the device, against the owners and rounds it was built for"""
    words = CC.link_words(case["k"], case["d"], case["n"], case["window"])
    owner, rounds = clump_words(ctx, words, case["window"], case["rank"], case["eligible"], guarded)
    bad = np.flatnonzero(owner != case["owner"])
    assert not len(bad) and rounds == case["rounds"], (case["window"], case["n"], bad[:10], owner[bad[:10]], rounds)


def check_case(ctx, case, guarded=False):
    """the same through check_clump: against clump_reference and the numpy rounds, and then against the case's own owners"""
    lb = CC.link_matrix(case["k"], case["d"], case["n"], case["window"])
    owner, rounds = check_clump(ctx, lb, case["rank"], case["eligible"], guarded)
    assert np.array_equal(owner, case["owner"]) and rounds == case["rounds"], (case["window"], case["n"])


@pytest.mark.parametrize("window", CC.CLUMP_WINDOWS)
def test_ld_clump_strided_paths(ctx, window):
    """chains of stride D, 9 D + 1 variants: all links in word (D - 1) // 64, for every word of the window at its first and
    its last usable bit.  Identity ranking: every blocker in a back word; reversed: in a forward word; both wait through
    that word for ten rounds.  Opposite: neighbouring lane groups of a wave give opposite verdicts in every round.  Guards a
    word that is not walked (a lane group too narrow for the window, idle lanes cut at the wrong place), a group mask that
    takes in the neighbour, the state handed over across the batch of eight rounds"""
    for _, D in CC.strided_distances(window):
        for ranking in CC.RANKINGS:
            run_case(ctx, CC.strided(window, D, ranking))


@pytest.mark.parametrize("ranking", CC.RANKINGS)
@pytest.mark.parametrize("window", CC.CLUMP_WINDOWS)
def test_ld_clump_strided_paths_against_the_reference(ctx, window, ranking):
    """the first and the last word of every window once more, against clump_reference and np_rounds themselves"""
    nq = CC.n_words(window)
    for q, D in CC.strided_distances(window):
        if q in (0, nq - 1):
            check_case(ctx, CC.strided(window, D, ranking))


@pytest.mark.parametrize("window", CC.CLUMP_WINDOWS)
def test_ld_clump_owner_is_the_minimum_over_the_words(ctx, window):
    """k_clump_owners' shuffle reduction over LPV lanes: per word j of the 2 nq a variant that is not eligible, with one
    linked index in word j and one in word j + 1 or j - 1 — the lower rank owns it, the earlier variant at equal ranks —,
    two such variants side by side that go different ways"""
    for turn in range(3):
        case = CC.gadgets(window, turn)
        run_case(ctx, case)
        if window <= 129:
            check_case(ctx, case)


@pytest.mark.parametrize("window", CC.CLUMP_WINDOWS)
def test_ld_clump_edges_of_the_last_word(ctx, window):
    """a link at exactly distance `window` counts, either way round; a bit at or past `window` in the last word of a window
    that is no multiple of 64 counts for nothing — csrc/clump.hip masks d < window on both sides when it gathers the
    blockers and the forward links, and again when the owners walk the back words — whether it sits on an eligible variant,
    on one that is not, or beside a real link (include/hhgt.h: hhgt_ld_decisions leaves such bits 0)"""
    cases = CC.edge_cases(window)
    assert len(cases) == (3 if window % 64 else 2)
    for case in cases:
        run_case(ctx, case)


@pytest.mark.parametrize("window", [1, 129])
def test_ld_clump_rounds_at_the_batch_boundary(ctx, window):
    """paths of n variants take n rounds: one below, at and one past the host's batches of eight launches, one and two
    variants; the owners alternate; a second call, on the workspace of the first, gives the same"""
    for n in (1, 2, 7, 8, 9, 15, 16, 17, 24, 25):
        for ranking in ("identity", "reversed"):
            case = CC.strided(window, 1, ranking, n=n)
            assert case["rounds"] == n
            if ranking == "identity":
                assert case["owner"].tolist() == [k - k % 2 for k in range(n)]
            else:
                assert case["owner"].tolist() == [k + (n - 1 - k) % 2 for k in range(n)]
            for _ in range(2):
                check_case(ctx, case)


@pytest.mark.parametrize("window", [64, 128, 192, 448, 960])
def test_ld_clump_variants_at_the_workgroup_boundary(ctx, window):
    """a workgroup holds 256 / LPV variants: one less, exactly that, one more, and two workgroups and one — the owners
    between sentinels, nothing written outside them"""
    per = 256 // CC.CLUMP_SHAPES[window][1]
    assert per == {64: 128, 128: 64, 192: 32, 448: 16, 960: 8}[window]
    for n in (per - 1, per, per + 1, 2 * per + 1):
        for D in sorted({1, 2, min(max(n // 3, 1), window)}):
            for ranking in CC.RANKINGS:
                case = CC.strided(window, D, ranking, n=n)
                assert len(case["k"]) == n - D > 0
                check_case(ctx, case, guarded=True)


# ---- both kernels on real tables ---------------------------------------------------------------------------------------------

def device_clump(ctx, table, window, r2, p, p1, pos=None, max_dist=None):
    n = len(table)
    pos_t = None if pos is None else torch.from_numpy(padded_pos(pos, window, 0, n)).to(ctx.device)
    bits = ctx.ld_decisions(to_dev(ctx, padded(table, window, 0, n)), r2, pos_t, max_dist)
    pt = torch.from_numpy(p).to(ctx.device)
    owner, rounds = ctx.ld_clump(bits, window, SS.clump_rank(pt).to(torch.int32), (pt <= p1).to(torch.uint8))
    return owner.cpu().numpy().astype(np.int64), rounds


@pytest.mark.parametrize("window", [7, 50, 65])
def test_ld_clump_on_the_recipe(ctx, recipe, window):
    table = recipe[window]
    p = random_p(SEED, V)
    for r2 in (0.2, 0.5):
        lb = np_linked_back(table, r2)
        for p1 in (1.0, 0.3):
            want = SS.clump_reference(lb, p, p1)
            got, rounds = device_clump(ctx, table, window, r2, p, p1)
            assert np.array_equal(got, want), (window, r2, p1, np.flatnonzero(got != want)[:10])
            assert rounds == np_rounds(lb, SS.clump_rank(p), p <= p1)[1] >= 3
        # ascending p, every variant eligible: the index variants are the variants hhgt_ld_prune keeps on the same table
        keep = ctx.ld_prune(to_dev(ctx, padded(table, window, 0, V)), r2).cpu().numpy()[window:].astype(bool)
        got, _ = device_clump(ctx, table, window, r2, np.linspace(1e-9, 1.0, V), 1.0)
        assert np.array_equal(got == np.arange(V), keep) and np.array_equal(keep, np_prune(table, r2)) and 0 < keep.sum() < V
    # positions 3 bp apart, 60 bp: the owners of window 20 without a limit
    if window == 50:
        pos = np.arange(V, dtype=np.int64) * 3 + 10
        got, _ = device_clump(ctx, table, 50, 0.2, p, 0.3, pos, 60)
        narrow, _ = device_clump(ctx, table[:, :20], 20, 0.2, p, 0.3)
        assert np.array_equal(got, narrow) and np.array_equal(got, SS.clump_reference(np_linked_back(table[:, :20], 0.2), p, 0.3))


@pytest.mark.parametrize("window", FAR_WINDOWS)
def test_ld_clump_on_the_far_recipe(ctx, far, window):
    """n = 3000 at windows of two to sixteen words a side (LPV 4 to 32; 300 and 513 with idle lanes); the only links are the
    planted copies, up to `window` places apart"""
    table = far["table"][:, :window]
    lb = far_links(far, window, 0.5)
    p = random_p(SEED, FAR_V)
    for p1 in (1.0, 0.3):
        want = SS.clump_reference(lb, p, p1)
        got, rounds = device_clump(ctx, table, window, 0.5, p, p1)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert rounds == np_rounds(lb, SS.clump_rank(p), p <= p1)[1] >= 2
        claimed = np.flatnonzero((want >= 0) & (want != np.arange(FAR_V)))
        farthest = np.abs(want[claimed] - claimed).max()
        if window == 1024:
            assert len(claimed) >= 10 and farthest >= 1000
        if p1 == 1.0:                                                    # the copy at distance `window`: its top word decides
            assert len(claimed) >= 10 and farthest == window
        assert len(claimed) >= 5
    keep = ctx.ld_prune(to_dev(ctx, padded(table, window, 0, FAR_V)), 0.5).cpu().numpy()[window:].astype(bool)
    got, _ = device_clump(ctx, table, window, 0.5, np.linspace(1e-9, 1.0, FAR_V), 1.0)
    assert np.array_equal(got == np.arange(FAR_V), keep) and not keep.all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def test_clump_kernels_refuse(ctx):
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=ctx.device)                                  # noqa: E731
    table = z((10, 4, 8), torch.int32)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(HhgtError, match="ld_decisions"):
            ctx.ld_decisions(table, bad)
    with pytest.raises(HhgtError, match="ld_decisions"):
        ctx.ld_decisions(z((1030, 1025, 8), torch.int32), 0.2)
    for bad in (z((4, 0, 8), torch.int32), z((3, 4, 8), torch.int32), z((10, 4, 7), torch.int32), z((10, 4, 8), torch.int64)):
        with pytest.raises(ValueError):
            ctx.ld_decisions(bad, 0.2)
    pos = z(10, torch.int64)
    for kw in (dict(pos=pos), dict(max_dist=5), dict(pos=pos[:9], max_dist=5), dict(pos=pos.to(torch.int32), max_dist=5),
               dict(pos=pos, max_dist=-1), dict(bits=z((6, 2), torch.int64)), dict(bits=z((6, 1), torch.int32))):
        with pytest.raises(ValueError):
            ctx.ld_decisions(table, 0.2, **kw)
    assert ctx.ld_decisions(table, 0.2, pos, 5).cpu().numpy().tolist() == [[0]] * 6
    bits, rank, elig = z((6, 1), torch.int64), z(6, torch.int32), z(6, torch.uint8)
    for window in (0, 1025):
        with pytest.raises(HhgtError, match="ld_clump"):
            ctx.ld_clump(z((6, 1 if window == 0 else 16), torch.int64), window, rank, elig)
    for args in ((z((6, 2), torch.int64), 64, rank, elig), (bits, 64, rank[:5], elig), (bits, 64, rank, elig[:5]),
                 (bits, 64, rank.to(torch.int64), elig), (bits.to(torch.int32), 64, rank, elig), (bits, 65, rank, elig)):
        with pytest.raises(ValueError):
            ctx.ld_clump(*args)
    with pytest.raises(ValueError):
        ctx.ld_clump(bits, 64, rank, elig, owner=z(5, torch.int32))
    # null arguments, named: straight at the library
    lib, h, p = ctx.lib, ctx.h, bits.data_ptr()
    for args, what in (((None, 6, 64, p, p, p, None, None), "link bits"), ((p, 6, 64, None, p, p, None, None), "ranks"),
                       ((p, 6, 64, p, None, p, None, None), "eligible"), ((p, 6, 64, p, p, None, None, None), "owners")):
        assert lib.hhgt_ld_clump(h, *args) != 0 and "ld_clump" in lib.hhgt_last_error().decode() and what in lib.hhgt_last_error().decode()
    for args, what in (((None, 6, 4, 0.2, None, 0, p, None), "table"), ((table.data_ptr(), 6, 4, 0.2, None, 0, None, None), "link bits")):
        assert lib.hhgt_ld_decisions(h, *args) != 0 and "ld_decisions" in lib.hhgt_last_error().decode() and what in lib.hhgt_last_error().decode()
    owner, rounds = ctx.ld_clump(bits, 64, rank, elig.to(torch.bool))
    assert owner.cpu().numpy().tolist() == [-1] * 6 and rounds == 0


# ---- the store ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stores(ctx, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("clump")
    out = []
    for sc, vc, n_v in GEOMS:
        g = ld_genotypes(vc, 130, n_v)
        d = str(tmp / f"c{vc}.hhgt")
        write_store(ctx, d, g, sc, vc)
        out.append(dict(g=g, sc=sc, vc=vc, V=n_v, paths=[d, export_h5(d, str(tmp / f"c{vc}.h5"))]))
    return dict(geoms=out, tmp=tmp)


_EXPECTED = {}


def store_p(n, nan_every=17):
    p = random_p(SEED, n)
    p[::nan_every] = np.nan
    return p


def expected_owner(g, ii, a, b, mask, p, window, r2, p1, p2, max_dist):
    """clump_reference on np_ld_table of the same selection -> int64 [b - a], offsets into the range"""
    with np.errstate(invalid="ignore"):
        take = (np.ones(b - a, bool) if mask is None else mask) & (p <= p2)
    key = (id(g), tuple(ii), a, b, take.tobytes(), p.tobytes(), window, r2, p1, max_dist)
    if key not in _EXPECTED:
        table = np_ld_table(g[:, a:b], window, samples=ii, variants=take)
        at = np.flatnonzero(take)
        pos = (np.arange(a, b, dtype=np.int64) * 3 + 10)[at]
        own = SS.clump_reference(np_linked_back(table, r2, None if max_dist is None else pos, max_dist), p[at], p1)
        full = np.full(b - a, -1, np.int64)
        full[at] = np.where(own >= 0, at[np.maximum(own, 0)], -1)
        _EXPECTED[key] = full
    return _EXPECTED[key]


def check_store(st, g, samples, a, b, p, p_arg=None, mask=None, mask_arg=None, window=50, r2=0.2, p1=0.3, p2=0.8, kb=None, **kw):
    ii = np.arange(g.shape[0]) if samples is None else np.array([st._sample_index(x) for x in samples], np.int64)
    want = expected_owner(g, ii, a, b, mask, p, window, r2, p1, p2, None if kb is None else int(kb * 1000))
    got = st.ld_clump(GROUP, p if p_arg is None else p_arg, samples, a, b, variant_mask=mask_arg, p1=p1, p2=p2, r2=r2,
                      window=window, kb=kb, **kw)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (b - a,)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (a, b, window, kw, np.flatnonzero(got != want)[:10])
    return want


@pytest.mark.parametrize("geom", range(len(GEOMS)))
def test_store_ld_clump(ctx, stores, geom):
    c = stores["geoms"][geom]
    g, n_v, vc = c["g"], c["V"], c["vc"]
    cut = (vc // 2 + 5, n_v - 7) if vc < 8192 else (4000, 8300)              # inside blocks at both ends
    p, pc = store_p(n_v), store_p(cut[1] - cut[0], 13)
    maf = np_variant_mask(g[np.unique(PICK), cut[0]:cut[1]], min_maf=0.1)
    for path in c["paths"]:
        st = GenotypeStore(path, ctx=ctx)
        st.stats.update(ld_pairs=0, clump_rounds=0, clump_window_short=0)
        whole = check_store(st, g, None, 0, n_v, p)
        roles = SS.clump_summary(whole, p)                                  # NaN and p > p2 count as none here
        assert min(roles["n_index"], roles["n_clumped_total"]) >= 0.1 * n_v and (whole[::17] == -1).all()
        n = int((p <= 0.8).sum())
        assert st.stats["ld_pairs"] == GenotypeStore._ld_pairs(n, 50) and st.stats["clump_rounds"] >= 2
        assert st.stats["clump_window_short"] == 0                          # (no distance limit)
        check_store(st, g, PICK, 0, n_v, p, p_arg=torch.from_numpy(p).to(ctx.device))          # p as a device tensor
        check_store(st, g, SPARSE, 0, n_v, p, p1=1.0, p2=1.0)
        check_store(st, g, [f"d{i:03d}" for i in SPARSE], *cut, pc, window=7, r2=0.5, plane_bytes=1)
        check_store(st, g, PICK, *cut, pc, mask=maf, mask_arg=st.variant_mask(GROUP, PICK, *cut, min_maf=0.1), window=7)
        check_store(st, g, PICK, *cut, pc, mask=maf, mask_arg=maf, window=7)                     # the mask as a host array
        assert 50 < maf.sum() < len(maf)
        check_store(st, g, None, 11, 11, np.zeros(0))                                          # an empty range
        check_store(st, g, [], 0, 40, p[:40])                                                  # no sample: nothing is linked
        check_store(st, g, None, 0, 40, np.full(40, np.nan))                                   # nothing counted
        # seams in every block, small slabs, tiles shorter than the window
        for kw in (dict(plane_bytes=1), dict(slab_bytes=3000), dict(plane_bytes=1, slab_bytes=3000)):
            check_store(st, g, None, 0, n_v, p, **kw)
            check_store(st, g, PICK, *cut, pc, window=65, r2=0.5, **kw)
        if vc == 128:                                                       # a window of more than two chunks of variants
            check_store(st, g, PICK, 0, n_v, p, window=300, plane_bytes=1)
            check_store(st, g, None, *cut, pc, window=300)
        # 3 bp apart, every variant counted: 60 bp are 20 places — the owners of window 20 without a limit; and the
        # variants at which the window, not the distance, ends the search
        pf = random_p(SEED + 1, n_v)
        st.stats["clump_window_short"] = 0
        limited = check_store(st, g, PICK, 0, n_v, pf, p2=1.0, kb=0.06)
        assert st.stats["clump_window_short"] == 0
        assert np.array_equal(limited, check_store(st, g, PICK, 0, n_v, pf, p2=1.0, window=20))
        check_store(st, g, PICK, 0, n_v, pf, p2=1.0, window=20, kb=0.06)
        assert st.stats["clump_window_short"] == n_v - 20
        check_store(st, g, PICK, 0, n_v, p, kb=0.06)                        # with gaps among the counted: by position
        # ascending p, every variant eligible, no limit: the index variants are ld_prune's
        asc = np.linspace(1e-9, 1.0, n_v)
        own = st.ld_clump(GROUP, asc, PICK, p1=1.0, p2=1.0, r2=0.2, window=50, kb=None)
        keep = st.ld_prune(GROUP, PICK, window=50, r2=0.2)
        assert torch.equal(own == torch.arange(n_v, device=own.device), keep) and 0 < int(keep.sum()) < n_v
        # the errors
        for bad in (dict(window=0), dict(window=1025), dict(r2=1.5), dict(p1=0.5, p2=0.1), dict(p1=-0.1), dict(p2=1.5),
                    dict(kb=-1.0), dict(variant_mask=maf[:10])):
            with pytest.raises(ValueError):
                st.ld_clump(GROUP, p, **bad)
        planted = lambda x: np.concatenate([p[:1], [x], p[2:]])                                            # noqa: E731
        for bad_p in (p[:10], torch.from_numpy(p.astype(np.float32)), planted(1.5), planted(-0.5), planted(np.inf), planted(-np.inf)):
            with pytest.raises(ValueError):
                st.ld_clump(GROUP, bad_p)
        with pytest.raises(KeyError):
            st.ld_clump("chr_6", p)
        with pytest.raises(IndexError):
            st.ld_clump(GROUP, p, v_lo=5, v_hi=n_v + 1)
        st.close()


def test_store_ld_clump_leaves_read_cache_alone(ctx, stores):
    c = stores["geoms"][0]
    p = store_p(c["V"])
    for path in c["paths"]:
        st = GenotypeStore(path, ctx=ctx)
        batch = [(GROUP, s, 100 * s % 1000, 100 * s % 1000 + 300) for s in (3, 70, 129)]
        first = [r.cpu().numpy() for r in st.read_windows(batch)]
        keys, used, n = list(st._cache), st._cache_used, st.stats["chunks_read"]
        a = st.ld_clump(GROUP, p, PICK, p1=0.3, p2=0.8).cpu().numpy()
        assert list(st._cache) == keys and st._cache_used == used
        again = [r.cpu().numpy() for r in st.read_windows(batch)]
        assert st.stats["chunks_read"] == n and all(np.array_equal(x, y) for x, y in zip(first, again))
        assert np.array_equal(st.ld_clump(GROUP, p, PICK, p1=0.3, p2=0.8, slab_bytes=3000).cpu().numpy(), a) and (a >= 0).any()
        st.close()


def test_store_ld_clump_far_windows(ctx, far, tmp_path):
    """the long-range cohort in a store of 128-variant chunks at windows of 3, 5 and 9 words (LPV 8, 16, 32, all with idle
    lanes): with the default budgets and with tiles shorter than the window, the bits then written by several
    hhgt_ld_decisions calls; a claimed variant lies in the top word of its owner"""
    d = str(tmp_path / "far.hhgt")
    write_store(ctx, d, far["g"], 64, 128)
    p = random_p(SEED, FAR_V)
    st = GenotypeStore(d, ctx=ctx)
    for window in (129, 300, 513):
        want = SS.clump_reference(far_links(far, window, 0.5), p, 1.0)
        claimed = np.flatnonzero((want >= 0) & (want != np.arange(FAR_V)))
        assert (np.abs(want[claimed] - claimed) > 64 * (CC.n_words(window) - 1)).any()
        for kw in (dict(), dict(plane_bytes=1, slab_bytes=3000)):
            st.stats["clump_rounds"] = 0
            got = st.ld_clump(GROUP, p, p1=1.0, p2=1.0, r2=0.5, window=window, kb=None, **kw).cpu().numpy()
            assert np.array_equal(got, want), (window, kw, np.flatnonzero(got != want)[:10])
            assert st.stats["clump_rounds"] == np_rounds(far_links(far, window, 0.5), SS.clump_rank(p), np.ones(FAR_V, bool))[1]
    st.close()


# ---- reader and CLI ----------------------------------------------------------------------------------------------------------

def test_reader_clump_and_cli(ctx, stores):
    from click.testing import CliRunner
    from haplohyped_varawareml_amd import score
    from haplohyped_varawareml_amd.assoc import HEADER as ASSOC_HEADER
    from haplohyped_varawareml_amd.clump import HEADER, main, read_assoc
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    c, tmp = stores["geoms"][0], stores["tmp"]
    g, n_v = c["g"], c["V"]
    rng = np.random.default_rng(9)
    p = store_p(n_v)
    beta = rng.normal(size=n_v)
    fmt = lambda x: "nan" if np.isnan(x) else "%.17g" % x                                                   # noqa: E731
    line = lambda v, name, pv: f"chr7\t{3 * v + 11}\tA\tG\t{name}\t130\t0.25\t{fmt(beta[v])}\t0.1\t1\t{fmt(pv)}"    # noqa: E731
    listed = [line(v, "y", p[v]) for v in range(n_v)]
    listed.insert(40, "chr7\t5\tA\tG\ty\t130\t0.25\t0.5\t0.1\t1\t1e-09")        # the cohort has no variant there
    listed.insert(90, "chr8\t11\tA\tG\ty\t130\t0.25\t0.5\t0.1\t1\t1e-09")       # nor that chromosome
    (tmp / "assoc.tsv").write_text(ASSOC_HEADER + "\n".join(listed) + "\n")
    both = [x for v in range(n_v) for x in (line(v, "y", p[v]), line(v, "z", 0.5))]
    (tmp / "assoc2.tsv").write_text(ASSOC_HEADER + "\n".join(both) + "\n")
    donors = [f"d{i:03d}" for i in PICK]
    (tmp / "clump_samples.txt").write_text("\n".join(donors) + "\n")
    cases = [(dict(p1=0.3, p2=0.8, r2=0.2, window=50), ["--p1", "0.3", "--p2", "0.8", "--r2", "0.2", "--window", "50"], None),
             (dict(p1=0.3, p2=0.8, r2=0.2, window=5, kb=0.03, donor_ids=donors),
              ["--p1", "0.3", "--p2", "0.8", "--r2", "0.2", "--window", "5", "--kb", "0.03", "--sample_list",
               str(tmp / "clump_samples.txt"), "--chromosome", "7"], np.unique(PICK))]
    out, index_out = tmp / "clumps.tsv", tmp / "index.tsv"
    for kw, args, ii in cases:
        kb = kw.get("kb", 250.0)
        own = expected_owner(g, np.arange(130) if ii is None else ii, 0, n_v, None, p, kw["window"], 0.2, 0.3, 0.8, int(kb * 1000))
        at = np.flatnonzero(p <= 0.8)
        row = np.full(n_v, -1)
        row[at] = np.arange(len(at))
        n_clumped = np.bincount(own[(own >= 0) & (own != np.arange(n_v))], minlength=n_v)
        w = kw["window"]                    # where the window-th counted follower is still within the distance
        short = int((3 * (at[w:] - at[:-w]) <= int(kb * 1000)).sum())
        # the reader
        r = VCFH5Reader(c["paths"][1], ctx=ctx)
        variants, pv, lines, _ = read_assoc(str(tmp / "assoc.tsv"))
        rec, info = r.clump(variants, pv, **kw)
        assert info == dict(matched=n_v - int(np.isnan(p).sum()), unmatched=2, window_short=short)
        assert len(rec) == len(at) and np.array_equal(rec["start"], 3 * at + 10) and set(rec["chrom"]) == {b"chr7"}
        assert np.array_equal(rec["p"], p[at]) and set(rec["ref"]) == {b"A"} and set(rec["alt"]) == {b"G"}
        assert np.array_equal(rec["index"], np.where(own[at] >= 0, row[np.maximum(own[at], 0)], -1))
        assert np.array_equal(rec["role"], np.where(own[at] == at, 1, np.where(own[at] >= 0, 2, 0)))
        assert np.array_equal(rec["n_clumped"], n_clumped[at]) and [lines[i] for i in rec["listed"]] == [line(v, "y", p[v]) for v in at]
        with pytest.raises(ValueError, match="listed twice"):
            r.clump(np.concatenate([variants, variants[:1]]), np.concatenate([pv, pv[:1]]))
        with pytest.raises(ValueError):
            r.clump(variants, pv[:-1])
        r.close()
        # the command: literal text from the reference
        text = HEADER
        for v in at:
            o = own[v]
            role = "index" if o == v else "clumped" if o >= 0 else "none"
            where = f"{3 * o + 11}\tA\tG" if o >= 0 else ".\t.\t."
            text += f"chr7\t{3 * v + 11}\tA\tG\t{'%.17g' % p[v]}\t{role}\t{where}\t{n_clumped[v] if o == v else '.'}\n"
        res = CliRunner().invoke(main, ["--h5", c["paths"][1], "--assoc", str(tmp / "assoc.tsv"), "--out", str(out),
                                        "--index_out", str(index_out)] + args)
        assert res.exit_code == 0, res.output
        assert out.read_text() == text, args
        index = np.flatnonzero(own == np.arange(n_v))
        assert 0.1 * n_v <= len(index) <= 0.5 * n_v
        assert index_out.read_text() == ASSOC_HEADER + "".join(line(v, "y", p[v]) + "\n" for v in index)
        # INDEX.tsv is a valid --weights of score: exactly the index variants, their BETA
        wv, names, w = score.read_weights(str(index_out), columns=["BETA"])
        assert names == ["BETA"] and wv["pos"].tolist() == (3 * index + 11).tolist() and np.array_equal(w[:, 0], beta[index])
        assert ("warning" in res.output) == (short > 0)
    # several phenotypes: --pheno is needed, and picks
    base = ["--h5", c["paths"][1], "--out", str(out), "--p1", "0.3", "--p2", "0.8", "--r2", "0.2", "--window", "50"]
    res = CliRunner().invoke(main, base + ["--assoc", str(tmp / "assoc2.tsv")])
    assert res.exit_code == 2 and "--pheno" in res.output
    first = CliRunner().invoke(main, base + ["--assoc", str(tmp / "assoc.tsv")])
    assert first.exit_code == 0
    want = out.read_text()
    res = CliRunner().invoke(main, base + ["--assoc", str(tmp / "assoc2.tsv"), "--pheno", "y"])
    assert res.exit_code == 0 and out.read_text() == want
    res = CliRunner().invoke(main, base + ["--assoc", str(tmp / "assoc2.tsv"), "--pheno", "z"])
    assert res.exit_code == 0 and out.read_text().count("\tnone\t") == n_v         # p = 0.5 > p1 everywhere: no index
    assert CliRunner().invoke(main, base + ["--assoc", str(tmp / "assoc.tsv"), "--sample_list", str(tmp / "assoc.tsv")]).exit_code == 2
