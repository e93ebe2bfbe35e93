"""CPU: the host side of LD between nearby variants (store.plane_positions, ld_sums, r2_from_counts, ld_exceeds) against a
brute-force numpy restatement from int8 [S, V, 2] genotypes — boolean class matrices for the table, np.corrcoef over the
jointly complete samples for r^2 —, and the pure-numpy greedy walk np_prune that the GPU tests compare masks with.  Also
home of the correlated genotype recipe those tests use (the synthetic generator's variants are independent: nothing to
prune)."""
import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd import store as S_


# ---- the recipe and the restatement (imported by tests/test_gpu_ld.py) -----------------------------------------------------

def ld_genotypes(seed, n_samples, n_variants):
    """int8 [S, V, 2] with linkage: every 8th variant, and any other with probability 0.3, is drawn fresh with an allele
    frequency in U(0.05, 0.5); otherwise a variant copies its predecessor with each allele flipped at 3 %.  Then 1 % of the
    alleles are set to -9 and 0.4 % to 2, two variants are made exact duplicates of earlier ones (three places and one place
    on) and one all-reference."""
    rng = np.random.default_rng(seed)
    g = np.zeros((n_samples, n_variants, 2), np.int8)
    for v in range(n_variants):
        if v % 8 == 0 or rng.random() < 0.3:
            g[:, v] = rng.random((n_samples, 2)) < rng.uniform(0.05, 0.5)
        else:
            g[:, v] = g[:, v - 1] ^ (rng.random((n_samples, 2)) < 0.03)
    g[rng.random(g.shape) < 0.01] = -9
    g[rng.random(g.shape) < 0.004] = 2
    if n_variants >= 8:
        g[:, n_variants // 2 + 3] = g[:, n_variants // 2]       # a duplicate three places on
        g[:, 2 * n_variants // 3 + 1] = g[:, 2 * n_variants // 3]       # and one right behind its original: any window sees it
        g[:, n_variants // 3] = 0                               # all reference: monomorphic
    return g


def np_classes(g):
    """int8 [S, V, 2] -> (M, H, A) bool [S, V]: complete, HET, HOM_ALT"""
    a, b = g[..., 0], g[..., 1]
    m = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
    return m, m & (a != b), m & (a == 1) & (b == 1)


def np_ld_table(g, window, samples=None, variants=None):
    """the LD table of genotypes int8 [S, V, 2] over `samples` (indices, each once) and the counted `variants` (indices or
    bool mask; None: all) -> int64 [n, window, 8]"""
    if samples is not None:
        g = g[np.unique(np.asarray(samples, np.int64))]
    if variants is not None:
        g = g[:, variants]
    m, h, a = np_classes(g)
    n = g.shape[1]
    t = np.zeros((n, window, 8), np.int64)
    for d in range(window):
        u = np.arange(max(n - 1 - d, 0))
        v = u + 1 + d
        cols = [m[:, u] & m[:, v], h[:, u] & m[:, v], a[:, u] & m[:, v], m[:, u] & h[:, v], m[:, u] & a[:, v],
                h[:, u] & h[:, v], (h[:, u] & a[:, v]) | (a[:, u] & h[:, v]), a[:, u] & a[:, v]]
        for c, x in enumerate(cols):
            t[u, d, c] = x.sum(0)
    return t


def np_products(table):
    """-> (num * num, dx * dy), float64: the contract's three products but for the threshold's"""
    t = np.asarray(table).astype(np.int64)
    n, hm, am, mh, ma, hh, ha, aa = (t[..., c] for c in range(8))
    sx, sxx, sy, syy, sxy = hm + 2 * am, hm + 4 * am, mh + 2 * ma, mh + 4 * ma, hh + 2 * ha + 4 * aa
    num, dx, dy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    num, dx, dy = num.astype(np.float64), dx.astype(np.float64), dy.astype(np.float64)
    return num * num, dx * dy


def np_r2(table):
    nn, den = np_products(table)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0, nn / den, np.nan)


def np_exceeds(table, r2):
    nn, den = np_products(table)
    return nn > np.float64(r2) * den


def np_prune(table, r2, n=None):
    """the greedy walk over an LD table [n, W, 8]: variant v is kept iff no kept u among the W before it exceeds -> bool [n]"""
    table = np.asarray(table)
    n = table.shape[0] if n is None else n
    window = table.shape[1]
    ex = np_exceeds(table, r2)
    keep = np.zeros(n, bool)
    for v in range(n):
        u = np.arange(max(v - window, 0), v)
        keep[v] = not (keep[u] & ex[u, v - u - 1]).any()
    return keep


def check_r2(got, want):
    """r^2 against the restatement: NaN in the same places, the rest within rtol 1e-12 (two products and one division in the
    same order differ by rounding at most)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=0)


# ---- the long-range recipe (wide windows: the keep flags of up to 1024 variants back decide) ---------------------------------

FAR_WINDOWS = (128, 129, 256, 300, 512, 513, 1024)
# distances of the planted duplicates: around every boundary of the walk's 64-bit register words that a power-of-two
# register has, five places into each of the 16 words, and w, w + 1 of every window tested (the last in reach, the first out)
FAR_DISTANCES = tuple(sorted({1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025}
                             | {64 * q + 5 for q in range(16)} | {w + e for w in FAR_WINDOWS for e in (0, 1)}))
FAR_S, FAR_V, FAR_SEED = 130, 3000, 7


def walk_words(window):
    """the 64-bit words of the walk's register (ld_walk_words of csrc/ld.hip restated): a power of two, 64 nq >= window"""
    nq = 1
    while nq * 64 < window:
        nq *= 2
    return nq


def chain_distances(window):
    """(D1, D2) of the chain planted for `window`: 700 and 600 at 1024, in proportion below — each within the window and
    in its upper half, together beyond it"""
    return 700 * window // 1024, 600 * window // 1024


def far_layout(n_variants, window):
    """where far_genotypes plants -> dict(dups=[(D, original, copy)], chains={w: (u0, u, v)}): every copy lies after
    position `window`, and no two planted positions (originals included) are less than three places apart, so the only
    identical variants are a duplicate and its original, and the three of a chain"""
    used = []

    def place(p, back):
        while True:
            spots = [p - b for b in back]
            if min(spots) >= 0 and all(abs(x - y) >= 3 for x in spots for y in used):
                used.extend(spots)
                return spots
            p += 1

    dups, chains, p = [], {}, window + 6
    for D in FAR_DISTANCES:
        copy, orig = place(max(p, D), (0, D))
        dups.append((D, orig, copy))
        p = copy + 5
    for w in sorted({x for x in FAR_WINDOWS if x <= window} | {window}):
        d1, d2 = chain_distances(w)
        v, u, u0 = place(max(p, d1 + d2), (0, d1, d1 + d2))
        chains[w] = (u0, u, v)
        p = v + 5
    assert p <= n_variants, (p, n_variants)
    return dict(dups=dups, chains=chains)


def far_genotypes(seed, n_samples, n_variants, window):
    """int8 [S, V, 2] with long-range structure and nothing else.  Base variants are independent, each with its own allele
    frequency in U(0.1, 0.5), 1 % of the alleles -9.  At far_layout's places a variant is an exact copy (missing calls
    included) of the one D places before it, for every D of FAR_DISTANCES; and per window w of FAR_WINDOWS up to `window`
    (and `window` itself) there is one chain u0 -> u -> v: u copies u0 from D2 places back, v copies u from D1 places back,
    (D1, D2) = chain_distances(w): at window w, u is pruned by u0, and v stays because u0 is out of reach and u not kept."""
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.1, 0.5, n_variants)
    g = (rng.random((n_samples, n_variants, 2)) < af[None, :, None]).astype(np.int8)
    g[rng.random(g.shape) < 0.01] = -9
    lay = far_layout(n_variants, window)
    for _, orig, copy in lay["dups"]:
        g[:, copy] = g[:, orig]
    for u0, u, v in lay["chains"].values():
        g[:, u] = g[:, u0]
        g[:, v] = g[:, u]
    return g


_FAR = {}


def far_cohort():
    """the long-range cohort and its LD table at window 1024, int32 and read-only, computed once per process (the table of
    a window w is its first w columns) -> dict(g, table, dups, chains)"""
    if not _FAR:
        g = far_genotypes(FAR_SEED, FAR_S, FAR_V, 1024)
        table = np_ld_table(g, 1024).astype(np.int32)
        table.setflags(write=False)
        _FAR.update(g=g, table=table, **far_layout(FAR_V, 1024))
    return _FAR


# ---- exact decisions (Python integers and fractions) and crafted entries ---------------------------------------------------

def exact_decisions(entries, t):
    """entries [n, 8] -> (exceeds, near), bool [n] each: num^2 > t dx dy over the integers and fractions.Fraction(t) (the
    exact value of the float), and the near ties |num^2 - t dx dy| <= 2^-48 num^2 with num != 0, the only entries at which
    three float64 products and three conversions, each within 2^-53, may decide otherwise (with num = 0 the left side is an
    exact 0 in float64 too, and never exceeds)"""
    from fractions import Fraction
    tt = Fraction(float(t))
    ex, near = [], []
    for e in np.asarray(entries).reshape(-1, 8).tolist():
        n, hm, am, mh, ma, hh, ha, aa = e
        sx, sxx, sy, syy, sxy = hm + 2 * am, hm + 4 * am, mh + 2 * ma, mh + 4 * ma, hh + 2 * ha + 4 * aa
        num, dx, dy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
        ex.append(num * num > tt * dx * dy)
        near.append(num != 0 and abs(num * num - tt * dx * dy) <= Fraction(num * num, 1 << 48))
    return np.array(ex), np.array(near)


def scaled_entries(seed=0):
    """the entries of a real table (ld_genotypes(1, 130, 600) at window 7), all eight counts of each multiplied by one
    factor per entry, drawn so that the entry's largest count lies in [2^28, 2^30) -> (small int64 [n, 8], scaled int64
    [n, 8]); r^2 is the same in both, N sxy and its like pass 2^57"""
    rng = np.random.default_rng(seed)
    small = np_ld_table(ld_genotypes(1, 130, 600), 7).reshape(-1, 8)
    top = small.max(axis=1)
    k = np.ones(len(small), np.int64)
    live = top > 0
    lo, hi = -(-(1 << 28) // top[live]), ((1 << 30) - 1) // top[live]
    k[live] = rng.integers(lo, hi + 1)
    big = small * k[:, None]
    assert (big[live].max(axis=1) >= 1 << 28).all() and big.max() < 1 << 30
    return small, big


def duplicate_entry(n, het, alt, k=1):
    """a variant of n complete calls, het HET and alt HOM_ALT, against itself, counts times k: r^2 is exactly 1"""
    return [n * k, het * k, alt * k, het * k, alt * k, het * k, 0, alt * k]


def quarter_entry(k=1):
    """two 0 / 1 dosages over 8 samples with the 2 x 2 table (3, 1; 1, 3), counts times k: num = 8 k^2, dx = dy = 16 k^2,
    so r^2 is exactly 1/4 — and in float64 too, whatever k: dx and dy are twice num, so dx dy rounds to 4 (num num)"""
    return [8 * k, 4 * k, 0, 4 * k, 0, 3 * k, 0, 0]


def tie_entries():
    """-> (entries int64 [n, 8], r2 [n]): crafted entries whose r^2 is exactly 1 or exactly 1/4, at small counts and scaled
    to the top of the contract's range (below 2^30)"""
    e = [duplicate_entry(130, 40, 7), duplicate_entry(130, 40, 7, 8259552), duplicate_entry(97, 1, 0),
         duplicate_entry(64, 0, 32, 1 << 23), quarter_entry(), quarter_entry(3), quarter_entry((1 << 27) - 1),
         quarter_entry(123456789)]
    return np.array(e, np.int64), np.array([1.0] * 4 + [0.25] * 4)


# ---- plane_positions ------------------------------------------------------------------------------------------------------

def brute_positions(v_lo, v_hi, blocksize, block0):
    vb = blocksize // 2
    wpb = -(-vb // 32)
    return np.array([(v // vb - block0) * wpb * 32 + v % vb for v in range(v_lo, v_hi)], np.int64).reshape(-1)


@pytest.mark.parametrize("v_lo,v_hi,blocksize,block0", [
    (0, 700, 200, None),          # padded: 100 variants per block in 4 words (128 positions)
    (150, 433, 200, None),        # cut inside blocks at both ends; the row begins at block 1
    (150, 433, 200, 0),           # the same variants in a row that begins at block 0
    (250, 251, 200, 1),
    (0, 9000, 8192, None),        # 4096 per block, no padding
    (5000, 9000, 8192, 0),
    (64, 64, 256, None),          # empty
])
def test_plane_positions(v_lo, v_hi, blocksize, block0):
    got = S_.plane_positions(v_lo, v_hi, blocksize) if block0 is None else S_.plane_positions(v_lo, v_hi, blocksize, block0)
    b0 = v_lo // (blocksize // 2) if block0 is None else block0
    assert got.dtype == np.int64 and np.array_equal(got, brute_positions(v_lo, v_hi, blocksize, b0))
    if v_hi > v_lo:
        assert np.all(np.diff(got) >= 1)


def test_plane_positions_agree_with_the_plane_planner():
    # a block's bits start at plan_planes' out_word, variant `lo` of the selection at bit lo of it
    sc, vc, bs, n_var = 64, 100, 200, 700
    for v_lo, v_hi in ((0, 700), (150, 433)):
        plan = S_.plan_planes(np.arange(130), 130, sc, vc, n_var, v_lo, v_hi, blocksize=bs)
        pos = S_.plane_positions(v_lo, v_hi, bs)
        want = sorted({int(w) * 32 + v for w, a, b in zip(plan["out_word"], plan["lo"], plan["hi"]) for v in range(a, b)})
        assert pos.tolist() == want


def test_plane_positions_padding_is_skipped_and_bad_rows_raise():
    pos = S_.plane_positions(0, 300, 200)
    assert pos[99] == 99 and pos[100] == 128 and pos[200] == 256          # positions 100..127 are padding
    with pytest.raises(IndexError):
        S_.plane_positions(100, 200, 200, 2)                              # the row begins behind the first variant
    with pytest.raises(IndexError):
        S_.plane_positions(10, 5, 200)


# ---- ld_sums, r2_from_counts, ld_exceeds -------------------------------------------------------------------------------------

S, V, W = 70, 300, 7


@pytest.fixture(scope="module")
def cohort():
    g = ld_genotypes(1, S, V)
    return g, np_ld_table(g, W)


def test_column_constants():
    assert (S_.LD_N, S_.LD_HM, S_.LD_AM, S_.LD_MH, S_.LD_MA, S_.LD_HH, S_.LD_HA, S_.LD_AA) == tuple(range(8))


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_sums_r2_and_exceeds_against_the_restatement(cohort, kind):
    g, table = cohort
    arg = table.astype(np.int32) if kind == "numpy" else torch.from_numpy(table.astype(np.int32))
    host = (lambda x: x) if kind == "numpy" else (lambda x: x.numpy())
    m, h, a = np_classes(g)
    x = (h + 2 * a).astype(np.int64)                    # dosage where complete
    sums = [host(s) for s in S_.ld_sums(arg)]
    assert all(s.dtype == np.int64 and s.shape == (V, W) for s in sums)
    for k, d in ((0, 0), (5, 6), (100, 3), (V - 2, 0), (V // 2, 2)):
        v = k + 1 + d
        both = m[:, k] & m[:, v]
        xs, ys = x[both, k], x[both, v]
        assert [int(s[k, d]) for s in sums] == [both.sum(), xs.sum(), ys.sum(), (xs * xs).sum(), (ys * ys).sum(), (xs * ys).sum()]
    r2 = host(S_.r2_from_counts(arg))
    check_r2(r2, np_r2(table))
    # the squared Pearson correlation of the dosages over the jointly complete samples: np.corrcoef centres in floating
    # point and sums S = 70 terms, so it agrees to a few hundred ulp at most; 1e-9 is far above that and far below any
    # difference a wrong column would make
    n_checked = 0
    for k in range(0, V - W, 11):
        for d in (0, W - 1):
            v = k + 1 + d
            both = m[:, k] & m[:, v]
            xs, ys = x[both, k], x[both, v]
            if xs.std() == 0 or ys.std() == 0:
                assert np.isnan(r2[k, d])
                continue
            np.testing.assert_allclose(r2[k, d], np.corrcoef(xs, ys)[0, 1] ** 2, rtol=1e-9)
            n_checked += 1
    assert n_checked >= 20
    for t in (0.2, 0.8, 0.999999):
        ex = host(S_.ld_exceeds(arg, t))
        assert ex.dtype == bool and np.array_equal(ex, np_exceeds(table, t))
        assert ex.any() and not ex.all()


def test_special_cases(cohort):
    g, table = cohort
    r2 = S_.r2_from_counts(table)
    dup, mono = V // 2, V // 3
    assert np.array_equal(g[:, dup + 3], g[:, dup])
    assert r2[dup, 2] == 1.0                                            # a duplicate: exactly 1
    assert S_.ld_exceeds(table, 0.999999)[dup, 2]
    for d in range(W):                                                  # monomorphic: NaN both ways round, never exceeds
        assert np.isnan(r2[mono, d]) and np.isnan(r2[mono - 1 - d, d])
        assert not S_.ld_exceeds(table, 0.0)[mono, d] and not S_.ld_exceeds(table, 0.0)[mono - 1 - d, d]
    assert np.all(table[V - 1] == 0) and np.all(np.isnan(r2[V - 1]))    # past the end: N = 0
    none = np.zeros((1, 1, 8), np.int32)
    assert np.isnan(S_.r2_from_counts(none)[0, 0]) and not S_.ld_exceeds(none, 0.0)[0, 0]
    assert np.isnan(S_.r2_from_counts(torch.from_numpy(none)).numpy()[0, 0])


@pytest.mark.parametrize("n_samples,n_variants,window", [(130, 600, 50), (70, 300, 7)])
def test_np_prune_on_the_recipe(n_samples, n_variants, window):
    g = ld_genotypes(1, n_samples, n_variants)
    table = np_ld_table(g, window)
    keep = np_prune(table, 0.2)
    assert keep[0] and keep[n_variants // 3]                             # the first, and the monomorphic one
    assert not keep[n_variants // 2 + 3] or not keep[n_variants // 2]    # of two duplicates in one window, not both
    assert 0.2 * n_variants <= keep.sum() <= 0.8 * n_variants, keep.sum()
    r2 = np_r2(table)
    assert np.isnan(r2[:n_variants - window]).any() and (r2 == 1.0).any()
    # every dropped variant has a kept one before it that exceeds; no two kept ones within a window do
    ex = np_exceeds(table, 0.2)
    for v in range(n_variants):
        hits = [u for u in range(max(v - window, 0), v) if keep[u] and ex[u, v - u - 1]]
        assert bool(hits) != bool(keep[v])
    assert np.array_equal(np_prune(table, 1.0), np.ones(n_variants, bool))


# ---- the long-range recipe bites -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def far():
    return far_cohort()


def test_far_recipe_layout_and_chance_pairs(far):
    """the recipe is what it says: every planted copy lies past position 1024, the planted places are apart, and at 0.5 (and
    at 0.999999) the pairs that exceed within 1024 places are exactly the pairs of identical planted variants — no chance
    pair among 3 million at S = 130 —, so every decision of a walk is one the layout names"""
    g, table, dups, chains = far["g"], far["table"], far["dups"], far["chains"]
    assert g.shape == (FAR_S, FAR_V, 2) and g.dtype == np.int8 and (g == -9).any()
    assert [D for D, _, _ in dups] == list(FAR_DISTANCES) and sorted(chains) == list(FAR_WINDOWS)
    groups = [(o, c) for _, o, c in dups] + list(chains.values())
    spots = sorted((x, i) for i, grp in enumerate(groups) for x in grp)
    assert all(b - a >= 3 for (a, i), (b, j) in zip(spots, spots[1:]) if i != j)
    assert spots[-1][0] < FAR_V and min(c for _, _, c in dups) > 1024
    want = {(a, b) for grp in groups for a in grp for b in grp if a < b and b - a <= 1024}
    for t in (0.5, 0.999999):
        u, d = np.nonzero(np_exceeds(table, t))
        assert {(int(a), int(a + 1 + b)) for a, b in zip(u, d)} == want
    for grp in groups:
        assert all(np.array_equal(g[:, grp[0]], g[:, x]) for x in grp[1:])


@pytest.mark.parametrize("window", FAR_WINDOWS)
def test_far_recipe_is_sensitive_to_every_register_word(far, window):
    """conditions on the data that the GPU tests of hhgt_ld_prune at 4, 8 and 16 register words lean on: a walk that drops
    an upper word of the keep-flag register or loses its carry, or cuts d < window one place early or late, gives another
    mask on this recipe.  A seed that fails them is the wrong seed."""
    table, dups, (u0, u, v) = far["table"][:, :window], far["dups"], far["chains"][window]
    keep = np_prune(table, 0.5)
    # a copy within reach goes, the first one out of reach stays; originals stay
    assert {window, window + 1} <= {D for D, _, _ in dups}
    for D, orig, copy in dups:
        assert keep[orig] and keep[copy] == (D > window), (D, window)
    # the chain: v's only exceeding predecessor in reach is u, whose flag is 0
    d1, d2 = chain_distances(window)
    assert (v - u, u - u0) == (d1, d2) and window / 2 < d2 <= d1 <= window < d1 + d2
    assert (keep[u0], keep[u], keep[v]) == (True, False, True)
    # every word of the register decides alone somewhere: a pruned variant whose only kept exceeding predecessor lies at
    # bit d = v - u - 1 of that word
    ex = np_exceeds(table, 0.5)
    alone = set()
    for x in np.nonzero(~keep)[0]:
        cand = np.arange(max(x - window, 0), x)
        hits = cand[keep[cand] & ex[cand, x - cand - 1]]
        if len(hits) == 1:
            alone.add(int(x - hits[0] - 1) // 64)
    assert alone >= set(range(-(-window // 64))), (window, sorted(alone))
    # and the next narrower register is not enough
    half = 64 * walk_words(window) // 2
    assert half < window and not np.array_equal(np_prune(table[:, :half], 0.5), keep)
    # at 1 nothing exceeds: every variant stays, duplicates included
    assert np_prune(table, 1.0).all()


# ---- the decision arithmetic: np_exceeds and store.ld_exceeds against exact integers ---------------------------------------

def test_exceeds_matches_exact_integers_at_large_counts():
    """a 32-bit (or float32) intermediate anywhere in N sxy - sx sy passes every table of 130 samples; here the counts
    reach 2^30 - 1 and the decisions are compared with Python integers.  Near ties (exact_decisions) are left out and must
    be at most 1 % — a condition on the data."""
    small, big = scaled_entries()
    assert len(big) == 600 * 7 and (np.abs(np_products(big)[0]) > 2.0 ** 100).any()
    for t in (0.0, 0.2, 0.5, 1.0):
        ex_small, _ = exact_decisions(small, t)
        ex, near = exact_decisions(big, t)
        assert np.array_equal(ex, ex_small)                              # r^2 does not change under the scaling
        assert near.mean() <= 0.01, (t, near.sum())
        for got in (np_exceeds(big, t), S_.ld_exceeds(big, t), S_.ld_exceeds(torch.from_numpy(big), t).numpy()):
            assert np.array_equal(got[~near], ex[~near]), t
        assert ex.any() == (t < 1.0) and not ex.all()
    # a product taken in 32 bits decides otherwise: the comparison notices
    n, hm, am, mh, ma, hh, ha, aa = (big[:, c].astype(np.int32) for c in range(8))
    with np.errstate(over="ignore"):
        num = n * (hh + 2 * ha + 4 * aa) - (hm + 2 * am) * (mh + 2 * ma)
        dx, dy = n * (hm + 4 * am) - (hm + 2 * am) ** 2, n * (mh + 4 * ma) - (mh + 2 * ma) ** 2
    wrong = num.astype(np.float64) ** 2 > 0.2 * (dx.astype(np.float64) * dy.astype(np.float64))
    assert not np.array_equal(wrong, exact_decisions(big, 0.2)[0])


def test_exceeds_at_ties_and_at_the_ends_of_the_range():
    """the contract says >: an entry whose r^2 is exactly t does not exceed, one ulp below it does (a >= would pass every
    other test); at 0 every entry with num != 0 exceeds and none with num = 0; at 1 nothing does"""
    entries, r2 = tie_entries()
    assert np.array_equal(np_r2(entries), r2)
    small, big = scaled_entries()
    every = np.concatenate([entries, small, big])
    num_is_0 = np_products(every)[0] == 0
    assert num_is_0.any() and not num_is_0.all()
    for f in (np_exceeds, S_.ld_exceeds):
        assert not f(entries, 1.0).any() and np.array_equal(f(entries, 0.25), r2 == 1.0)
        assert np.array_equal(f(entries, np.nextafter(1.0, 0.0)), r2 == 1.0)
        assert f(entries, np.nextafter(0.25, 0.0)).all() and not f(entries, np.nextafter(0.25, 1.0))[r2 == 0.25].any()
        assert np.array_equal(f(every, 0.0), ~num_is_0) and not f(every, 1.0).any()
    assert np.array_equal(exact_decisions(every, 0.0)[0], ~num_is_0) and not exact_decisions(every, 1.0)[0].any()
