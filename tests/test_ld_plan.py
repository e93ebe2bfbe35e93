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
        keep[v] = not any(keep[u] and ex[u, v - u - 1] for u in range(max(v - window, 0), v))
    return keep


def check_r2(got, want):
    """r^2 against the restatement: NaN in the same places, the rest within rtol 1e-12 (two products and one division in the
    same order differ by rounding at most)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=0)


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
