"""hhgt_score_sums (the f64 MFMA over genotype planes) against numpy; GenotypeStore.score_sums / score / project against
the generator's genotypes and the formulas of store_stats restated in numpy; the reader and the command lines."""
import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd import synth
from haplohyped_varawareml_amd._lib import HhgtError
from haplohyped_varawareml_amd.store import (AC, AN, SCORE_SLICE, SCORE_SPAN, GenotypeStore, loadings_from_sums, plan_planes,
                                             projection_class_weights, standardized_dosages, top_eigenpairs)
from tests.test_assoc_stats import np_sums
from tests.test_gpu_allele_counts import CHROM3, S3, V3, cohort  # noqa: F401 (cohort: fixture)
from tests.test_gpu_assoc import PLANT_SEED, SAMPLES, guarded, two_populations, unpack
from tests.test_gpu_ld import GROUP, random_vplanes, write_store
from tests.test_gpu_sample_counts import np_variant_mask, two_groups  # noqa: F401 (two_groups: fixture)
from tests.test_grm_stats import np_counts, np_grm_sums
from tests.test_score_stats import np_dense_score, np_score_sums

pytestmark = pytest.mark.gpu

ROWS = [1, 15, 16, 17, 127, 128, 129, 257]                 # around a wave's 16 rows and a workgroup's 128
COLS = [1, 15, 16, 17, 33, 64]                             # around the column tiles of 16
# row words: the first few, around the staged slice and around one and two spans (0: nothing to do)
WORDS = sorted({1, 2, 3, SCORE_SLICE - 1, SCORE_SLICE + 1, SCORE_SPAN - 1, SCORE_SPAN, SCORE_SPAN + 1, 2 * SCORE_SPAN + 1})
CLASS_OF_PLANE = (1, 0, 2)                                 # planes HET, HOM_REF, HOM_ALT read the weights of dosage 1, 0, 2


# ---- the kernel ------------------------------------------------------------------------------------------------------------
def np_kernel(planes, w, w_lo=0, w_hi=None):
    """uint32 [3, n, words], float64 [3, 32 words, C] -> float64 [n, C]: the bits of words [w_lo, w_hi) times the weights of
    each plane's class, the three planes added"""
    w_hi = planes.shape[2] if w_hi is None else w_hi
    bits = unpack(planes)[:, :, 32 * w_lo:32 * w_hi]
    return sum(bits[k] @ w[c, 32 * w_lo:32 * w_hi] for k, c in enumerate(CLASS_OF_PLANE))


def device_planes(ctx, planes):
    return torch.from_numpy(planes.view(np.int32)).to(ctx.device)


@pytest.mark.parametrize("words", WORDS)
def test_kernel_is_exact_on_quarters(ctx, words):
    """every row count with every length of row, and every column count with every length: quarters in [-2, 2], so every
    partial sum is representable and the sums, which ADD to what the tensor holds, are exact"""
    assert SCORE_SLICE - 1 in WORDS and 2 * SCORE_SPAN + 1 in WORDS and len(WORDS) >= 8
    for i, n_rows in enumerate(ROWS):
        n_cols = COLS[(i + WORDS.index(words)) % len(COLS)]
        rng = np.random.default_rng(1000 * words + n_rows)
        w = rng.integers(-8, 9, (3, 32 * words, n_cols)) / 4.0
        planes, _ = random_vplanes(rng, n_rows, words)       # (H, M, A: the planes overlap, and all of them count)
        start = rng.integers(-8, 9, (n_rows, n_cols)) / 4.0
        buf, view = guarded(ctx, (n_rows, n_cols))
        view.copy_(torch.from_numpy(start))
        got = ctx.score_sums(device_planes(ctx, planes), torch.from_numpy(w).to(ctx.device), sums=view)
        assert got is view
        host = buf.cpu().numpy()
        assert np.isnan(host[:1024]).all() and np.isnan(host[-1024:]).all()
        assert np.array_equal(host[1024:-1024].reshape(n_rows, n_cols), start + np_kernel(planes, w)), (n_rows, n_cols)


@pytest.mark.parametrize("n_rows, n_cols", [(129, 17), (16, 64), (257, 1)])
def test_kernel_ranges(ctx, n_rows, n_cols):
    words = 2 * SCORE_SPAN + 1
    rng = np.random.default_rng(n_rows)
    w = rng.integers(-8, 9, (3, 32 * words, n_cols)) / 4.0
    planes, _ = random_vplanes(rng, n_rows, words)
    d_planes, d_w = device_planes(ctx, planes), torch.from_numpy(w).to(ctx.device)
    whole = ctx.score_sums(d_planes, d_w)
    assert whole.is_cuda and whole.dtype == torch.float64 and tuple(whole.shape) == (n_rows, n_cols)
    assert np.array_equal(whole.cpu().numpy(), np_kernel(planes, w))
    # a sub-range: the weights outside it are not read (NaN there), whatever its ends' place in a span
    for lo, hi in ((3, 100), (1, 2), (SCORE_SPAN - 1, 2 * SCORE_SPAN), (5, 5 + SCORE_SPAN), (words - 1, words)):
        assert 0 < lo < hi <= words
        masked = np.full_like(w, np.nan)
        masked[:, 32 * lo:32 * hi] = w[:, 32 * lo:32 * hi]
        got = ctx.score_sums(d_planes, torch.from_numpy(masked).to(ctx.device), lo, hi).cpu().numpy()
        assert np.array_equal(got, np_kernel(planes, w, lo, hi)), (lo, hi)
    # two calls over [0, a) and [a, words) into one tensor are one call, bit for bit
    for a in (1, SCORE_SPAN, SCORE_SPAN + 7):
        two = ctx.score_sums(d_planes, d_w, a, words, sums=ctx.score_sums(d_planes, d_w, 0, a))
        assert torch.equal(two.view(torch.int64), whole.view(torch.int64)), a
    # an empty range touches nothing
    nan = torch.full((n_rows, n_cols), float("nan"), dtype=torch.float64, device=ctx.device)
    for lo in (0, 7, words):
        assert torch.isnan(ctx.score_sums(d_planes, d_w, lo, lo, sums=nan)).all()
    # no bit: zeros are added; every bit: the column totals of the three classes
    for fill, want in ((0, np.zeros(n_cols)), (-1, w.sum(axis=(0, 1)))):
        full = torch.full((3, n_rows, words), fill, dtype=torch.int32, device=ctx.device)
        assert np.array_equal(ctx.score_sums(full, d_w).cpu().numpy(), np.broadcast_to(want, (n_rows, n_cols)))


@pytest.mark.parametrize("n_rows, words, n_cols", [(130, 2 * SCORE_SPAN + 5, 13), (65, 8, 64), (17, 3, 33)])
def test_kernel_error_bound_on_real_weights(ctx, n_rows, words, n_cols):
    """an entry that sums m values is within m 2^-52 sum |w| of numpy's float64 sum: hhgt_score_sums' first-order bound
    (m - 1) 2^-53 sum |w|, doubled for the second-order terms and for numpy's own summation"""
    rng = np.random.default_rng(n_rows)
    w = rng.normal(size=(3, 32 * words, n_cols))
    planes, _ = random_vplanes(rng, n_rows, words)
    want, total = np_kernel(planes, w), np_kernel(planes, np.abs(w))
    m = unpack(planes).sum(axis=(0, 2))[:, None]
    d_planes, d_w = device_planes(ctx, planes), torch.from_numpy(w).to(ctx.device)
    got, again = ctx.score_sums(d_planes, d_w), ctx.score_sums(d_planes, d_w)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))                  # deterministic
    err, bound = np.abs(got.cpu().numpy() - want), m * 2.0 ** -52 * total
    print(f"score_sums {n_rows} x {32 * words} x {n_cols}: largest error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
    assert (err <= bound).all()


def test_kernel_arguments(ctx):
    dev = ctx.device
    planes = torch.zeros((3, 5, 2), dtype=torch.int32, device=dev)
    w = torch.ones((3, 64, 3), dtype=torch.float64, device=dev)
    assert tuple(ctx.score_sums(planes, w).shape) == (5, 3)
    for n_cols in (0, 65):
        with pytest.raises(HhgtError, match="columns"):
            ctx.score_sums(planes, torch.ones((3, 64, n_cols), dtype=torch.float64, device=dev))
    for lo, hi in ((2, 1), (0, 3), (3, 3)):
        with pytest.raises(HhgtError, match="words"):
            ctx.score_sums(planes, w, lo, hi)
    for kw in (dict(w=w.float()), dict(w=w[:, :63]), dict(w=w[:2]), dict(w=torch.ones((3, 96, 3), dtype=torch.float64, device=dev)),
               dict(w=w.cpu()), dict(w=torch.ones((3, 64, 6), dtype=torch.float64, device=dev)[:, :, ::2]), dict(w=w[:, :, 0]),
               dict(planes=planes.float()), dict(planes=planes[:2]), dict(planes=planes[:, :, :1]),
               dict(sums=torch.zeros((5, 3), dtype=torch.float32, device=dev)),
               dict(sums=torch.zeros((5, 4), dtype=torch.float64, device=dev)),
               dict(sums=torch.zeros((5, 3), dtype=torch.float64)),
               dict(sums=torch.zeros((5, 6), dtype=torch.float64, device=dev)[:, ::2])):
        with pytest.raises(ValueError):
            ctx.score_sums(**{**dict(planes=planes, w=w), **kw})
    # no row: an empty result; no word: nothing is added
    assert tuple(ctx.score_sums(planes[:, :0].contiguous(), w).shape) == (0, 3)
    none = ctx.score_sums(torch.zeros((3, 5, 0), dtype=torch.int32, device=dev), torch.zeros((3, 0, 3), dtype=torch.float64, device=dev))
    assert tuple(none.shape) == (5, 3) and not none.any()


# ---- the store -------------------------------------------------------------------------------------------------------------
TWICE = SAMPLES + [SAMPLES[2]]                             # one sample named twice


def test_store_score_sums(ctx, cohort):
    g, G = f"chr_{CHROM3}", cohort["bits"]                                            # G: [S, V, 2]
    names = synth.sample_names(S3)
    idx = np.array(TWICE)
    rng = np.random.default_rng(11)
    Wd = rng.integers(-8, 9, (3, V3, 5)) / 4.0
    for n_path, path in enumerate(cohort["paths"]):
        st = GenotypeStore(path, ctx=ctx)
        for samples, a, b in ((TWICE, 0, V3), ([names[i] for i in TWICE], 4000, 12500), (TWICE, 4095, 4097), (TWICE, 7, 7)):
            w = Wd[:, a:b] if a else torch.from_numpy(Wd).to(ctx.device)
            got = st.score_sums(w, g, samples, a, b)
            assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (len(idx), 5)
            assert np.array_equal(got.cpu().numpy(), np_score_sums(G[idx, a:b], Wd[:, a:b])), (path, a, b)
            assert a != b or not got.any()
        # a variant class as a device tensor and as a host array, and the output of ld_prune; NaN weights where masked
        vm = st.variant_mask(g, SAMPLES, 4000, 12500, min_maf=0.1)
        keep = np_variant_mask(G[np.array(SAMPLES), 4000:12500], min_maf=0.1)
        assert 0 < keep.sum() < len(keep)
        want = np_score_sums(G[idx, 4000:12500][:, keep], Wd[:, 4000:12500][:, keep])
        holes = Wd[:, 4000:12500].copy()
        holes[:, ~keep] = np.nan
        for mask in (vm, keep):
            assert np.array_equal(st.score_sums(holes, g, TWICE, 4000, 12500, variant_mask=mask).cpu().numpy(), want)
        if n_path == 0:
            kept = st.ld_prune(g, SAMPLES, 4000, 12500, variant_mask=vm, window=20, r2=0.2)
            k = kept.cpu().numpy()
            assert 0 < int(k.sum()) < keep.sum()
            assert np.array_equal(st.score_sums(Wd[:, 4000:12500], g, TWICE, 4000, 12500, variant_mask=kept).cpu().numpy(),
                                  np_score_sums(G[idx, 4000:12500][:, k], Wd[:, 4000:12500][:, k]))
        # windows and slabs: the same sums, every selected row of every touched block column once
        whole = np_score_sums(G[idx], Wd)
        for kw in (dict(), dict(plane_bytes=1), dict(slab_bytes=300_000)):
            st.stats.update(score_plane_blocks=0, score_variants=0, assoc_plane_blocks=0)
            assert np.array_equal(st.score_sums({g: Wd}, samples=TWICE, **kw).cpu().numpy(), whole), kw
            plan = plan_planes(idx, S3, 64, 8192, V3, 0, V3)
            assert st.stats["score_plane_blocks"] == sum(bin(int(m)).count("1") for m in plan["row_mask"]) == 8 * 5
            assert st.stats["score_variants"] == V3 and st.stats["assoc_plane_blocks"] == 0
        st.stats.update(score_variants=0)
        st.score_sums(Wd[:, 4000:12500], g, TWICE, 4000, 12500, variant_mask=vm)
        assert st.stats["score_variants"] == keep.sum()
        # no sample: an empty table
        assert tuple(st.score_sums(Wd, g, []).shape) == (0, 5)
        # refusals, before anything is allocated: shapes, types, an unknown group, a listed group without weights
        torch.cuda.reset_peak_memory_stats(ctx.device)
        before = torch.cuda.max_memory_allocated(ctx.device)
        for bad in (Wd[:2], Wd[:, :-1], Wd.astype(np.float32), Wd[..., 0], np.ones((3, V3, 65)), np.ones((3, V3, 0))):
            with pytest.raises(ValueError):
                st.score_sums(bad, g, SAMPLES)
        with pytest.raises(KeyError):
            st.score_sums(Wd, "chr_6", SAMPLES)
        with pytest.raises(KeyError):
            st.score_sums({}, [g], SAMPLES)
        assert torch.cuda.max_memory_allocated(ctx.device) == before
        with pytest.raises(ValueError):
            st.score_sums(Wd, g, SAMPLES, variant_mask=keep[:100])
        st.close()


def test_store_score_leaves_read_cache_alone(ctx, cohort):
    g = f"chr_{CHROM3}"
    Wd = np.ones((3, V3, 2))
    for path in cohort["paths"]:
        st = GenotypeStore(path, ctx=ctx)
        a = st.score_sums(Wd, g, SAMPLES)
        n = st.stats["count_compressed_bytes_read"]
        assert torch.equal(st.score_sums(Wd, g, SAMPLES, slab_bytes=300_000), a)
        assert st.stats["count_compressed_bytes_read"] == 2 * n       # the same chunks read, once each, per call
        batch = [(g, s, 1000 * s % 15000, 1000 * s % 15000 + 3000) for s in (3, 70, 500, 999)]
        first = [r.cpu().numpy() for r in st.read_windows(batch)]
        keys, used, n = list(st._cache), st._cache_used, st.stats["chunks_read"]
        assert torch.equal(st.score_sums(Wd, g, SAMPLES), a)
        assert list(st._cache) == keys and st._cache_used == used
        again = [r.cpu().numpy() for r in st.read_windows(batch)]
        assert st.stats["chunks_read"] == n                           # served from the cache: nothing read from the file
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        m = st.stats["count_compressed_bytes_read"]
        st.score_sums(Wd[:, :100], g, [3], v_lo=0, v_hi=100)          # cached chunks are used, not read again
        assert st.stats["count_compressed_bytes_read"] == m
        st.close()


def test_several_groups_accumulate(ctx, two_groups):
    st = GenotypeStore(two_groups["path"], ctx=ctx)
    bits = two_groups["bits"]
    rng = np.random.default_rng(2)
    Wd = {g: rng.integers(-8, 9, (3, bits[g].shape[1], 3)) / 4.0 for g in bits}
    pick = [100, 3, 3]
    each = {g: st.score_sums(Wd[g], g, pick) for g in bits}
    for g in bits:
        assert np.array_equal(each[g].cpu().numpy(), np_score_sums(bits[g][pick], Wd[g]))
    total = st.score_sums(Wd, samples=pick)
    assert torch.equal(total, sum(each.values())) and torch.equal(total, st.score_sums(Wd, list(bits)[::-1], pick))
    one = list(bits)[0]
    assert torch.equal(st.score_sums(Wd, one, pick), each[one])
    with pytest.raises(KeyError):
        st.score_sums({one: Wd[one]}, list(bits), pick)
    with pytest.raises(ValueError):
        st.score_sums(Wd[one], None, pick)                                 # one array, two groups
    # score over both groups: the offsets add, the variants used are counted per group
    betas = {g: rng.normal(size=(bits[g].shape[1], 2)) for g in bits}
    got, used = st.score(betas, samples=pick)
    want = sum(np_dense_score(bits[g][pick], betas[g], np_counts(bits[g][[3, 100]]), "mean") for g in bits)
    V = sum(b.shape[1] for b in bits.values())
    tol = V * 2.0 ** -50 * sum(np.abs(b).sum(0) for b in betas.values())
    assert (np.abs(got.cpu().numpy() - want) <= tol[None, :]).all()
    assert used == {g: int((np_counts(bits[g][[3, 100]])[:, AN] > 0).sum()) for g in bits}
    st.close()


def test_store_score(ctx, cohort):
    """real betas against the dense formula: both routes sum at most V + 1 terms of size <= 2 |beta| per entry, so they
    differ by at most V 2^-50 sum |beta| (twice the first-order bound of either)"""
    g, G = f"chr_{CHROM3}", cohort["bits"]
    rng = np.random.default_rng(4)
    idx, freq = np.array(TWICE), np.arange(3, S3, 50)
    st = GenotypeStore(cohort["paths"][0], ctx=ctx)
    for a, b, K in ((0, V3, 3), (4000, 12500, 1)):
        beta = rng.normal(size=(b - a, K))
        tol = (b - a) * 2.0 ** -50 * np.abs(beta).sum(0)
        for impute in ("mean", "none"):
            for freq_samples, counts in ((None, np_counts(G[np.array(SAMPLES), a:b])), (freq, np_counts(G[freq, a:b]))):
                got, used = st.score(beta if K > 1 else beta[:, 0], g, TWICE, a, b, impute=impute, freq_samples=freq_samples)
                assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (len(idx), K)
                err = np.abs(got.cpu().numpy() - np_dense_score(G[idx, a:b], beta, counts, impute))
                print(f"score [{a}, {b}) {impute}, K = {K}: largest error / tolerance = {(err / tol[None, :]).max():.3g}")
                assert (err <= tol[None, :]).all()
                assert used == {g: b - a if impute == "none" else int((counts[:, AN] > 0).sum())}
    # under a mask a variant that is left out is in neither the sums nor the offset
    keep = np_variant_mask(G[np.array(SAMPLES), 4000:12500], min_maf=0.1)
    beta = rng.normal(size=(8500, 2))
    got, used = st.score(beta, g, TWICE, 4000, 12500, variant_mask=keep)
    counts = np_counts(G[np.array(SAMPLES), 4000:12500])
    want = np_dense_score(G[idx, 4000:12500][:, keep], beta[keep], counts[keep], "mean")
    assert (np.abs(got.cpu().numpy() - want) <= 8500 * 2.0 ** -50 * np.abs(beta).sum(0)[None, :]).all()
    assert used == {g: int(keep.sum())}
    with pytest.raises(ValueError):
        st.score(beta, g, TWICE, 4000, 12500, impute="median")
    st.close()


# ---- projection ---------------------------------------------------------------------------------------------------------------
TRAIN, HELD = list(range(64)), list(range(64, 96))


def np_projection(G, train, vectors, values):
    """the formulas of projection_weights restated on the genotypes -> (Wd float64 [3, V, k], Wd with every factor replaced
    by its absolute value)"""
    z, used = standardized_dosages(np_counts(G[train]))
    T, Ta = np_sums(G[train][:, used], vectors), np_sums(G[train][:, used], np.abs(vectors))
    Wd, Wa = np.zeros((3, G.shape[1], len(values))), np.zeros((3, G.shape[1], len(values)))
    Wd[:, used] = projection_class_weights(z[:, used], loadings_from_sums(T, z[:, used], values, int(used.sum())))
    Wa[:, used] = projection_class_weights(np.abs(z[:, used]), loadings_from_sums(Ta, np.abs(z[:, used]), np.abs(values), int(used.sum())))
    return Wd, Wa


def test_projection_of_held_out_samples(ctx, tmp_path):
    G, pop, _, _ = two_populations()
    write_store(ctx, str(tmp_path / "pops.hhgt"), G, 64, 128)
    st = GenotypeStore(str(tmp_path / "pops.hhgt"), ctx=ctx)
    values, vectors = st.pca(2, samples=TRAIN)
    got = st.project(vectors, values, TRAIN, HELD)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (len(HELD), 2)
    Wd, Wa = np_projection(G, TRAIN, vectors, values)
    want, scale = np_score_sums(G[HELD], Wd), np_score_sums(G[HELD], Wa)
    tol = (G.shape[1] + len(TRAIN)) * 2.0 ** -50 * scale
    err = np.abs(got.cpu().numpy() - want)
    print(f"project, held-out samples: largest error / tolerance = {(err / tol).max():.3g}")
    assert (err <= tol).all()
    # project = score_sums of projection_weights, which are the numpy formulas' weights
    W = st.projection_weights(vectors, values, samples=TRAIN)
    assert list(W) == [GROUP] and tuple(W[GROUP].shape) == (3, G.shape[1], 2)
    assert (np.abs(W[GROUP].cpu().numpy() - Wd) <= (len(TRAIN) + 4) * 2.0 ** -50 * Wa).all()
    assert torch.equal(st.score_sums(W, samples=HELD), got)
    # the first component separates the populations, and every held-out sample falls on its population's side
    side = [np.sign(vectors[pop[TRAIN] == p, 0]) for p in (0, 1)]
    assert all(len(set(s.tolist())) == 1 for s in side) and side[0][0] == -side[1][0] != 0
    held = got[:, 0].cpu().numpy()
    assert all((np.sign(held[pop[HELD] == p]) == side[p][0]).all() for p in (0, 1))
    # a variant mask takes part in the fit and in the projection alike
    mask = st.variant_mask(GROUP, TRAIN, min_maf=0.2)
    values_m, vectors_m = st.pca(2, samples=TRAIN, variant_mask=mask)
    keep = mask.cpu().numpy()
    Wd_m, Wa_m = np_projection(G[:, keep], TRAIN, vectors_m, values_m)
    err = np.abs(st.project(vectors_m, values_m, TRAIN, HELD, variant_mask=mask).cpu().numpy() - np_score_sums(G[HELD][:, keep], Wd_m))
    tol_m = (keep.sum() + len(TRAIN)) * 2.0 ** -50 * np_score_sums(G[HELD][:, keep], Wa_m)
    assert 0 < keep.sum() < len(keep) and (err <= tol_m).all()
    # refusals: a training sample twice, vectors of another length, an eigenvalue that is not positive
    with pytest.raises(ValueError):
        st.project(vectors, values, TRAIN[:-1] + [0], HELD)
    with pytest.raises(ValueError):
        st.project(vectors[:-1], values, TRAIN, HELD)
    with pytest.raises(ValueError, match="eigenvalue"):
        st.project(vectors, np.array([values[0], 0.0]), TRAIN, HELD)
    st.close()


def test_projection_returns_the_fitted_samples_without_missing_calls(ctx, tmp_path):
    """the cohort of two_populations() before its 1 % missing calls: project(training samples) is the training samples'
    eigenvector entries up to the relationship matrix's f32-chain error passed through eigh.  That error is not derivable
    here; it is measured against the reference — the distance between pca's vectors and numpy's eigh vectors of the float64
    relationship matrix of the same genotypes, per component — and 4 x that distance is allowed, for the conditioning of an
    eigenvector"""
    G, pop = two_populations()[:2]
    rng = np.random.default_rng(PLANT_SEED)                    # two_populations' first draws, without the missing calls
    base = rng.random(G.shape[1]) * 0.6 + 0.2
    freq = np.stack([base, np.clip(base + rng.uniform(-0.3, 0.3, G.shape[1]), 0.02, 0.98)])
    C = (rng.random(G.shape) < freq[pop][:, :, None]).astype(np.int8)
    assert (C[G != -9] == G[G != -9]).all() and 0.005 < (G == -9).mean() < 0.015 and C.min() == 0
    write_store(ctx, str(tmp_path / "complete.hhgt"), C, 64, 128)
    st = GenotypeStore(str(tmp_path / "complete.hhgt"), ctx=ctx)
    values, vectors = st.pca(2, samples=TRAIN)
    z, used = standardized_dosages(np_counts(C[TRAIN]))
    S, _, N = np_grm_sums(C[TRAIN], z.astype(np.float64), used)
    _, exact = top_eigenpairs(S / N, 2)
    distance = np.abs(vectors - exact).max(axis=0)
    err = np.abs(st.project(vectors, values, TRAIN, TRAIN).cpu().numpy() - vectors).max(axis=0)
    print(f"project(training samples) against the fitted vectors: {err} per component; "
          f"pca's vectors against float64 eigh: {distance}; allowed {4 * distance}")
    assert (distance > 0).all() and (err <= 4 * distance).all()
    st.close()


# ---- the reader and the command lines -------------------------------------------------------------------------------------
def test_reader_and_score_cli(ctx, cohort):
    from click.testing import CliRunner
    from haplohyped_varawareml_amd.assoc import main as assoc_main
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    from haplohyped_varawareml_amd.score import main
    tmp = cohort["tmp"]
    g, path = f"chr_{CHROM3}", cohort["paths"][0]
    names = synth.sample_names(S3)
    donors, freq = [names[i] for i in SAMPLES], [names[i] for i in range(3, S3, 50)]
    r = VCFH5Reader(path, ctx=ctx)
    st = r.store
    start, ref, alt, _ = st.variants(g)
    rng = np.random.default_rng(6)
    at = np.sort(rng.choice(V3, 500, replace=False))
    w = rng.normal(size=(len(at), 2))
    base = lambda x: [chr(c) for c in x]                                                               # noqa: E731
    listed = [(f"chr{CHROM3}", int(p) + 1, a, b) for p, a, b in zip(start[at], base(ref[at]), base(alt[at]))]
    other = "A" if chr(alt[at[0]]) != "A" else "C"
    # a position the store does not have, a two-base ALT at a position it has, another ALT base, another chromosome
    extra = [(f"chr{CHROM3}", int(start.max()) + 100, "A", "C"), (listed[0][0], listed[0][1], listed[0][2], listed[0][3] + "T"),
             (listed[0][0], listed[0][1], listed[0][2], other), ("chr6", listed[0][1], listed[0][2], listed[0][3])]
    variants, weights = listed + extra, np.concatenate([w, rng.normal(size=(len(extra), 2))])
    betas = np.zeros((V3, 2))
    betas[at] = w
    mask = np.zeros(V3, bool)
    mask[at] = True
    for impute, fr in (("mean", None), ("none", None), ("mean", freq)):
        rec, info = r.polygenic_scores(variants, weights, ["height", "weight"], donors, impute=impute, freq_donor_ids=fr)
        by_hand, used = st.score(betas, g, donors, variant_mask=mask, impute=impute, freq_samples=fr)
        assert rec.dtype.names == ("sample", "n_variants", "height", "weight") and [x.decode() for x in rec["sample"]] == donors
        assert np.array_equal(np.stack([rec["height"], rec["weight"]], axis=1), by_hand.cpu().numpy())
        assert (rec["n_variants"] == used[g]).all()
        assert info == dict(matched=len(at), unmatched=len(extra), unused=len(at) - used[g])
    one, _ = r.polygenic_scores(np.array(listed, dtype=[("chrom", "S8"), ("pos", np.int64), ("ref", "S1"), ("alt", "S1")]), w[:, 0],
                                donor_ids=donors, chromosomes=[CHROM3])
    assert one.dtype.names == ("sample", "n_variants", "score1")
    assert np.array_equal(one["score1"], st.score(betas[:, 0], g, donors, variant_mask=mask)[0].cpu().numpy()[:, 0])
    with pytest.raises(ValueError, match="twice"):
        r.polygenic_scores(variants + [listed[7]], np.concatenate([weights, weights[:1]]), donor_ids=donors)
    with pytest.raises(ValueError):
        r.polygenic_scores(variants, weights[:-1], donor_ids=donors)
    with pytest.raises(KeyError):
        r.polygenic_scores(variants, weights, donor_ids=donors, chromosomes=[6])
    # the command line: %.17g round-trips, so the file holds the reader's numbers
    lines = ["#CHROM\tPOS\tREF\tALT\theight\tweight"] + [
        "\t".join([c, str(p), a, b] + ["%.17g" % x for x in row]) for (c, p, a, b), row in zip(variants, weights.tolist())]
    (tmp / "weights.tsv").write_text("\n".join(lines) + "\n")
    (tmp / "score_samples.txt").write_text("\n".join(donors) + "\n")
    (tmp / "score_freq.txt").write_text("\n".join(freq) + "\n")
    out = str(tmp / "scores.tsv")
    common = ["--h5", path, "--weights", str(tmp / "weights.tsv"), "--out", out, "--sample_list", str(tmp / "score_samples.txt")]
    for args, kw in (([], dict()), (["--no_mean_imputation", "--columns", "weight"], dict(impute="none")),
                     (["--freq_sample_list", str(tmp / "score_freq.txt"), "--chromosome", str(CHROM3)], dict(freq_donor_ids=freq))):
        res = CliRunner().invoke(main, common + args)
        assert res.exit_code == 0, res.output
        cols = ["weight"] if "--columns" in args else ["height", "weight"]
        want, info = r.polygenic_scores(variants, weights[:, -len(cols):], cols, donors, **kw)
        got = [ln.split("\t") for ln in open(out).read().splitlines()]
        assert got[0] == ["#IID", "N_VARIANTS"] + cols and [c[0] for c in got[1:]] == donors
        assert [int(c[1]) for c in got[1:]] == want["n_variants"].tolist()
        for k, name in enumerate(cols):
            assert np.array_equal(np.array([float(c[2 + k]) for c in got[1:]]), want[name])
        assert f"{info['matched']} variants matched, {info['unmatched']} unmatched, {info['unused']} unused" in res.output
    # --columns BETA on the output of the assoc command line, as it is (untested variants say nan: they are left out)
    many = [names[i] for i in range(3, S3, 25)]
    y = rng.normal(size=len(many))
    (tmp / "score_pheno.tsv").write_text("#IID\ty\n" + "".join(f"{d}\t{v:.17g}\n" for d, v in zip(many, y)))
    res = CliRunner().invoke(assoc_main, ["--h5", path, "--pheno", str(tmp / "score_pheno.tsv"), "--out", str(tmp / "score_assoc.tsv")])
    assert res.exit_code == 0, res.output
    res = CliRunner().invoke(main, ["--h5", path, "--weights", str(tmp / "score_assoc.tsv"), "--columns", "BETA", "--out", out,
                                    "--sample_list", str(tmp / "score_samples.txt")])
    assert res.exit_code == 0, res.output
    scan = r.association(y, donor_ids=many)[0]
    tested = ~np.isnan(scan["beta"])
    assert 0 < tested.sum() < V3
    beta = np.where(tested, scan["beta"], 0.0)
    want = st.score(beta, g, donors, variant_mask=tested)[0].cpu().numpy()[:, 0]
    got = [ln.split("\t") for ln in open(out).read().splitlines()]
    assert got[0] == ["#IID", "N_VARIANTS", "BETA"] and np.array_equal(np.array([float(c[2]) for c in got[1:]]), want)
    # a sample the cohort lacks, an unknown column, a key twice: non-zero exits
    (tmp / "score_bad.txt").write_text("\n".join(donors + ["nobody"]) + "\n")
    (tmp / "weights_twice.tsv").write_text("\n".join(lines + lines[5:6]) + "\n")
    for args in (["--weights", str(tmp / "weights.tsv"), "--sample_list", str(tmp / "score_bad.txt")],
                 ["--weights", str(tmp / "weights.tsv"), "--columns", "bmi"],
                 ["--weights", str(tmp / "weights_twice.tsv")]):
        res = CliRunner().invoke(main, ["--h5", path, "--out", out] + args)
        assert res.exit_code != 0, args
    r.close()


def test_project_components_and_grm_cli(ctx, cohort):
    from click.testing import CliRunner
    from haplohyped_varawareml_amd.grm import main as grm_main
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    tmp = cohort["tmp"]
    g, path = f"chr_{CHROM3}", cohort["paths"][0]
    names = synth.sample_names(S3)
    train, held = [names[i] for i in range(3, S3, 25)], [names[i] for i in (0, 999, 500, 28)]     # (28 is a training donor)
    r = VCFH5Reader(path, ctx=ctx)
    st = r.store
    kw = dict(min_maf=0.05, ld_window=20, ld_r2=0.3)
    fitted, projected, values = r.project_components(3, train, held, **kw)
    pcs, pcs_values = r.principal_components(3, donor_ids=train, **kw)
    assert fitted.dtype == pcs.dtype and all(np.array_equal(fitted[f], pcs[f]) for f in pcs.dtype.names)
    assert np.array_equal(values, pcs_values)
    mask = st.ld_prune(g, train, variant_mask=st.variant_mask(g, train, min_maf=0.05), window=20, r2=0.3)
    vectors = np.stack([pcs[f"pc{c + 1}"] for c in range(3)], axis=1)
    by_hand = st.project(vectors, values, train, held, variant_mask=mask).cpu().numpy()
    assert projected.dtype == pcs.dtype and [x.decode() for x in projected["sample"]] == held
    assert np.array_equal(np.stack([projected[f"pc{c + 1}"] for c in range(3)], axis=1), by_hand)
    # the default: every sample outside the training set, in store order
    _, rest, _ = r.project_components(1, train, min_maf=0.05)
    assert [x.decode() for x in rest["sample"]] == [n for n in names if n not in set(train)]
    with pytest.raises(ValueError):
        r.project_components(len(train) + 1, train, held)
    # grm --project_list: PREFIX.projected.tsv beside files that do not change
    (tmp / "pc_train.txt").write_text("\n".join(train) + "\n")
    (tmp / "pc_held.txt").write_text("\n".join(held) + "\n")
    args = ["--h5", path, "--sample_list", str(tmp / "pc_train.txt"), "--min_maf", "0.05", "--ld_window", "20", "--ld_r2", "0.3",
            "--pcs", "3"]
    for prefix, more in (("plain", []), ("proj", ["--project_list", str(tmp / "pc_held.txt")])):
        res = CliRunner().invoke(grm_main, args + ["--out", str(tmp / prefix)] + more)
        assert res.exit_code == 0, res.output
    for ext in (".grm.npy", ".grm.id", ".eigenvec.tsv", ".eigenval.txt"):
        assert open(tmp / ("plain" + ext), "rb").read() == open(tmp / ("proj" + ext), "rb").read(), ext
    assert not (tmp / "plain.projected.tsv").exists()
    lines = [ln.split("\t") for ln in open(tmp / "proj.projected.tsv").read().splitlines()]
    assert lines[0] == open(tmp / "proj.eigenvec.tsv").read().splitlines()[0].split("\t") == ["#IID", "PC1", "PC2", "PC3"]
    assert [c[0] for c in lines[1:]] == held
    assert np.array_equal(np.array([[float(x) for x in c[1:]] for c in lines[1:]]), by_hand)
    res = CliRunner().invoke(grm_main, ["--h5", path, "--out", str(tmp / "bad"), "--project_list", str(tmp / "pc_held.txt")])
    assert res.exit_code != 0                                           # --project_list without --pcs
    r.close()
