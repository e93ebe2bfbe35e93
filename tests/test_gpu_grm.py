"""-m gpu: the genetic relationship matrix.  hhgt_grm (64 x 64 tiles of pairs on the f32-input MFMA, plane bits expanded to
weights in LDS) against numpy with weights for which float32 is exact — one tile, the tile edge, off-diagonal and edge
tiles; rows below, at and across the ends of a chain; word sub-ranges; calls accumulating; the mirror write —; against
np_grm_chain of tests/test_grm_stats.py, the header's arithmetic restated on the CPU, where float32 rounds — the restart of
the chain every GRM_SPAN words from w_lo, exact; the chain bit for bit —; with standardised dosages of rare variants within
S_BOUND at up to eight spans; overlapping planes (HET before HOM_REF before HOM_ALT);
GenotypeStore.grm_sums / grm / pca, VCFH5Reader.genetic_relationship / principal_components and the grm CLI on converter
output against the synthetic generator's own genotypes in float64, within the bound of a float32 chain of 32 * GRM_SPAN
steps; two populations told apart by the first principal component."""
import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd import synth
from haplohyped_varawareml_amd._lib import HhgtError
from haplohyped_varawareml_amd.store import (NSNP, GenotypeStore, grm_from_sums, plan_planes, standardized_dosages,
                                             top_eigenpairs)
from tests.test_gpu_allele_counts import CHROM3, S3, V3, cohort  # noqa: F401 (cohort: fixture)
from tests.test_gpu_pair_counts import PICK, random_planes
from tests.test_gpu_sample_counts import np_variant_mask, two_groups  # noqa: F401 (two_groups: fixture)
from tests.test_grm_stats import (CHAIN_SHAPES, S_BOUND, SPAN_SUM, SPAN_W, chain_case, chain_ranges, chain_reference, np_counts,
                                  np_exact_ranges, np_grm_sums, np_plane_values, np_z, span_case, span_signs, span_split_sums,
                                  span_splits)

pytestmark = pytest.mark.gpu


# ---- the kernel ----------------------------------------------------------------------------------------------------------
def np_grm_words(planes, z, w_lo, w_hi):
    """uint32 [3, n, W] (HET, HOM_REF, HOM_ALT: disjoint), float32 [3, 32 W] (HOM_REF, HET, HOM_ALT) -> float64 [n, n] over
    the words [w_lo, w_hi)"""
    bits = np.unpackbits(np.ascontiguousarray(planes[:, :, w_lo:w_hi]).view(np.uint8), axis=-1, bitorder="little")
    zz = z[:, 32 * w_lo:32 * w_hi].astype(np.float64)
    x = bits[0] * zz[1] + bits[1] * zz[0] + bits[2] * zz[2]
    return x @ x.T


def quarter_weights(rng, W):
    """multiples of 1/4 in [-2, 2]: every product is a multiple of 1/16 of magnitude at most 4, and a sum of up to 2^18 of
    them is exact in float32 — 300 words are 9600"""
    return (rng.integers(-8, 9, (3, 32 * W)) / 4.0).astype(np.float32)


@pytest.mark.parametrize("n_rows", [1, 33, 64, 65, 130])
@pytest.mark.parametrize("row_words", [1, 5, 127, 128, 129, 300])
def test_grm_kernel_is_exact_on_quarters(ctx, n_rows, row_words):
    rng = np.random.default_rng(n_rows * 1000 + row_words)
    host, z = random_planes(rng, n_rows, row_words), quarter_weights(rng, row_words)
    planes, dz = torch.from_numpy(host.view(np.int32)).to(ctx.device), torch.from_numpy(z).to(ctx.device)
    want = np_grm_words(host, z, 0, row_words)
    assert row_words < 5 or np.abs(want).max() > 8
    table = ctx.grm(planes, dz)
    assert table.dtype == torch.float64 and tuple(table.shape) == (n_rows, n_rows) and table.is_cuda
    got = table.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got.view(np.uint64), got.T.copy().view(np.uint64))          # symmetric, bit for bit
    assert torch.equal(ctx.grm(planes, dz), table)                                    # the same bits every time
    # a table that holds an asymmetric pattern: both writes of a pair land where they belong, and a second call adds
    k = np.arange(n_rows, dtype=np.float64)
    pattern = k[:, None] * 4096.0 + k[None, :] * 3.0 + 1.0
    pre = torch.from_numpy(pattern.copy()).to(ctx.device)
    assert ctx.grm(planes, dz, table=pre) is pre
    assert np.array_equal(pre.cpu().numpy(), pattern + want)
    ctx.grm(planes, dz, table=pre)
    assert np.array_equal(pre.cpu().numpy(), pattern + 2 * want)
    # word ranges, also from a w_lo that is a multiple of nothing: chains are counted from w_lo
    ranges = [(row_words - 1, row_words)]
    if row_words >= 5:
        ranges += [(1, row_words), (3, row_words - 1)]
    if row_words >= 127:
        ranges += [(7, row_words - 2), (row_words - 125, row_words)]
    if row_words == 300:
        ranges += [(5, 133), (5, 134), (129, 300), (11, 11 + 257)]
    for a, b in ranges:
        assert np.array_equal(ctx.grm(planes, dz, a, b).cpu().numpy(), np_grm_words(host, z, a, b)), (a, b)
    cut = (row_words + 1) // 3
    acc = ctx.grm(planes, dz, 0, cut)                                                 # two word ranges make the whole
    ctx.grm(planes, dz, cut, row_words, table=acc)
    assert np.array_equal(acc.cpu().numpy(), want)
    # nothing to do: the table stays as it is
    for a, b in ((0, 0), (row_words, row_words), (cut, cut)):
        ctx.grm(planes, dz, a, b, table=pre)
    assert np.array_equal(pre.cpu().numpy(), pattern + 2 * want)
    assert not ctx.grm(torch.zeros_like(planes), dz).any()
    assert not ctx.grm(planes, torch.zeros_like(dz)).any()


def on_device(ctx, planes, z):
    return torch.from_numpy(planes.view(np.int32)).to(ctx.device), torch.from_numpy(z).to(ctx.device)


def grm_calls(ctx, planes, dz, ranges):
    """one table, one call per range"""
    table = None
    for a, b in ranges:
        table = ctx.grm(planes, dz, a, b, table=table)
    return table.cpu().numpy()


SPAN_ROWS = [dict(n_rows=2, plus=(0, 1), minus=()), dict(n_rows=66, plus=(0, 64), minus=(63, 65)),
             dict(n_rows=130, plus=(0, 64, 129), minus=(63, 65))]


@pytest.mark.parametrize("w_lo", [0, 5])
@pytest.mark.parametrize("rows", SPAN_ROWS, ids=lambda r: str(r["n_rows"]))
def test_grm_chain_restarts_every_span_from_w_lo(ctx, rows, w_lo):
    """the span case of tests/test_grm_stats.py: 4096 positions of 64 * 64 followed by 4096 of 2^-6 * 2^-6 sum to 2^24 + 1
    only if the first chain is put aside before the second begins, GRM_SPAN words from w_lo.  Guards an `in_span == SPAN`
    flush that never fires (2^24) and spans counted from word 0 (0.96 short at w_lo = 5).  At 66 and 130 rows the carrying
    rows sit on both sides of the tile edges, so the diagonal, off-diagonal and edge tiles all hold such pairs, of both signs;
    the other rows have no bit.  Then the same range in several calls into one table, where the second call's spans count
    from its own w_lo, against the emulator given the same calls.  Exact: nothing here depends on how the instruction takes
    its two positions."""
    host, z = span_case(w_lo, **rows)
    planes, dz = on_device(ctx, host, z)
    s = span_signs(**rows)
    want = SPAN_SUM * np.outer(s, s)
    assert (want != 0).sum() == len(rows["plus"] + rows["minus"]) ** 2
    got = ctx.grm(planes, dz, w_lo, SPAN_W).cpu().numpy()
    assert np.array_equal(got, want), (got[got != want][:4], want[got != want][:4])
    for ranges, (seq, two) in zip(span_splits(w_lo), span_split_sums(w_lo)):
        assert seq == two                                                             # (whatever the instruction does)
        want = seq * np.outer(s, s)                                                   # (rounding is symmetric in the sign)
        got = grm_calls(ctx, planes, dz, ranges)
        assert np.array_equal(got, want), (ranges, got[got != want][:4], want[got != want][:4])


@pytest.mark.parametrize("n_rows,row_words", CHAIN_SHAPES)
def test_grm_kernel_is_the_sequential_chain_bit_for_bit(ctx, n_rows, row_words):
    """the arithmetic contract of include/hhgt.h on weights that round at almost every step (tests/test_grm_stats.py shows
    that at least half of the entries differ from the exact sum and from the paired chain): the table equals
    np_grm_chain(paired=False) — one rounding per position, in ascending order, restarts every GRM_SPAN words from w_lo —
    in every bit, is symmetric in every bit, and is the same on a second call.  (On an MI355X the table differed from the
    sequential chain in no entry, from the paired chain in 76 % to 90 % of them: v_mfma_f32_32x32x2_f32 rounds after each
    of its two positions, as the header says.)"""
    host, z = chain_case(n_rows, row_words)
    planes, dz = on_device(ctx, host, z)
    for words in chain_ranges(row_words):
        table = ctx.grm(planes, dz, *words)
        got = table.cpu().numpy()
        seq, two = chain_reference(n_rows, row_words, words, False), chain_reference(n_rows, row_words, words, True)
        exact = np_exact_ranges(np_plane_values(host, z), [words])
        print(f"grm chain {n_rows} x {row_words} {words}: differs from the sequential chain in {(got != seq).mean():.3f} of "
              f"the entries, from the paired chain in {(got != two).mean():.3f}, from the exact sum in {(got != exact).mean():.3f}")
        assert np.array_equal(got.view(np.uint64), seq.view(np.uint64)), words
        assert np.array_equal(got.view(np.uint64), got.T.copy().view(np.uint64)), words
        assert torch.equal(ctx.grm(planes, dz, *words), table), words


def rare_cohort(n, V):
    """int8 [n, V, 2] with allele frequencies log-uniform from a singleton (1 / 2n) to 1/2, 1 % of the alleles missing:
    standardised values up to sqrt(n) at the rare variants, products with a heavy tail"""
    rng = np.random.default_rng(V)
    p = np.exp(rng.uniform(np.log(0.5 / n), np.log(0.5), V))
    g = (rng.random((n, V, 2)) < p[None, :, None]).astype(np.int8)
    g[rng.random((n, V, 2)) < 0.01] = -9
    return g


@pytest.mark.parametrize("row_words", [1, 128, 129, 1024])
def test_grm_kernel_with_real_weights_is_within_the_bound(ctx, row_words):
    """the header's bound at the kernel: float32 z of standardized_dosages, 130 rows, rows of one position word, one span,
    one span and a word, eight spans — every entry within S_BOUND * T of the float64 product of the same float32 values"""
    from tests.test_gpu_pair_counts import np_classes, pack_bits
    n = 130
    g = rare_cohort(n, 32 * row_words)
    z, used = standardized_dosages(np_counts(g))
    host = pack_bits(np_classes(g))
    assert host.shape == (3, n, row_words) and used.any() and (row_words == 1 or np.abs(z).max() > 10.0)
    x = np_plane_values(host, z).astype(np.float64)
    want, total = x @ x.T, np.abs(x) @ np.abs(x).T
    got = ctx.grm(*on_device(ctx, host, z)).cpu().numpy()
    err, bound = np.abs(got - want), S_BOUND * total
    print(f"grm kernel, {row_words} words: largest error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
    assert (err <= bound).all()
    assert np.array_equal(got.view(np.uint64), got.T.copy().view(np.uint64))


def test_grm_kernel_overlapping_planes_het_then_ref_then_alt(ctx):
    """the overlap rule of include/hhgt.h: a position with bits in several planes takes the HET weight before the HOM_REF
    weight before the HOM_ALT weight.  Every combination of the three bits, many times in every row, with quarter weights
    that differ between the classes at every position: exact.  Guards another order of the select chain, and planes whose
    weights add (hhgt_score_sums' rule, which np_grm_words restates: it must give another table here)."""
    n_rows, row_words = 65, 5
    rng = np.random.default_rng(65005)
    combo = rng.integers(0, 8, (n_rows, 32 * row_words))                              # bit 0 HET, 1 HOM_REF, 2 HOM_ALT
    assert min(int((combo[r] == c).sum()) for r in range(n_rows) for c in range(1, 8)) >= 5
    host = np.stack([np.packbits((combo >> k & 1).astype(bool), axis=1, bitorder="little").view(np.uint32) for k in range(3)])
    z = np.ascontiguousarray(rng.permuted(np.tile(np.r_[-8:0, 1:9], (32 * row_words, 1)), axis=1)[:, :3].T / 4.0, np.float32)
    assert (z[0] != z[1]).all() and (z[0] != z[2]).all() and (z[1] != z[2]).all() and (z != 0).all()
    x = np.where(combo & 1, z[1], np.where(combo & 2, z[0], np.where(combo & 4, z[2], 0.0))).astype(np.float64)
    assert np.array_equal(x, np_plane_values(host, z))
    want = x @ x.T
    assert not np.array_equal(np_grm_words(host, z, 0, row_words), want)
    planes, dz = on_device(ctx, host, z)
    got = ctx.grm(planes, dz).cpu().numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)
    for a, b in ((1, 4), (4, 5)):
        assert np.array_equal(ctx.grm(planes, dz, a, b).cpu().numpy(), x[:, 32 * a:32 * b] @ x[:, 32 * a:32 * b].T)


def test_grm_kernel_arguments(ctx):
    rng = np.random.default_rng(5)
    host, z = random_planes(rng, 10, 4), quarter_weights(rng, 4)
    planes, dz = torch.from_numpy(host.view(np.int32)).to(ctx.device), torch.from_numpy(z).to(ctx.device)
    none = ctx.grm(planes[:, :0].contiguous(), dz)                                    # no rows
    assert tuple(none.shape) == (0, 0)
    empty = ctx.grm(planes[:, :, :0].contiguous(), dz[:, :0].contiguous())            # no words
    assert tuple(empty.shape) == (10, 10) and not empty.any()
    with pytest.raises(HhgtError):
        ctx.grm(planes, dz, 2, 1)
    with pytest.raises(HhgtError):
        ctx.grm(planes, dz, 0, 5)
    for bad in (dict(planes=planes[:2].contiguous()), dict(planes=planes.to(torch.int64)), dict(planes=planes.transpose(1, 2)),
                dict(z=dz[:, :96].contiguous()), dict(z=dz.double()), dict(z=dz.cpu()), dict(z=dz[:2].contiguous()),
                dict(table=torch.zeros((10, 10), dtype=torch.float32, device=ctx.device)),
                dict(table=torch.zeros((10, 11), dtype=torch.float64, device=ctx.device)),
                dict(table=torch.zeros((10, 20), dtype=torch.float64, device=ctx.device)[:, ::2])):
        kw = dict(dict(planes=planes, z=dz), **bad)
        with pytest.raises(ValueError):
            ctx.grm(**kw)


# ---- the store -------------------------------------------------------------------------------------------------------------
def expected(G, idx, a, b, keep=None):
    """the contract on the generator's genotypes int8 [S, V, 2], in float64 (z not rounded): the samples idx (an index may
    repeat), the variants [a, b) that `keep` (bool [b - a], or None) marks -> (S, T, N, take): take = the variants that
    took part"""
    z, used = np_z(np_counts(G[np.unique(idx), a:b]))
    take = used if keep is None else used & keep
    return np_grm_sums(G[idx, a:b], z, take) + (take,)


def check_sums(got, want, what=None):
    (S, N), (wS, wT, wN, _) = got, want
    assert S.is_cuda and S.dtype == torch.float64 and N.is_cuda and N.dtype == torch.int32
    assert tuple(S.shape) == tuple(N.shape) == wS.shape
    S, N = S.cpu().numpy(), N.cpu().numpy()
    assert np.array_equal(N, wN), what
    err, bound = np.abs(S - wS), S_BOUND * wT
    print(f"grm_sums {what}: largest error / bound = {(err / np.maximum(bound, 1e-300)).max(initial=0.0):.3g}")
    assert (err <= bound).all(), what
    assert np.array_equal(S.view(np.uint64), S.T.copy().view(np.uint64)), what      # symmetric, bit for bit


def test_store_grm_sums(ctx, cohort):
    g, G = f"chr_{CHROM3}", cohort["bits"]                                            # G: [S, V, 2]
    names = synth.sample_names(S3)
    idx = np.array(PICK)
    for n_path, path in enumerate(cohort["paths"]):
        st = GenotypeStore(path, ctx=ctx)
        for samples, a, b in ((PICK, 0, V3), ([names[i] for i in PICK], 4000, 12500), (PICK, 4095, 4097), (PICK, 7, 7),
                              ([], 0, V3), ([S3 - 1], 0, V3)):
            ii = np.array([st._sample_index(x) for x in samples], np.int64)
            want = expected(G, ii, a, b)
            got = st.grm_sums(g, samples, a, b)
            check_sums(got, want, (path, a, b))
            if len(ii):                                                              # N is pair_counts' under the same mask
                assert torch.equal(got[1], st.pair_counts(g, samples, a, b, variant_mask=want[3])[..., NSNP])
            m = st.grm(g, samples, a, b)
            assert np.array_equal(m.cpu().numpy(), grm_from_sums(*got).cpu().numpy(), equal_nan=True)
            if len(ii) == len(PICK) and b - a > 1000:
                assert want[3].sum() > 1000 and m[0, 3] == m[0, 0] == m[3, 3] and m[0, 0] > 0.5      # the duplicate
        assert np.isnan(st.grm(g, PICK, 7, 7).cpu().numpy()).all()                    # no variant: N = 0
        # a variant class as a device tensor and as a host array, and the output of ld_prune
        vm = st.variant_mask(g, PICK, 4000, 12500, min_maf=0.05)
        keep = np_variant_mask(G[np.unique(idx), 4000:12500], min_maf=0.05)
        want = expected(G, idx, 4000, 12500, keep)
        assert 0 < want[3].sum() <= keep.sum() < len(keep)
        check_sums(st.grm_sums(g, PICK, 4000, 12500, variant_mask=vm), want, "device mask")
        check_sums(st.grm_sums(g, PICK, 4000, 12500, variant_mask=keep), want, "host mask")
        if n_path == 0:
            pruned = st.ld_prune(g, PICK, 4000, 12500, variant_mask=vm, window=20, r2=0.2)
            kept = pruned.cpu().numpy()
            assert pruned.is_cuda and 0 < kept.sum() < keep.sum()
            check_sums(st.grm_sums(g, PICK, 4000, 12500, variant_mask=pruned), expected(G, idx, 4000, 12500, kept), "ld_prune")
        # windows and slabs: the same bound, the same N, every selected row of every touched block column once
        whole = expected(G, idx, 0, V3)
        for kw in (dict(), dict(slab_bytes=300_000), dict(plane_bytes=1), dict(plane_bytes=3 * 384 * 128 * 4 * 2, slab_bytes=200_000)):
            st.stats.update(grm_plane_blocks=0, grm_words=0, pair_plane_blocks=0, pair_words=0)
            check_sums(st.grm_sums(g, PICK, **kw), whole, kw)
            plan = plan_planes(idx, S3, 64, 8192, V3, 0, V3)
            assert st.stats["grm_plane_blocks"] == sum(bin(int(m)).count("1") for m in plan["row_mask"]) == 8 * 5
            assert st.stats["grm_words"] == 5 * 128 and st.stats["pair_plane_blocks"] == st.stats["pair_words"] == 0
        with pytest.raises(ValueError):
            st.grm_sums(g, variant_mask=keep[:100])
        with pytest.raises(KeyError):
            st.grm_sums("chr_6")
        # both tables, 16 + 8 bytes per pair of plane rows, refused before anything is allocated
        torch.cuda.reset_peak_memory_stats(ctx.device)
        before = torch.cuda.max_memory_allocated(ctx.device)
        for call in (st.grm_sums, st.grm, lambda *a, **kw: st.pca(2, *a, **kw)):
            with pytest.raises(ValueError, match="max_table_bytes"):
                call(g, max_table_bytes=(24 << 20) - 1)                              # 1024 x 1024 pairs: one byte more
            with pytest.raises(ValueError, match="max_table_bytes"):
                call(g, PICK, max_table_bytes=384 * 384 * 24 - 1)
        assert torch.cuda.max_memory_allocated(ctx.device) == before
        check_sums(st.grm_sums(g, PICK, max_table_bytes=384 * 384 * 24), whole, "the table fits exactly")
        st.close()


def test_store_grm_leaves_read_cache_alone(ctx, cohort):
    g = f"chr_{CHROM3}"
    for path in cohort["paths"]:
        st = GenotypeStore(path, ctx=ctx)
        a = st.grm_sums(g, PICK)
        n = st.stats["count_compressed_bytes_read"]
        b = st.grm_sums(g, PICK, slab_bytes=300_000)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                    # (one plane window either way)
        assert st.stats["count_compressed_bytes_read"] == 2 * n       # the same chunks read, once each per stage, per call
        batch = [(g, s, 1000 * s % 15000, 1000 * s % 15000 + 3000) for s in (3, 70, 500, 999)]
        first = [r.cpu().numpy() for r in st.read_windows(batch)]
        keys, used, n = list(st._cache), st._cache_used, st.stats["chunks_read"]
        assert torch.equal(st.grm_sums(g, PICK)[0], a[0])
        assert list(st._cache) == keys and st._cache_used == used
        again = [r.cpu().numpy() for r in st.read_windows(batch)]
        assert st.stats["chunks_read"] == n                           # served from the cache: nothing read from the file
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        m = st.stats["count_compressed_bytes_read"]
        st.grm_sums(g, [3], v_lo=0, v_hi=100)                         # cached chunks are used, not read again
        assert st.stats["count_compressed_bytes_read"] == m
        st.close()


def expected_groups(bits, idx, keeps=None):
    parts = [expected(bits[g], idx, 0, bits[g].shape[1], None if keeps is None else keeps.get(g)) for g in bits]
    return tuple(sum(p[c] for p in parts) for c in range(3)) + (None,)


def np_top(grm, k):
    """the sign rule, restated"""
    w, v = np.linalg.eigh(grm)
    w, v = w[::-1][:k], v[:, ::-1][:, :k].copy()
    for c in range(k):
        if v[np.argmax(np.abs(v[:, c])), c] < 0:
            v[:, c] = -v[:, c]
    return w, v


def test_several_groups_and_pca(ctx, two_groups):
    st = GenotypeStore(two_groups["path"], ctx=ctx)
    bits, S = two_groups["bits"], two_groups["S"]
    every = np.arange(S)
    each = {g: st.grm_sums(g) for g in bits}
    for g in bits:
        check_sums(each[g], expected(bits[g], every, 0, bits[g].shape[1]), g)
    total = st.grm_sums(None)
    check_sums(total, expected_groups(bits, every), "every group")
    assert torch.equal(total[0], st.grm_sums(list(bits))[0]) and torch.equal(total[1], sum(e[1] for e in each.values()))
    assert torch.equal(total[0], sum(e[0] for e in each.values()))    # one window per group: the same additions
    pick = np.array([100, 3, 3, 129])
    masks = {g: st.variant_mask(g, pick, min_maf=0.05) for g in bits}
    keeps = {g: m.cpu().numpy() for g, m in masks.items()}
    check_sums(st.grm_sums(None, pick, variant_mask=masks), expected_groups(bits, pick, keeps), "a mask per group")
    one = {"chr_11": masks["chr_11"]}                                  # a group the dict does not name is counted whole
    check_sums(st.grm_sums(None, pick, variant_mask=one), expected_groups(bits, pick, {"chr_11": keeps["chr_11"]}), "one mask")
    with pytest.raises(ValueError):
        st.grm_sums(None, v_lo=5)
    with pytest.raises(ValueError):
        st.grm_sums(None, variant_mask=masks["chr_3"])
    # the matrix and its principal components
    m = st.grm()
    assert m.is_cuda and m.dtype == torch.float64 and torch.equal(m, grm_from_sums(*total)) and torch.equal(m, m.T)
    host = m.cpu().numpy()
    assert not np.isnan(host).any() and abs(np.trace(host) / S - 1.0) < 0.2
    for k in (1, 4, S):
        vals, vecs = st.pca(k)
        w, v = np_top(host, k)
        assert vals.dtype == vecs.dtype == np.float64 and vecs.shape == (S, k)
        assert np.array_equal(vals, w) and np.array_equal(vecs, v)
        assert np.abs(vecs.T @ vecs - np.eye(k)).max() < 1e-12
        assert (vecs[np.argmax(np.abs(vecs), axis=0), np.arange(k)] > 0).all() and (np.diff(vals) <= 0).all()
    sub = st.pca(2, "chr_3", pick[:2].tolist() + [7], variant_mask=masks["chr_3"])
    w, v = np_top(st.grm("chr_3", [100, 3, 7], variant_mask=masks["chr_3"]).cpu().numpy(), 2)
    assert np.array_equal(sub[0], w) and np.array_equal(sub[1], v)
    for k in (0, S + 1):
        with pytest.raises(ValueError):
            st.pca(k)
    with pytest.raises(ValueError):
        st.pca(4, samples=[1, 2, 3])
    with pytest.raises(ValueError, match="jointly complete"):
        st.pca(2, "chr_3", v_lo=7, v_hi=7)                             # no variant: N = 0 everywhere
    st.close()


# ---- two populations -----------------------------------------------------------------------------------------------------
def test_first_component_splits_two_populations(ctx, tmp_path):
    """96 samples x 4096 variants, the two halves of the samples (interleaved in store order) drawn from allele frequencies
    that differ by up to 0.3 per variant, 1 % of the alleles missing: the sign of PC1 is the population"""
    from tests.test_gpu_ld import GROUP, write_store
    rng = np.random.default_rng(8)
    n, V = 96, 4096
    pop = np.arange(n) % 2
    base = rng.random(V) * 0.6 + 0.2
    freq = np.stack([base, np.clip(base + rng.uniform(-0.3, 0.3, V), 0.02, 0.98)])
    G = (rng.random((n, V, 2)) < freq[pop][:, :, None]).astype(np.int8)
    G[rng.random((n, V, 2)) < 0.01] = -9
    write_store(ctx, str(tmp_path / "pops.hhgt"), G, 64, 128)
    st = GenotypeStore(str(tmp_path / "pops.hhgt"), ctx=ctx)
    check_sums(st.grm_sums(GROUP), expected(G, np.arange(n), 0, V), "two populations")
    vals, vecs = st.pca(3)
    assert vals[0] > 3 * vals[1]
    side = vecs[:, 0] > 0
    assert np.array_equal(side, pop == pop[np.argmax(np.abs(vecs[:, 0]))]) and side.sum() == n // 2
    st.close()


# ---- the reader and the CLI -----------------------------------------------------------------------------------------------
def test_reader_and_cli(ctx, cohort, two_groups):
    from click.testing import CliRunner
    from haplohyped_varawareml_amd.grm import main
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    tmp = cohort["tmp"]
    names = synth.sample_names(S3)
    donors = [names[i] for i in PICK]
    (tmp / "grm_samples.txt").write_text("\n".join(donors) + "\n")
    g = f"chr_{CHROM3}"
    for path in cohort["paths"][:2]:
        r = VCFH5Reader(path, ctx=ctx)
        st = r.store
        for kw in (dict(), dict(min_maf=0.05), dict(chromosomes=[CHROM3], min_maf=0.05, ld_window=20),
                   dict(ld_window=10, ld_r2=0.5)):
            mask = st.variant_mask(g, PICK, min_maf=kw["min_maf"]) if "min_maf" in kw else None
            if "ld_window" in kw:
                mask = st.ld_prune(g, PICK, variant_mask=mask, window=kw["ld_window"], r2=kw.get("ld_r2", 0.2))
            sums, nsnp = st.grm_sums(g, PICK, variant_mask=mask)
            who, m, n = r.genetic_relationship(donor_ids=donors, **kw)
            assert who == donors and m.dtype == np.float64 and n.dtype == np.int32
            assert np.array_equal(m, grm_from_sums(sums, nsnp).cpu().numpy()) and np.array_equal(n, nsnp.cpu().numpy())
            rec, vals = r.principal_components(3, donor_ids=donors, **kw)
            w, v = top_eigenpairs(m, 3)
            assert rec.dtype.names == ("sample", "pc1", "pc2", "pc3") and [x.decode() for x in rec["sample"]] == donors
            assert np.array_equal(vals, w) and all(np.array_equal(rec[f"pc{c + 1}"], v[:, c]) for c in range(3))
        with pytest.raises(ValueError):
            r.principal_components(10, donor_ids=donors)
        with pytest.raises(KeyError):
            r.genetic_relationship(6)
        with pytest.raises(KeyError):
            r.genetic_relationship(CHROM3, donor_ids=["nobody"])
        r.close()
    # every sample of a small cohort, several chromosomes; k defaults to 10
    r = VCFH5Reader(two_groups["path"], ctx=ctx)
    who, m, n = r.genetic_relationship()
    sums, nsnp = r.store.grm_sums(None)
    assert who == list(r.store.samples) and np.array_equal(m, grm_from_sums(sums, nsnp).cpu().numpy())
    rec, vals = r.principal_components()
    assert len(rec) == two_groups["S"] and len(rec.dtype.names) == 11 and len(vals) == 10
    assert np.array_equal(r.genetic_relationship([11])[2], r.store.grm_sums("chr_11")[1].cpu().numpy())
    r.close()
    # the CLI
    st = GenotypeStore(cohort["paths"][0], ctx=ctx)
    prefix = str(tmp / "rel")
    for args, mask, k in ((["--sample_list", str(tmp / "grm_samples.txt")], None, None),
                          (["--sample_list", str(tmp / "grm_samples.txt"), "--min_maf", "0.05", "--chromosome", str(CHROM3),
                            "--ld_window", "20", "--ld_r2", "0.3", "--pcs", "4"],
                           st.ld_prune(g, PICK, variant_mask=st.variant_mask(g, PICK, min_maf=0.05), window=20, r2=0.3), 4)):
        res = CliRunner().invoke(main, ["--h5", cohort["paths"][0], "--out", prefix] + args)
        assert res.exit_code == 0, res.output
        want = st.grm(g, PICK, variant_mask=mask).cpu().numpy()
        got = np.load(prefix + ".grm.npy")
        assert got.dtype == np.float64 and np.array_equal(got, want)                # the .npy round-trips
        assert open(prefix + ".grm.id").read().split() == donors
        if k:
            w, v = top_eigenpairs(want, k)
            lines = open(prefix + ".eigenvec.tsv").read().splitlines()
            assert lines[0] == "#IID\tPC1\tPC2\tPC3\tPC4" and [ln.split("\t")[0] for ln in lines[1:]] == donors
            assert np.array_equal(np.array([[float(x) for x in ln.split("\t")[1:]] for ln in lines[1:]]), v)
            assert np.array_equal(np.array([float(x) for x in open(prefix + ".eigenval.txt").read().split()]), w)
    st.close()
    res = CliRunner().invoke(main, ["--h5", cohort["paths"][0], "--out", prefix, "--sample_list", str(tmp / "grm_samples.txt"),
                                    "--pcs", "10"])
    assert res.exit_code != 0 and isinstance(res.exception, ValueError)
