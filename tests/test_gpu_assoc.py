"""hhgt_assoc_sums (the f64 MFMA over variant-major planes) against numpy, GenotypeStore.assoc_sums / assoc against the
generator's genotypes and the per-variant lstsq reference, the reader and the CLI."""
import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd import synth
from haplohyped_varawareml_amd._lib import HhgtError
from haplohyped_varawareml_amd.store import (ASSOC_P, ASSOC_T, GenotypeStore, assoc_design, assoc_from_sums, plan_planes)
from tests.test_assoc_stats import STAT_RTOL, np_lstsq_scan, np_sums, rel_diff
from tests.test_gpu_allele_counts import CHROM3, S3, V3, cohort  # noqa: F401 (cohort: fixture)
from tests.test_gpu_ld import random_vplanes
from tests.test_gpu_sample_counts import np_variant_mask

pytestmark = pytest.mark.gpu

SAMPLES = [900, 5, 64, 130, 999, 70, 3, 449]          # no duplicate, not in order, six chunk rows of 64


# ---- the kernel ------------------------------------------------------------------------------------------------------------
def unpack(planes):
    """uint32 [3, n, sw] -> float64 [3, n, 32 sw] of 0 / 1"""
    return np.unpackbits(planes.view(np.uint8), axis=2, bitorder="little").astype(np.float64)


def guarded(ctx, shape, guard=1024):
    """-> (buf, view): a float64 buffer of NaNs and the contiguous view of `shape` in its middle, `guard` doubles either side"""
    size = int(np.prod(shape))
    buf = torch.full((2 * guard + size,), float("nan"), dtype=torch.float64, device=ctx.device)
    return buf, buf[guard:guard + size].view(shape)


@pytest.mark.parametrize("sw", [1, 2, 3, 8, 79])
@pytest.mark.parametrize("n_cols", [1, 15, 16, 17, 33, 64])
def test_kernel_is_exact_on_quarters(ctx, sw, n_cols):
    rng = np.random.default_rng(100 * sw + n_cols)
    w = rng.integers(-8, 9, (32 * sw, n_cols)) / 4.0                   # multiples of 1/4 in [-2, 2]: every sum is exact
    d_w = torch.from_numpy(w).to(ctx.device)
    for n_var in (1, 15, 16, 17, 64, 65, 130):
        planes, _ = random_vplanes(rng, n_var, sw)
        want = unpack(planes) @ w                                      # [3, n, C]
        d_planes = torch.from_numpy(planes.view(np.int32)).to(ctx.device)
        got = ctx.assoc_sums(d_planes, d_w)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (n_var, 3, n_cols)
        assert np.array_equal(got.cpu().numpy(), want.transpose(1, 0, 2)), n_var
        # into the caller's tensor: every entry overwritten, nothing beside it touched, the same bits again
        buf, view = guarded(ctx, (n_var, 3, n_cols))
        assert ctx.assoc_sums(d_planes, d_w, sums=view) is view
        host = buf.cpu().numpy()
        assert np.isnan(host[:1024]).all() and np.isnan(host[-1024:]).all()
        assert np.array_equal(host[1024:-1024].view(np.uint64), got.cpu().numpy().reshape(-1).view(np.uint64)), n_var
    # no bit: zeros; every bit: the column totals (a plane is any bits)
    n_var = 33
    for fill, want in ((0, np.zeros(n_cols)), (-1, w.sum(axis=0))):
        d_planes = torch.full((3, n_var, sw), fill, dtype=torch.int32, device=ctx.device)
        got = ctx.assoc_sums(d_planes, d_w).cpu().numpy()
        assert np.array_equal(got, np.broadcast_to(want, (n_var, 3, n_cols)))


@pytest.mark.parametrize("n_var, sw, n_cols", [(130, 79, 13), (65, 8, 64), (17, 3, 33)])
def test_kernel_error_bound_on_real_weights(ctx, n_var, sw, n_cols):
    """an entry that sums m values is within m 2^-52 sum |w| of numpy's float64 sum: hhgt_assoc_sums' first-order bound
    (m - 1) 2^-53 sum |w|, doubled for the second-order terms and for numpy's own summation"""
    rng = np.random.default_rng(n_var)
    w = rng.normal(size=(32 * sw, n_cols))
    planes, _ = random_vplanes(rng, n_var, sw)
    bits = unpack(planes)
    want, total, m = bits @ w, bits @ np.abs(w), bits.sum(axis=2, keepdims=True)
    got = ctx.assoc_sums(torch.from_numpy(planes.view(np.int32)).to(ctx.device), torch.from_numpy(w).to(ctx.device))
    again = ctx.assoc_sums(torch.from_numpy(planes.view(np.int32)).to(ctx.device), torch.from_numpy(w).to(ctx.device))
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))                  # deterministic
    err, bound = np.abs(got.cpu().numpy().transpose(1, 0, 2) - want), m * 2.0 ** -52 * total
    print(f"assoc_sums {n_var} x {32 * sw} x {n_cols}: largest error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
    assert (err <= bound).all()


def test_kernel_arguments(ctx):
    dev = ctx.device
    planes = torch.zeros((3, 5, 2), dtype=torch.int32, device=dev)
    w = torch.ones((64, 3), dtype=torch.float64, device=dev)
    assert tuple(ctx.assoc_sums(planes, w).shape) == (5, 3, 3)
    for n_cols in (0, 65):
        with pytest.raises(HhgtError, match="columns"):
            ctx.assoc_sums(planes, torch.ones((64, n_cols), dtype=torch.float64, device=dev))
    for kw in (dict(w=w.float()), dict(w=w[:63]), dict(w=torch.ones((96, 3), dtype=torch.float64, device=dev)),
               dict(w=w.cpu()), dict(w=torch.ones((64, 6), dtype=torch.float64, device=dev)[:, ::2]), dict(w=w[:, 0]),
               dict(vplanes=planes.float()), dict(vplanes=planes[:2]), dict(vplanes=planes[:, :, :1]),
               dict(sums=torch.zeros((5, 3, 3), dtype=torch.float32, device=dev)),
               dict(sums=torch.zeros((5, 3, 4), dtype=torch.float64, device=dev)),
               dict(sums=torch.zeros((5, 3, 6), dtype=torch.float64, device=dev)[:, :, ::2])):
        with pytest.raises(ValueError):
            ctx.assoc_sums(**{**dict(vplanes=planes, w=w), **kw})
    # no variant: an empty result; no sample word: zeros
    assert tuple(ctx.assoc_sums(planes[:, :0].contiguous(), w).shape) == (0, 3, 3)
    none = ctx.assoc_sums(torch.zeros((3, 5, 0), dtype=torch.int32, device=dev), torch.zeros((0, 3), dtype=torch.float64, device=dev),
                          sums=torch.full((5, 3, 3), float("nan"), dtype=torch.float64, device=dev))
    assert tuple(none.shape) == (5, 3, 3) and not none.any()


# ---- the store -------------------------------------------------------------------------------------------------------------
def test_store_assoc_sums(ctx, cohort):
    g, G = f"chr_{CHROM3}", cohort["bits"]                                            # G: [S, V, 2]
    names = synth.sample_names(S3)
    idx = np.array(SAMPLES)
    rng = np.random.default_rng(5)
    W = rng.integers(-3, 4, (len(idx), 5)).astype(np.float64)
    W[:, 0] = 1.0
    y = rng.normal(size=len(idx)) + G[idx, 4100].clip(0).sum(1)
    for n_path, path in enumerate(cohort["paths"]):
        st = GenotypeStore(path, ctx=ctx)
        for samples, a, b in ((SAMPLES, 0, V3), ([names[i] for i in SAMPLES], 4000, 12500), (SAMPLES, 4095, 4097),
                              (SAMPLES, 7, 7)):
            got = st.assoc_sums(g, W if a else torch.from_numpy(W).to(ctx.device), samples, a, b)
            assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (b - a, 3, 5)
            assert np.array_equal(got.cpu().numpy(), np_sums(G[idx, a:b], W)), (path, a, b)
        # a variant class as a device tensor and as a host array, and the output of ld_prune
        vm = st.variant_mask(g, SAMPLES, 4000, 12500, min_maf=0.1)
        keep = np_variant_mask(G[idx, 4000:12500], min_maf=0.1)
        want = np_sums(G[idx, 4000:12500][:, keep], W)
        assert 0 < keep.sum() < len(keep)
        for mask in (vm, keep):
            assert np.array_equal(st.assoc_sums(g, W, SAMPLES, 4000, 12500, variant_mask=mask).cpu().numpy(), want)
        if n_path == 0:
            kept = st.ld_prune(g, SAMPLES, 4000, 12500, variant_mask=vm, window=20, r2=0.2)
            assert 0 < int(kept.sum()) < keep.sum()
            assert np.array_equal(st.assoc_sums(g, W, SAMPLES, 4000, 12500, variant_mask=kept).cpu().numpy(),
                                  np_sums(G[idx, 4000:12500][:, kept.cpu().numpy()], W))
        # windows and slabs: the same sums, every selected row of every touched block column once
        whole = np_sums(G[idx], W)
        for kw in (dict(), dict(plane_bytes=1), dict(slab_bytes=300_000)):
            st.stats.update(assoc_plane_blocks=0, assoc_variants=0, ld_plane_blocks=0)
            assert np.array_equal(st.assoc_sums(g, W, SAMPLES, **kw).cpu().numpy(), whole), kw
            plan = plan_planes(idx, S3, 64, 8192, V3, 0, V3)
            assert st.stats["assoc_plane_blocks"] == sum(bin(int(m)).count("1") for m in plan["row_mask"]) == 8 * 5
            assert st.stats["assoc_variants"] == V3 and st.stats["ld_plane_blocks"] == 0
        st.stats.update(assoc_variants=0)
        st.assoc_sums(g, W, SAMPLES, 4000, 12500, variant_mask=vm)
        assert st.stats["assoc_variants"] == keep.sum()
        # refusals: a sample twice (before anything is allocated), W of another shape or type, an unknown group
        torch.cuda.reset_peak_memory_stats(ctx.device)
        before = torch.cuda.max_memory_allocated(ctx.device)
        with pytest.raises(ValueError, match="twice"):
            st.assoc_sums(g, np.ones((3, 1)), [5, 70, 5])
        with pytest.raises(ValueError, match="twice"):
            st.assoc(g, np.arange(5.0), None, [names[5], 70, 3, 5, 9])
        assert torch.cuda.max_memory_allocated(ctx.device) == before
        for bad in (W[:7], W.astype(np.float32), np.ones((8, 65)), np.ones((8, 0)), W[:, 0]):
            with pytest.raises(ValueError):
                st.assoc_sums(g, bad, SAMPLES)
        with pytest.raises(ValueError):
            st.assoc_sums(g, W, SAMPLES, variant_mask=keep[:100])
        with pytest.raises(KeyError):
            st.assoc_sums("chr_6", W, SAMPLES)
        with pytest.raises(KeyError):
            st.assoc("chr_6", y, None, SAMPLES)
        # the scan of a real-valued phenotype against the per-variant lstsq, and assoc = design + sums + statistics
        stats, calls = st.assoc(g, y, None, SAMPLES, 4000, 6000)
        want, want_calls = np_lstsq_scan(G[idx, 4000:6000], y)
        assert stats.is_cuda and stats.dtype == torch.float64 and calls.is_cuda and calls.dtype == torch.int64
        assert np.array_equal(calls.cpu().numpy(), want_calls)
        d = rel_diff(stats.cpu().numpy(), want)
        print(f"assoc, 8 samples, no covariate: largest relative difference {d:.3g}, {int(np.isnan(want[:, 0, 0]).sum())} untested")
        assert d <= STAT_RTOL and 0 < np.isnan(want[:, 0, 0]).sum() < 2000
        Wd, q, yy = assoc_design(y)
        by_hand = assoc_from_sums(st.assoc_sums(g, Wd, SAMPLES, 4000, 6000), torch.from_numpy(Wd.sum(axis=0)).to(ctx.device), q,
                                  torch.from_numpy(yy).to(ctx.device))
        assert torch.equal(by_hand[1], calls) and np.array_equal(by_hand[0].cpu().numpy(), stats.cpu().numpy(), equal_nan=True)
        if n_path == 0:         # 200 samples, two covariates, two phenotypes
            many = np.arange(3, S3, 5)
            cov = rng.normal(size=(len(many), 2))
            yy2 = rng.normal(size=(len(many), 2)) + cov[:, :1] + 0.5 * G[many, 4100].clip(0).sum(1)[:, None]
            stats, calls = st.assoc(g, yy2, cov, many, 4000, 4600)
            want, want_calls = np_lstsq_scan(G[many, 4000:4600], yy2, cov)
            assert np.array_equal(calls.cpu().numpy(), want_calls)
            d = rel_diff(stats.cpu().numpy(), want)
            print(f"assoc, 200 samples, two covariates: largest relative difference {d:.3g}")
            assert d <= STAT_RTOL
        st.close()


def test_store_assoc_leaves_read_cache_alone(ctx, cohort):
    g = f"chr_{CHROM3}"
    W = np.ones((len(SAMPLES), 2))
    for path in cohort["paths"]:
        st = GenotypeStore(path, ctx=ctx)
        a = st.assoc_sums(g, W, SAMPLES)
        n = st.stats["count_compressed_bytes_read"]
        assert torch.equal(st.assoc_sums(g, W, SAMPLES, slab_bytes=300_000), a)
        assert st.stats["count_compressed_bytes_read"] == 2 * n       # the same chunks read, once each, per call
        batch = [(g, s, 1000 * s % 15000, 1000 * s % 15000 + 3000) for s in (3, 70, 500, 999)]
        first = [r.cpu().numpy() for r in st.read_windows(batch)]
        keys, used, n = list(st._cache), st._cache_used, st.stats["chunks_read"]
        assert torch.equal(st.assoc_sums(g, W, SAMPLES), a)
        assert list(st._cache) == keys and st._cache_used == used
        again = [r.cpu().numpy() for r in st.read_windows(batch)]
        assert st.stats["chunks_read"] == n                           # served from the cache: nothing read from the file
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        m = st.stats["count_compressed_bytes_read"]
        st.assoc_sums(g, W[:1], [3], v_lo=0, v_hi=100)                # cached chunks are used, not read again
        assert st.stats["count_compressed_bytes_read"] == m
        st.close()


# ---- a planted signal under population structure ----------------------------------------------------------------------------
PLANT_SEED, PLANTED = 8, 1234


def two_populations():
    """the cohort of test_first_component_splits_two_populations, a phenotype = population shift + 0.8 x the dosage of
    variant PLANTED + noise, and the variant whose allele frequencies differ most between the populations"""
    rng = np.random.default_rng(PLANT_SEED)
    n, V = 96, 4096
    pop = np.arange(n) % 2
    base = rng.random(V) * 0.6 + 0.2
    freq = np.stack([base, np.clip(base + rng.uniform(-0.3, 0.3, V), 0.02, 0.98)])
    G = (rng.random((n, V, 2)) < freq[pop][:, :, None]).astype(np.int8)
    G[rng.random((n, V, 2)) < 0.01] = -9
    y = 2.0 * pop + 0.8 * G[:, PLANTED].clip(0).sum(1) + rng.normal(size=n)
    return G, pop, y, int(np.argmax(np.abs(freq[0] - freq[1])))


def test_planted_variant_under_population_structure(ctx, tmp_path):
    """with PC1 as covariate the planted variant has the smallest P; the variant that differs most between the populations
    loses |T| when PC1 comes in.  (The seed was chosen so that the numpy reference, with the population label in the place
    of PC1, shows both.)"""
    from tests.test_gpu_ld import GROUP, write_store
    G, pop, y, stratified = two_populations()
    write_store(ctx, str(tmp_path / "pops.hhgt"), G, 64, 128)
    st = GenotypeStore(str(tmp_path / "pops.hhgt"), ctx=ctx)
    _, vecs = st.pca(1)
    with_pc, _ = st.assoc(GROUP, y, vecs)
    without, _ = st.assoc(GROUP, y)
    want = np_lstsq_scan(G, y, vecs)[0]
    assert rel_diff(with_pc.cpu().numpy(), want) <= STAT_RTOL
    p = with_pc[:, 0, ASSOC_P].cpu().numpy()
    assert np.nanargmin(p) == PLANTED and stratified != PLANTED
    assert abs(float(without[stratified, 0, ASSOC_T])) > abs(float(with_pc[stratified, 0, ASSOC_T]))
    st.close()


# ---- the reader and the CLI -----------------------------------------------------------------------------------------------
FIELDS = ("chrom", "pos", "ref", "alt", "n", "af", "beta", "se", "t", "p")


def same_records(a, b):
    """two record arrays of association(): every field equal, NaN equal to NaN"""
    return a.dtype == b.dtype and all(np.array_equal(a[f], b[f], equal_nan=a[f].dtype.kind == "f") for f in a.dtype.names)


def test_reader_and_cli(ctx, cohort):
    from click.testing import CliRunner
    from haplohyped_varawareml_amd.assoc import main
    from haplohyped_varawareml_amd.grm import main as grm_main
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    tmp, G = cohort["tmp"], cohort["bits"]
    g = f"chr_{CHROM3}"
    names = synth.sample_names(S3)
    many = np.arange(3, S3, 25)                                        # 40 donors
    donors = [names[i] for i in many]
    rng = np.random.default_rng(3)
    y = rng.normal(size=(len(many), 2)) + G[many, 4100].clip(0).sum(1)[:, None]
    cov = rng.normal(size=(len(many), 1))
    path = cohort["paths"][0]
    r = VCFH5Reader(path, ctx=ctx)
    st = r.store
    start, ref, alt, _ = st.variants(g)
    for kw in (dict(), dict(covariates=cov, min_maf=0.05, chromosomes=[CHROM3])):
        mask = st.variant_mask(g, donors, min_maf=kw["min_maf"]) if "min_maf" in kw else None
        stats, calls = (x.cpu().numpy() for x in st.assoc(g, y, kw.get("covariates"), donors, variant_mask=mask))
        at = np.arange(V3) if mask is None else np.flatnonzero(mask.cpu().numpy())
        recs = r.association(y, donor_ids=donors, **kw)
        assert len(recs) == 2 and all(rec.dtype.names == FIELDS and len(rec) == len(at) for rec in recs)
        for k, rec in enumerate(recs):
            assert np.array_equal(rec["pos"], start[at] + 1) and np.array_equal(rec["ref"], ref.view("S1")[at])
            assert np.array_equal(rec["alt"], alt.view("S1")[at]) and (rec["chrom"] == f"chr{CHROM3}".encode()).all()
            assert np.array_equal(rec["n"], calls[:, 0])
            assert np.array_equal(rec["af"], (calls[:, 1] + 2.0 * calls[:, 2]) / calls[:, 0] / 2.0, equal_nan=True)
            for c, f in enumerate(("beta", "se", "t", "p")):
                assert np.array_equal(rec[f], stats[:, k, c], equal_nan=True)
    one = r.association(y[:, 0], donor_ids=donors)
    assert len(one) == 1 and same_records(one[0], r.association(y, donor_ids=donors)[0])
    # pcs = 2 is principal_components(2) passed by hand, under the same variant choices; the scan uses the MAF mask only
    kw = dict(min_maf=0.05, ld_window=20, ld_r2=0.3)
    pcs, _ = r.principal_components(2, donor_ids=donors, **kw)
    by_hand = np.concatenate([cov, np.stack([pcs["pc1"], pcs["pc2"]], axis=1)], axis=1)
    a = r.association(y, cov, donor_ids=donors, pcs=2, **kw)
    b = r.association(y, by_hand, donor_ids=donors, min_maf=0.05)
    assert all(same_records(x, z) for x, z in zip(a, b)) and len(a[0]) == int(st.variant_mask(g, donors, min_maf=0.05).sum())
    with pytest.raises(KeyError):
        r.association(y, chromosomes=[6], donor_ids=donors)
    with pytest.raises(ValueError):
        r.association(y[:5], donor_ids=donors)
    # the CLI: the pheno file's samples in its order, the covar file in another; grm --pcs writes a valid --covar
    table = lambda who, cols, x: "#IID\t" + "\t".join(cols) + "\n" + "".join(
        d + "\t" + "\t".join("%.17g" % v for v in row) + "\n" for d, row in zip(who, x.tolist()))
    (tmp / "pheno.tsv").write_text(table(donors, ["height", "weight"], y))
    (tmp / "covar.tsv").write_text(table(donors[::-1], ["age"], cov[::-1]))
    out = str(tmp / "assoc.tsv")
    res = CliRunner().invoke(main, ["--h5", path, "--pheno", str(tmp / "pheno.tsv"), "--covar", str(tmp / "covar.tsv"),
                                    "--out", out, "--min_maf", "0.05", "--chromosome", str(CHROM3)])
    assert res.exit_code == 0, res.output
    want = r.association(y, cov, donor_ids=donors, min_maf=0.05)
    lines = open(out).read().splitlines()
    assert lines[0] == "#CHROM\tPOS\tREF\tALT\tPHENO\tN\tAF\tBETA\tSE\tT\tP" and len(lines) == 1 + 2 * len(want[0])
    cells = [ln.split("\t") for ln in lines[1:]]
    for k, name in enumerate(("height", "weight")):
        mine = cells[k::2]
        assert all(c[4] == name for c in mine)
        assert [c[0] for c in mine] == [x.decode() for x in want[k]["chrom"]]
        assert np.array_equal(np.array([int(c[1]) for c in mine]), want[k]["pos"])
        assert [c[2] for c in mine] == [x.decode() for x in want[k]["ref"]]
        assert np.array_equal(np.array([int(c[5]) for c in mine]), want[k]["n"])
        for col, f in zip(range(6, 11), ("af", "beta", "se", "t", "p")):
            assert np.array_equal(np.array([float(c[col]) for c in mine]), want[k][f], equal_nan=True)      # %.17g round-trips
    assert all(x == "nan" for c in cells for x in c[6:] if x.lower() == "nan")                             # nan is spelled nan
    (tmp / "assoc_samples.txt").write_text("\n".join(donors) + "\n")
    res = CliRunner().invoke(grm_main, ["--h5", path, "--out", str(tmp / "pc"), "--sample_list", str(tmp / "assoc_samples.txt"),
                                        "--min_maf", "0.05", "--pcs", "3"])
    assert res.exit_code == 0, res.output
    res = CliRunner().invoke(main, ["--h5", path, "--pheno", str(tmp / "pheno.tsv"), "--covar", str(tmp / "pc.eigenvec.tsv"),
                                    "--out", out, "--min_maf", "0.05"])
    assert res.exit_code == 0, res.output
    pcs, _ = r.principal_components(3, donor_ids=donors, min_maf=0.05)
    want = r.association(y, np.stack([pcs[f"pc{c + 1}"] for c in range(3)], axis=1), donor_ids=donors, min_maf=0.05)
    got = np.array([float(ln.split("\t")[10]) for ln in open(out).read().splitlines()[1::2]])
    assert np.array_equal(got, want[0]["p"], equal_nan=True)
    # a sample the cohort does not have, a NaN, a covar file of other samples: non-zero exits
    (tmp / "bad1.tsv").write_text(table(donors[:-1] + ["nobody"], ["height", "weight"], y))
    (tmp / "bad2.tsv").write_text(table(donors, ["height", "weight"], y).replace("%.17g" % y[3, 1], "nan"))
    (tmp / "bad3.tsv").write_text(table(donors[1:], ["age"], cov[1:]))
    for args in (["--pheno", str(tmp / "bad1.tsv")], ["--pheno", str(tmp / "bad2.tsv")],
                 ["--pheno", str(tmp / "pheno.tsv"), "--covar", str(tmp / "bad3.tsv")]):
        res = CliRunner().invoke(main, ["--h5", path, "--out", out] + args)
        assert res.exit_code != 0, args
    r.close()
