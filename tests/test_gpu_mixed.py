"""The mixed-model scan on the device: store_mixed.mixed_sums / assoc_mixed against the dense numpy reference
(store_stats.mixed_reference) on the generator's genotypes, across the store's paths, windows and masks; the reader and
the CLI."""
import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd import synth
from haplohyped_varawareml_amd.store import (ASSOC_BETA, MIXED_BETA, GenotypeStore, mixed_null, mixed_reference)
from haplohyped_varawareml_amd.store_mixed import assoc_mixed, mixed_sums
from tests.test_assoc_stats import STAT_RTOL, np_sums, rel_diff
from tests.test_gpu_allele_counts import CHROM3, S3, V3, cohort  # noqa: F401 (cohort: fixture)
from tests.test_gpu_sample_counts import np_variant_mask
from tests.test_mixed_stats import MIXED_RTOL

pytestmark = pytest.mark.gpu

GROUP = f"chr_{CHROM3}"
SAMPLES = np.random.default_rng(17).permutation(S3)[:150]        # distinct, out of order, every chunk row of 64
LO, HI = 8000, 8400                                              # crosses the chunk column at 8192 and Blosc blocks


def dosages(G):
    """int8 [n, V, 2] -> (dosage int64 [n, V], complete bool [n, V])"""
    ok = ((G == 0) | (G == 1)).all(axis=2)
    return np.where(ok, G.clip(0).sum(axis=2), 0), ok


@pytest.fixture(scope="module")
def inputs(cohort):
    """the samples' genotypes in the range, a quarter-valued W, a real symmetric A, and the dense reference of both"""
    rng = np.random.default_rng(23)
    G = cohort["bits"][SAMPLES, LO:HI]
    n = len(SAMPLES)
    W = rng.integers(-8, 9, (n, 3)) / 4.0
    W[:, 0] = 1.0
    A = rng.normal(size=(n, n))
    A = (A + A.T) / 2.0
    d, ok = dosages(G)
    ref = mixed_reference(d, ok, A, np.zeros(n))
    bound = ((np.abs(A) @ np.abs(ref["x"])) * np.abs(ref["x"])).sum(0)
    return dict(G=G, W=W, A=A, T=np_sums(G, W), q=ref["q"], bound=bound)


def test_mixed_sums(ctx, cohort, inputs):
    W, A = inputs["W"], inputs["A"]
    first = None
    for n_path, path in enumerate(cohort["paths"]):
        st = GenotypeStore(path, ctx=ctx)
        sw = -(-st._plane_rows(SAMPLES)[0] // 32)
        T, q = mixed_sums(st, GROUP, A, W, SAMPLES, LO, HI)
        assert T.is_cuda and q.is_cuda and T.dtype == q.dtype == torch.float64
        assert tuple(T.shape) == (HI - LO, 3, 3) and tuple(q.shape) == (HI - LO,)
        assert np.array_equal(T.cpu().numpy(), inputs["T"])                     # quarters: exact
        err, bound = np.abs(q.cpu().numpy() - inputs["q"]), 32 * sw * 2.0 ** -51 * inputs["bound"]
        print(f"mixed_sums {path.rsplit('.', 1)[-1]}: n = {32 * sw}, largest error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
        assert (err <= bound).all()
        if first is None:
            first = (T, q)
        assert torch.equal(T.view(torch.int64), first[0].view(torch.int64)) and torch.equal(q.view(torch.int64), first[1].view(torch.int64))
        # windows, slabs, device tensors for A and W: the same bits; the stat keys move as assoc_sums moves them
        for kw in (dict(plane_bytes=1), dict(slab_bytes=300_000), dict()):
            st.stats.update(assoc_plane_blocks=0, assoc_variants=0)
            Tk, qk = mixed_sums(st, GROUP, torch.from_numpy(A).to(ctx.device), torch.from_numpy(W).to(ctx.device), SAMPLES, LO, HI, **kw)
            assert torch.equal(Tk.view(torch.int64), T.view(torch.int64)) and torch.equal(qk.view(torch.int64), q.view(torch.int64)), kw
            moved = (st.stats["assoc_plane_blocks"], st.stats["assoc_variants"])
            st.stats.update(assoc_plane_blocks=0, assoc_variants=0)
            st.assoc_sums(GROUP, W, SAMPLES, LO, HI, **kw)
            assert moved == (st.stats["assoc_plane_blocks"], st.stats["assoc_variants"]) and moved[1] == HI - LO and moved[0] > 0
        # a variant mask, on the device and on the host: the rows it marks
        vm = st.variant_mask(GROUP, SAMPLES, LO, HI, min_maf=0.1)
        keep = np_variant_mask(inputs["G"], min_maf=0.1)
        assert 0 < keep.sum() < len(keep)
        at = torch.from_numpy(np.flatnonzero(keep)).to(ctx.device)
        for mask in (vm, keep):
            Tm, qm = mixed_sums(st, GROUP, A, W, SAMPLES, LO, HI, variant_mask=mask)
            assert torch.equal(Tm.view(torch.int64), T[at].view(torch.int64)) and torch.equal(qm.view(torch.int64), q[at].view(torch.int64))
        if n_path == 0:
            # no counted variant; refusals: W without its ones, A not symmetric or of another shape or type
            T0, q0 = mixed_sums(st, GROUP, A, W, SAMPLES, 7, 7)
            assert tuple(T0.shape) == (0, 3, 3) and tuple(q0.shape) == (0,)
            skew = A.copy()
            skew[3, 5] += 1e-9
            for a, w in ((A, W[:, 1:]), (skew, W), (A[:-1], W), (A.astype(np.float32), W), (A, W[:-1]), (A, np.ones((len(SAMPLES), 65)))):
                with pytest.raises(ValueError, match="mixed_sums"):
                    mixed_sums(st, GROUP, a, w, SAMPLES, LO, HI)
            with pytest.raises(ValueError, match="max_table_bytes"):
                mixed_sums(st, GROUP, A, W, SAMPLES, LO, HI, max_table_bytes=8 * (32 * sw) ** 2 - 1)
            with pytest.raises(KeyError):
                mixed_sums(st, "chr_6", A, W, SAMPLES)
        st.close()


def test_mixed_sums_leaves_read_cache_alone(ctx, cohort, inputs):
    st = GenotypeStore(cohort["paths"][0], ctx=ctx)
    batch = [(GROUP, s, 8000, 8300) for s in (3, 70, 500)]
    first = [r.cpu().numpy() for r in st.read_windows(batch)]
    keys, used = list(st._cache), st._cache_used
    mixed_sums(st, GROUP, inputs["A"], inputs["W"], SAMPLES, LO, HI)
    assert list(st._cache) == keys and st._cache_used == used
    assert all(np.array_equal(x, y.cpu().numpy()) for x, y in zip(first, st.read_windows(batch)))
    st.close()


def phenotype(G, n_pheno=2, seed=29):
    rng = np.random.default_rng(seed)
    cov = rng.normal(size=(G.shape[0], 2))
    y = rng.normal(size=(G.shape[0], n_pheno)) + cov[:, :1] + 0.5 * G[:, 100].clip(0).sum(1)[:, None]
    return y, cov


def test_assoc_mixed(ctx, cohort, inputs):
    G = inputs["G"]
    n = len(SAMPLES)
    y, cov = phenotype(G)
    d, ok = dosages(G)
    st = GenotypeStore(cohort["paths"][0], ctx=ctx)
    K = st.grm(GROUP, SAMPLES, 0, 4096)                              # a device tensor: the relatedness over other variants
    stats, calls, nulls = assoc_mixed(st, GROUP, y, K, cov, SAMPLES, LO, HI)
    assert stats.is_cuda and stats.dtype == torch.float64 and tuple(stats.shape) == (HI - LO, 2, 4)
    assert calls.dtype == torch.int64 and len(nulls) == 2 and all(sorted(x) == ["h2", "q", "sigma2"] for x in nulls)
    for p in range(2):
        null = mixed_null(K.cpu().numpy(), y[:, p], cov)
        assert (nulls[p]["h2"], nulls[p]["sigma2"], nulls[p]["q"]) == (null["h2"], null["sigma2"], 3)
        ref = mixed_reference(d, ok, null["M"], y[:, p])
        assert np.array_equal(calls.cpu().numpy(), ref["calls"])
        diff = rel_diff(stats[:, p].cpu().numpy(), ref["stats"])
        print(f"assoc_mixed, phenotype {p}: h2 = {null['h2']:.4f}, largest relative difference {diff:.3g}, "
              f"{int(np.isnan(ref['stats'][:, 0]).sum())} untested")
        assert diff <= MIXED_RTOL and np.isnan(ref["stats"][:, 0]).sum() < (HI - LO) // 2
    one = assoc_mixed(st, GROUP, y[:, 0], K.cpu().numpy(), cov, SAMPLES, LO, HI)
    assert torch.equal(one[0].view(torch.int64), stats[:, :1].view(torch.int64)) and torch.equal(one[1], calls)
    # K = I is ordinary least squares: the new kernel against the existing device route
    eye, _, _ = assoc_mixed(st, GROUP, y, np.eye(n), cov, SAMPLES, LO, HI)
    ols, ols_calls = st.assoc(GROUP, y, cov, SAMPLES, LO, HI)
    assert torch.equal(ols_calls, calls)
    got, want = eye[:, :, MIXED_BETA].cpu().numpy(), ols[:, :, ASSOC_BETA].cpu().numpy()
    tested = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~tested) and tested.sum() > (HI - LO)
    diff = float((np.abs(got - want)[tested] / np.abs(want)[tested]).max())
    print(f"assoc_mixed with K = I against assoc: largest relative difference of BETA {diff:.3g}")
    assert diff <= STAT_RTOL
    # refusals: a sample twice (before anything is allocated), a relationship matrix with a NaN, a matrix over budget
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(ctx.device)
    before = torch.cuda.max_memory_allocated(ctx.device)
    twice = list(SAMPLES[:5]) + [int(SAMPLES[0])]
    with pytest.raises(ValueError, match="twice"):
        assoc_mixed(st, GROUP, np.arange(6.0), np.eye(6), None, twice, LO, HI)
    with pytest.raises(ValueError, match="twice"):
        mixed_sums(st, GROUP, np.eye(6), np.ones((6, 1)), twice, LO, HI)
    assert torch.cuda.max_memory_allocated(ctx.device) == before
    bad = np.eye(n)
    bad[4, 9] = bad[9, 4] = np.nan
    with pytest.raises(ValueError, match="finite"):
        assoc_mixed(st, GROUP, y, bad, cov, SAMPLES, LO, HI)
    with pytest.raises(ValueError, match="max_table_bytes"):
        assoc_mixed(st, GROUP, y, np.eye(n), cov, SAMPLES, LO, HI, max_table_bytes=1000)
    with pytest.raises(ValueError):
        assoc_mixed(st, GROUP, y[:-1], np.eye(n), cov, SAMPLES, LO, HI)
    st.close()


def test_reader_and_cli(ctx, cohort):
    from click.testing import CliRunner
    from haplohyped_varawareml_amd.assoc import scan
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    tmp, G = cohort["tmp"], cohort["bits"]
    names = synth.sample_names(S3)
    many = np.arange(3, S3, 25)                                        # 40 donors
    donors = [names[i] for i in many]
    y, cov = phenotype(G[many][:, 4000:4200], seed=31)
    path = cohort["paths"][0]
    r = VCFH5Reader(path, ctx=ctx)
    st = r.store
    kw = dict(min_maf=0.2, grm_min_maf=0.05, ld_window=20, ld_r2=0.3)
    recs, nulls = r.mixed_association(y, cov, donor_ids=donors, **kw)
    _, K, _ = r.genetic_relationship(donor_ids=donors, min_maf=0.05, ld_window=20, ld_r2=0.3)
    mask = st.variant_mask(GROUP, donors, min_maf=0.2)
    stats, calls, fitted = assoc_mixed(st, GROUP, y, K, cov, donors, variant_mask=mask)
    stats, calls = stats.cpu().numpy(), calls.cpu().numpy()
    at = np.flatnonzero(mask.cpu().numpy())
    start, ref, alt, _ = st.variants(GROUP)
    assert len(recs) == len(nulls) == 2 and 0 < len(at) < V3
    for k, rec in enumerate(recs):
        assert rec.dtype.names == ("chrom", "pos", "ref", "alt", "n", "af", "beta", "se", "z", "p") and len(rec) == len(at)
        assert np.array_equal(rec["pos"], start[at] + 1) and (rec["chrom"] == f"chr{CHROM3}".encode()).all()
        assert np.array_equal(rec["ref"], ref.view("S1")[at]) and np.array_equal(rec["alt"], alt.view("S1")[at])
        assert np.array_equal(rec["n"], calls[:, 0])
        assert np.array_equal(rec["af"], (calls[:, 1] + 2.0 * calls[:, 2]) / calls[:, 0] / 2.0, equal_nan=True)
        for c, f in enumerate(("beta", "se", "z", "p")):
            assert np.array_equal(rec[f], stats[:, k, c], equal_nan=True)
        assert len(nulls[k]) == 1 and nulls[k]["chrom"][0] == b"*"
        assert (nulls[k]["h2"][0], nulls[k]["sigma2"][0]) == (fitted[k]["h2"], fitted[k]["sigma2"])
    with pytest.raises(ValueError, match="only group"):
        r.mixed_association(y, cov, donor_ids=donors, loco=True, **kw)
    # the CLI writes those records; --test and --case_control_12 belong to the logistic model
    table = lambda who, cols, x: "#IID\t" + "\t".join(cols) + "\n" + "".join(
        d + "\t" + "\t".join("%.17g" % v for v in row) + "\n" for d, row in zip(who, x.tolist()))
    (tmp / "mixed_pheno.tsv").write_text(table(donors, ["height", "weight"], y))
    (tmp / "mixed_covar.tsv").write_text(table(donors[::-1], ["age", "bmi"], cov[::-1]))
    out = str(tmp / "mixed.tsv")
    args = ["--h5", path, "--pheno", str(tmp / "mixed_pheno.tsv"), "--covar", str(tmp / "mixed_covar.tsv"), "--out", out,
            "--model", "mixed", "--min_maf", "0.2", "--grm_min_maf", "0.05", "--ld_window", "20", "--ld_r2", "0.3"]
    res = CliRunner().invoke(scan, args)
    assert res.exit_code == 0, res.output
    lines = open(out).read().splitlines()
    assert lines[0] == "#CHROM\tPOS\tREF\tALT\tPHENO\tN\tAF\tBETA\tSE\tZ\tP" and len(lines) == 1 + 2 * len(at)
    cells = [ln.split("\t") for ln in lines[1:]]
    for k, name in enumerate(("height", "weight")):
        mine = cells[k::2]
        assert all(c[4] == name for c in mine)
        assert np.array_equal(np.array([int(c[1]) for c in mine]), recs[k]["pos"])
        assert np.array_equal(np.array([int(c[5]) for c in mine]), recs[k]["n"])
        for col, f in zip(range(6, 11), ("af", "beta", "se", "z", "p")):
            assert np.array_equal(np.array([float(c[col]) for c in mine]), recs[k][f], equal_nan=True)      # %.17g round-trips
    for extra in (["--test", "score"], ["--case_control_12"], ["--pcs", "2"], ["--loco"]):
        res = CliRunner().invoke(scan, args + extra)
        assert res.exit_code != 0, extra
    res = CliRunner().invoke(scan, args[:8] + ["--loco"])             # --loco without --model mixed
    assert res.exit_code != 0
    r.close()
