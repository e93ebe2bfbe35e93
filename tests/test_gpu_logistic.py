"""hhgt_logistic_fit (a wave's Newton iteration over variant-major planes) against store_stats.logistic_fit_reference and,
for its first evaluation, against hhgt_assoc_sums; GenotypeStore.assoc_logistic against the reference on the generator's
genotypes; a planted signal under population structure; the reader and the CLI."""
import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd import synth
from haplohyped_varawareml_amd._lib import HhgtError
from haplohyped_varawareml_amd.store import (LOGIT_BETA, LOGIT_COLLINEAR, LOGIT_NO_CALL, LOGIT_NOT_CONVERGED, LOGIT_ONE_CLASS,
                                             LOGIT_P, LOGIT_REC, LOGIT_SCORE_CHI2, LOGIT_SCORE_P, LOGIT_SE, LOGIT_TESTED, LOGIT_Z,
                                             GenotypeStore, logistic_design, logistic_fit_reference, logistic_from_fit,
                                             logistic_score_design, logistic_score_from_sums, normal_two_sided)
from tests.test_gpu_allele_counts import CHROM3, S3, V3, cohort  # noqa: F401 (cohort: fixture)
from tests.test_gpu_assoc import SAMPLES, guarded, two_populations
from tests.test_gpu_sample_counts import np_variant_mask
from tests.test_logistic_stats import LOGIT_RTOL, SCORE_RTOL, dosages, score_diff, separated, wald_diff

pytestmark = pytest.mark.gpu


def agree(got, want, who):
    """(stats, calls, info) of the device against the reference's: the calls, the status and with it the NaN pattern
    exactly; BETA and SE within LOGIT_RTOL, the score chi^2 within SCORE_RTOL (tests/test_logistic_stats.py derives both on
    the CPU), Z and the two P by their formulas; the steps of a fitted variant within one — the step that brings max |delta|
    just under or just over 1e-8 may fall on either side, and the evaluation after the last step makes that a difference of
    second order: it is BETA and SE that are held to the tolerance"""
    stats, calls, info = (x.cpu().numpy() if torch.is_tensor(x) else x for x in got)
    assert np.array_equal(calls, want[1]), who
    assert np.array_equal(info[..., 1], want[2][..., 1]), who
    assert np.array_equal(np.isnan(stats), np.isnan(want[0])), who
    tested = want[2][..., 1] == LOGIT_TESTED
    unfit = ~tested & (want[2][..., 1] != LOGIT_NOT_CONVERGED)
    assert (np.abs(info[..., 0] - want[2][..., 0])[tested] <= 1).all() and not info[..., 0][unfit].any(), who
    s, w = stats.reshape(-1, 6), want[0].reshape(-1, 6)
    dw, ds = wald_diff(s, w), score_diff(s, w)
    print(f"{who}: BETA / SE differ from the reference by {dw:.3g} (allowed {LOGIT_RTOL:.3g}), the score chi^2 by {ds:.3g} "
          f"(allowed {SCORE_RTOL:.3g}); {int(tested.sum())} of {tested.size} fitted, steps {np.bincount(info[..., 0][tested]).tolist()}")
    assert dw <= LOGIT_RTOL and ds <= SCORE_RTOL, who
    # Z and the two P are read from these by logistic_from_fit's formulas
    fit = ~np.isnan(s[:, LOGIT_BETA])
    assert np.array_equal(s[fit, LOGIT_Z], s[fit, LOGIT_BETA] / s[fit, LOGIT_SE]), who
    assert np.allclose(s[fit, LOGIT_P], normal_two_sided(s[fit, LOGIT_Z]), rtol=1e-12, atol=0), who
    assert np.allclose(s[fit, LOGIT_SCORE_P], normal_two_sided(np.sqrt(s[fit, LOGIT_SCORE_CHI2])), rtol=1e-12, atol=0), who


# ---- the kernel ------------------------------------------------------------------------------------------------------------
N_VAR = 130


def kernel_case(sw, q, seed=0):
    """one launch's worth of inputs on 32 sw positions -> dict: the listed samples are the positions that d_valid marks — a
    scattered tenth left out, and the whole last word where there are several —; genotypes [n, N_VAR, 2] with 2 % missing
    alleles; variant 0 monomorphic, 1 without a call, 2 the last column of the covariates (q >= 2: collinear), 3 and 4
    separated (a dosage above 0 exactly in the cases: their waves run all 25 steps beside waves that stop after 3), 5 with
    a planted effect, the rest null.  The planes are packed from the genotypes, and the positions that are not listed carry
    bits of their own in the planes and NaN in X and y: nothing of them may be read."""
    rng = np.random.default_rng(1000 * sw + 10 * q + seed)
    n_pos = 32 * sw
    listed = rng.random(n_pos) < 0.9
    if sw > 1:
        listed[-32:] = False
    pos = np.flatnonzero(listed)
    n = len(pos)
    G = (rng.random((n, N_VAR, 2)) < rng.uniform(0.1, 0.9, N_VAR)[None, :, None]).astype(np.int8)
    G[rng.random((n, N_VAR, 2)) < 0.02] = -9
    G[:, 0], G[:, 1] = 1, -9
    G[:, 2] = (rng.random((n, 2)) < 0.4).astype(np.int8)
    cov = rng.normal(size=(n, q - 1)) * 3 + 1
    if q >= 2:
        cov[:, -1] = G[:, 2].sum(1)
    eta = 0.8 * G[:, 5].clip(0).sum(1) + (0.7 * (cov[:, 0] - 1) / 3 if q >= 3 else 0.0) - 0.6
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    y[:2] = 0.0, 1.0
    S = separated(y, rng, 2)
    G[:, 3:5] = np.stack([S >= 1, S >= 2], axis=2).transpose(1, 0, 2)
    X, beta0 = logistic_design(y, cov)
    all_G = rng.integers(-1, 2, (n_pos, N_VAR, 2)).astype(np.int8)                 # what the unlisted positions hold
    all_G[pos] = G
    ok = ((all_G == 0) | (all_G == 1)).all(axis=2)
    classes = (ok & (all_G[..., 0] != all_G[..., 1]), ok, ok & (all_G.sum(axis=2) == 2))
    planes = np.stack([np.ascontiguousarray(np.packbits(c.T, axis=1, bitorder="little")).view(np.uint32) for c in classes])
    valid = np.packbits(listed, bitorder="little").view(np.uint32)
    full_X, full_y = np.full((n_pos, q), np.nan), np.full(n_pos, np.nan)
    full_X[pos], full_y[pos] = X, y
    rec = logistic_fit_reference(dosages(G), X, y, beta0)
    return dict(G=G, X=X, y=y, beta0=beta0, pos=pos, planes=planes, valid=valid, full_X=full_X, full_y=full_y, rec=rec,
                want=logistic_from_fit(rec))


def on_device(ctx, c, n_var=N_VAR):
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(ctx.device)
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)
    return i32(c["planes"][:, :n_var]), i32(c["valid"]), f64(c["full_X"]), f64(c["full_y"]), f64(c["beta0"])


# 14 columns of X and the dosage are 15 coefficients: they take the 200 samples of 8 words to be fitted at all, so q = 14
# goes with sw = 8 and 79 and the narrow designs with every sw
@pytest.mark.parametrize("sw, q", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2), (8, 1), (8, 2), (8, 14), (79, 1), (79, 2),
                                   (79, 14)])
def test_kernel_matches_reference(ctx, sw, q):
    c = kernel_case(sw, q)
    status = c["want"][2][:, 1]
    # the launch holds what it is meant to hold: every kind of variant, short fits and the longest the reference reports
    assert status[0] == LOGIT_ONE_CLASS and status[1] == LOGIT_NO_CALL and (status[3:5] == LOGIT_NOT_CONVERGED).all()
    assert status[2] == (LOGIT_COLLINEAR if q >= 2 else LOGIT_TESTED)
    steps = c["want"][2][status == LOGIT_TESTED, 0]
    assert (status == LOGIT_TESTED).sum() >= 100 and steps.min() <= 4 and steps.max() >= 5
    args = on_device(ctx, c)
    raw = ctx.logistic_fit(*args)
    assert raw.is_cuda and raw.dtype == torch.float64 and tuple(raw.shape) == (N_VAR, LOGIT_REC)
    agree(logistic_from_fit(raw), c["want"], f"logistic_fit sw={sw} q={q}")
    host = raw.cpu().numpy()
    for n_var in (1, 7, 8, 9, 16, 17, 63, 64, 65, N_VAR):          # (a workgroup has 8 waves and 64 variants)
        # fewer variants: the same records, bit for bit (a variant is a wave's own, whoever shares its workgroup), into the
        # caller's tensor with nothing beside it touched; and the same bits on a second call
        buf, view = guarded(ctx, (n_var, LOGIT_REC))
        sub = on_device(ctx, c, n_var)
        assert ctx.logistic_fit(*sub, out=view) is view
        whole = buf.cpu().numpy()
        assert np.isnan(whole[:1024]).all() and np.isnan(whole[-1024:]).all()
        assert np.array_equal(whole[1024:-1024].view(np.uint64), host[:n_var].reshape(-1).view(np.uint64)), n_var
    assert torch.equal(ctx.logistic_fit(*args).view(torch.int64), raw.view(torch.int64))


@pytest.mark.parametrize("sw, q", [(3, 2), (8, 14), (79, 2)])
def test_first_evaluation_matches_assoc_sums(ctx, sw, q):
    """LOGIT_SCORE_CHI2 by two device routes that share no code: hhgt_logistic_fit's first evaluation, and hhgt_assoc_sums
    over [1 | y - mu0 | w0 | w0 X] read by logistic_score_from_sums"""
    c = kernel_case(sw, q, seed=1)
    planes, valid, _, _, _ = on_device(ctx, c)
    fit = logistic_from_fit(ctx.logistic_fit(*on_device(ctx, c)))
    W, XWX = logistic_score_design(c["X"], c["y"], c["beta0"])
    full_W = np.zeros((32 * sw, W.shape[1]))
    full_W[c["pos"]] = W
    T = ctx.assoc_sums(planes, torch.from_numpy(full_W).to(ctx.device))
    stats, calls, info = logistic_score_from_sums(T, torch.from_numpy(W.sum(axis=0)).to(ctx.device), q,
                                                  torch.from_numpy(XWX).to(ctx.device))
    assert torch.equal(calls, fit[1])
    # (a separated variant has a score test but no fit: compared where the fit stands)
    status, fitted = info[:, 1].cpu().numpy(), (fit[2][:, 1] == LOGIT_TESTED).cpu().numpy()
    assert status[0] == LOGIT_ONE_CLASS and status[1] == LOGIT_NO_CALL and status[2] == LOGIT_COLLINEAR
    assert (status[3:5] == LOGIT_TESTED).all() and (status[fitted] == LOGIT_TESTED).all() and not info[:, 0].any()
    d = score_diff(stats.cpu().numpy()[fitted], fit[0].cpu().numpy()[fitted])
    print(f"score chi^2, sw={sw} q={q}: hhgt_logistic_fit and hhgt_assoc_sums differ by {d:.3g} (allowed {2 * SCORE_RTOL:.3g})")
    assert d <= 2 * SCORE_RTOL                                          # (each route within SCORE_RTOL of the reference)
    assert fitted.sum() >= 100


def test_kernel_arguments(ctx):
    dev = ctx.device
    planes = torch.zeros((3, 5, 2), dtype=torch.int32, device=dev)
    planes[1] = -1                                                     # every call complete and HOM_REF
    valid = torch.full((2,), -1, dtype=torch.int32, device=dev)
    X = torch.ones((64, 3), dtype=torch.float64, device=dev)
    y = torch.zeros(64, dtype=torch.float64, device=dev)
    beta0 = torch.zeros(3, dtype=torch.float64, device=dev)
    good = dict(vplanes=planes, valid=valid, X=X, y=y, beta0=beta0)
    raw = ctx.logistic_fit(**good)
    assert tuple(raw.shape) == (5, LOGIT_REC) and (raw[:, 5] == LOGIT_ONE_CLASS).all() and (raw[:, 6] == 64).all()
    for q in (0, 15):
        with pytest.raises(HhgtError, match="columns"):
            ctx.logistic_fit(planes, valid, torch.ones((64, q), dtype=torch.float64, device=dev), y,
                             torch.zeros(q, dtype=torch.float64, device=dev))
    ctx.logistic_fit(planes, valid, torch.ones((64, 14), dtype=torch.float64, device=dev), y,
                     torch.zeros(14, dtype=torch.float64, device=dev))
    for kw in (dict(X=X.float()), dict(X=X[:63]), dict(X=X.cpu()), dict(X=torch.ones((64, 6), dtype=torch.float64, device=dev)[:, ::2]),
               dict(X=X[:, 0]), dict(y=y.float()), dict(y=y[:63]), dict(y=y.cpu()), dict(y=torch.zeros(128, dtype=torch.float64, device=dev)[::2]),
               dict(beta0=beta0.float()), dict(beta0=beta0[:2]), dict(beta0=beta0.cpu()),
               dict(valid=valid.float()), dict(valid=valid[:1]), dict(valid=valid.cpu()), dict(valid=valid.to(torch.int64)),
               dict(vplanes=planes.float()), dict(vplanes=planes[:2]), dict(vplanes=planes[:, :, :1]),
               dict(out=torch.zeros((5, LOGIT_REC), dtype=torch.float32, device=dev)),
               dict(out=torch.zeros((5, LOGIT_REC + 1), dtype=torch.float64, device=dev)),
               dict(out=torch.zeros((5, 2 * LOGIT_REC), dtype=torch.float64, device=dev)[:, ::2])):
        with pytest.raises(ValueError):
            ctx.logistic_fit(**{**good, **kw})
    # no variant: an empty result; no sample word: no call anywhere
    assert tuple(ctx.logistic_fit(planes[:, :0].contiguous(), valid, X, y, beta0).shape) == (0, LOGIT_REC)
    none = ctx.logistic_fit(torch.zeros((3, 5, 0), dtype=torch.int32, device=dev), valid[:0], X[:0], y[:0], beta0,
                            out=torch.full((5, LOGIT_REC), 7.0, dtype=torch.float64, device=dev)).cpu().numpy()
    assert np.isnan(none[:, :4]).all() and (none[:, 4] == 0).all() and (none[:, 5] == LOGIT_NO_CALL).all() and not none[:, 6:].any()


# ---- the store -------------------------------------------------------------------------------------------------------------
RANGES = [(4000, 4600), (4095, 4097), (4000, 9000)]                     # each cuts a block of 4096 variants; the last, windows


@pytest.fixture(scope="module")
def scan(cohort):
    """200 samples of the cohort, out of order across its chunk rows of 64, two covariates, two phenotypes with a planted
    variant, and per range of variants the reference on the generator's genotypes (computed once, never changed)"""
    G = cohort["bits"]
    rng = np.random.default_rng(11)
    many = rng.permutation(np.arange(3, S3, 5))
    cov = rng.normal(size=(len(many), 2)) * [1.0, 40.0] + [0.0, 170.0]
    eta = 0.9 * G[many, 4100].clip(0).sum(1)[:, None] + 0.6 * cov[:, :1] - [0.8, 1.3]
    y = (rng.random((len(many), 2)) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    designs = [logistic_design(y[:, p], cov) for p in range(2)]

    def reference(a, b, keep=None):
        D = dosages(G[many, a:b] if keep is None else G[many, a:b][:, keep])
        out = [logistic_from_fit(logistic_fit_reference(D, X, y[:, p], beta0)) for p, (X, beta0) in enumerate(designs)]
        return np.stack([o[0] for o in out], 1), out[0][1], np.stack([o[2] for o in out], 1)

    return dict(many=many, cov=cov, y=y, reference=reference, want={r: reference(*r) for r in RANGES})


def test_store_assoc_logistic(ctx, cohort, scan):
    g, G = f"chr_{CHROM3}", cohort["bits"]
    names = synth.sample_names(S3)
    many, cov, y = scan["many"], scan["cov"], scan["y"]
    for n_path, path in enumerate(cohort["paths"]):
        st = GenotypeStore(path, ctx=ctx)
        for k, (a, b) in enumerate(RANGES[:2]):
            got = st.assoc_logistic(g, y if k else torch.from_numpy(y).to(ctx.device), cov, [names[i] for i in many] if k else many, a, b)
            assert all(x.is_cuda for x in got) and [x.dtype for x in got] == [torch.float64, torch.int64, torch.int64]
            assert [tuple(x.shape) for x in got] == [(b - a, 2, 6), (b - a, 3), (b - a, 2, 2)]
            agree(got, scan["want"][a, b], f"assoc_logistic {path[-12:]} [{a}, {b})")
        for test in ("wald", "score"):                                 # no variant: empty tables
            assert [tuple(x.shape) for x in st.assoc_logistic(g, y, cov, many, 7, 7, test=test)] == [(0, 2, 6), (0, 3), (0, 2, 2)]
        # windows and slabs: the same bits as one window gives, and the reference's numbers
        a, b = RANGES[2]
        st.stats.update(logistic_variants=0, assoc_variants=0)
        whole = st.assoc_logistic(g, y, cov, many, a, b)
        assert st.stats["logistic_variants"] == 2 * (b - a) and st.stats["assoc_variants"] == 0
        agree(whole, scan["want"][a, b], f"assoc_logistic {path[-12:]} [{a}, {b})")
        p_min = np.nanargmin(whole[0][:, 1, LOGIT_P].cpu().numpy())
        assert p_min == 4100 - a and float(whole[0][p_min, 1, LOGIT_P]) < 1e-3           # the planted variant (the reference: 5.6e-4)
        for kw in (dict(plane_bytes=1), dict(slab_bytes=300_000)):
            again = st.assoc_logistic(g, y, cov, many, a, b, **kw)
            assert all(torch.equal(u.view(torch.int64), v.view(torch.int64)) for u, v in zip(again, whole)), kw
        # two phenotypes are two calls
        for p in range(2):
            one = st.assoc_logistic(g, y[:, p], cov, many, a, b)
            assert tuple(one[0].shape) == (b - a, 1, 6) and torch.equal(one[1], whole[1])
            assert torch.equal(one[0][:, 0].view(torch.int64), whole[0][:, p].view(torch.int64)) and torch.equal(one[2][:, 0], whole[2][:, p])
        # a variant class as a device tensor and as a host array, and the output of ld_prune
        vm = st.variant_mask(g, many, a, b, min_maf=0.1)
        keep = np_variant_mask(G[many, a:b], min_maf=0.1)
        assert 0 < keep.sum() < len(keep)
        masked = [st.assoc_logistic(g, y, cov, many, a, b, variant_mask=m) for m in (vm, keep)]
        for got in masked:
            assert all(torch.equal(u.view(torch.int64), v[torch.from_numpy(keep).to(ctx.device)].view(torch.int64))
                       for u, v in zip(got, whole))
        if n_path == 0:
            kept = st.ld_prune(g, many, a, b, variant_mask=vm, window=20, r2=0.01)
            assert 0 < int(kept.sum()) < keep.sum()
            agree(st.assoc_logistic(g, y, cov, many, a, b, variant_mask=kept), scan["reference"](a, b, kept.cpu().numpy()),
                  "assoc_logistic under ld_prune's mask")
        # the score test alone: hhgt_assoc_sums and logistic_score_from_sums — the reference's score columns, no Wald column
        stats, calls, info = (x.cpu().numpy() for x in st.assoc_logistic(g, y, cov, many, a, b, test="score"))
        want = scan["want"][a, b]
        assert np.array_equal(calls, want[1]) and np.isnan(stats[..., :LOGIT_SCORE_CHI2]).all() and not info[..., 0].any()
        fitted = want[2][..., 1] == LOGIT_TESTED
        assert (info[..., 1][fitted] == LOGIT_TESTED).all() and np.array_equal(info[..., 1] > LOGIT_TESTED, np.isnan(stats[..., LOGIT_SCORE_CHI2]))
        d = score_diff(stats[fitted], want[0][fitted])
        print(f"assoc_logistic test=score {path[-12:]}: the chi^2 differs from the reference by {d:.3g} (allowed {SCORE_RTOL:.3g})")
        assert d <= SCORE_RTOL
        # refusals: a sample twice (before anything is allocated), a phenotype that is not 0 / 1, shapes, names
        torch.cuda.reset_peak_memory_stats(ctx.device)
        before = torch.cuda.max_memory_allocated(ctx.device)
        with pytest.raises(ValueError, match="twice"):
            st.assoc_logistic(g, np.array([0.0, 1, 0, 1, 1]), None, [names[5], 70, 3, 5, 9])
        assert torch.cuda.max_memory_allocated(ctx.device) == before
        for bad in (dict(y=y + 1), dict(y=y * 0.5), dict(y=y[:-1]), dict(y=np.zeros(len(many))), dict(test="lrt"),
                    dict(covariates=cov[:-1]), dict(covariates=np.concatenate([cov] * 7, axis=1)),
                    dict(variant_mask=keep[:100])):
            with pytest.raises(ValueError):
                st.assoc_logistic(**{**dict(group=g, y=y, covariates=cov, samples=many, v_lo=a, v_hi=b), **bad})
        with pytest.raises(KeyError):
            st.assoc_logistic("chr_6", y, cov, many)
        st.close()


def test_store_assoc_logistic_leaves_read_cache_alone(ctx, cohort, scan):
    g = f"chr_{CHROM3}"
    many, cov, y = scan["many"][:40], scan["cov"][:40, :1], scan["y"][:40, 0]
    for path in cohort["paths"][:2]:
        st = GenotypeStore(path, ctx=ctx)
        batch = [(g, s, 1000 * s % 15000, 1000 * s % 15000 + 3000) for s in (3, 70, 500, 999)]
        first = [r.cpu().numpy() for r in st.read_windows(batch)]
        keys, used, n = list(st._cache), st._cache_used, st.stats["chunks_read"]
        for test in ("wald", "score"):
            st.assoc_logistic(g, y, cov, many, 0, 9000, test=test)
            assert list(st._cache) == keys and st._cache_used == used
        again = [r.cpu().numpy() for r in st.read_windows(batch)]
        assert st.stats["chunks_read"] == n                           # served from the cache: nothing read from the file
        assert all(np.array_equal(u, v) for u, v in zip(first, again))
        st.close()


# ---- a planted signal under population structure ----------------------------------------------------------------------------
PLANT_SEED, PLANTED = 7, 1234


def case_control_populations():
    """the two-population cohort of test_gpu_assoc.two_populations, and a 0 / 1 phenotype drawn from the population shift
    plus the dosage of variant PLANTED"""
    G, pop, _, stratified = two_populations()
    rng = np.random.default_rng(PLANT_SEED)
    eta = 2.0 * pop + 2.0 * G[:, PLANTED].clip(0).sum(1) - 1.0 - 2.0 * G[:, PLANTED].clip(0).sum(1).mean()
    return G, pop, (rng.random(len(pop)) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64), stratified


def test_planted_variant_under_population_structure(ctx, tmp_path):
    """with PC1 as covariate the planted variant has the smallest Wald P.  (PLANT_SEED was chosen on the CPU so that the numpy
    reference, with the population label in the place of PC1, shows this.)"""
    from tests.test_gpu_ld import GROUP, write_store
    G, pop, y, stratified = case_control_populations()
    write_store(ctx, str(tmp_path / "pops.hhgt"), G, 64, 128)
    st = GenotypeStore(str(tmp_path / "pops.hhgt"), ctx=ctx)
    _, vecs = st.pca(1)
    got = st.assoc_logistic(GROUP, y, vecs)
    X, beta0 = logistic_design(y, vecs)
    want = logistic_from_fit(logistic_fit_reference(dosages(G), X, y, beta0))
    agree(got, (want[0][:, None], want[1], want[2][:, None]), "assoc_logistic, two populations, PC1")
    p = got[0][:, 0, LOGIT_P].cpu().numpy()
    assert np.nanargmin(p) == PLANTED and stratified != PLANTED
    st.close()


# ---- the reader and the CLI -----------------------------------------------------------------------------------------------
FIELDS = ("chrom", "pos", "ref", "alt", "n", "af", "beta", "se", "z", "p", "score_chi2", "score_p", "steps", "status")
STATUS_NAMES = ("tested", "no_call", "one_class", "collinear", "not_converged")


def test_reader_and_cli(ctx, cohort, scan):
    from click.testing import CliRunner
    from haplohyped_varawareml_amd.assoc import scan as scan_main
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    from tests.test_gpu_assoc import same_records
    tmp = cohort["tmp"]
    g = f"chr_{CHROM3}"
    names = synth.sample_names(S3)
    many, cov, y = scan["many"][:120], scan["cov"][:120], scan["y"][:120]
    donors = [names[i] for i in many]
    path = cohort["paths"][0]
    r = VCFH5Reader(path, ctx=ctx)
    st = r.store
    mask = st.variant_mask(g, donors, min_maf=0.2)
    at = np.flatnonzero(mask.cpu().numpy())
    for test in ("wald", "score"):
        stats, calls, info = (x.cpu().numpy() for x in st.assoc_logistic(g, y, cov, donors, variant_mask=mask, test=test))
        recs = r.association(y, cov, donor_ids=donors, min_maf=0.2, chromosomes=[CHROM3], model="logistic", test=test)
        assert len(recs) == 2 and all(rec.dtype.names == FIELDS and len(rec) == len(at) for rec in recs)
        for k, rec in enumerate(recs):
            assert np.array_equal(rec["n"], calls[:, 0])
            assert np.array_equal(rec["af"], (calls[:, 1] + 2.0 * calls[:, 2]) / calls[:, 0] / 2.0, equal_nan=True)
            for c, f in enumerate(FIELDS[6:12]):
                assert np.array_equal(rec[f], stats[:, k, c], equal_nan=True)
            assert np.array_equal(rec["steps"], info[:, k, 0]) and np.array_equal(rec["status"], info[:, k, 1])
        shared = r.association(y, cov, donor_ids=donors, min_maf=0.2)[0]
        assert all(np.array_equal(recs[0][f], shared[f], equal_nan=f == "af") for f in FIELDS[:6])
    # the default is the linear scan, and naming it changes nothing
    lin = r.association(y, cov, donor_ids=donors, min_maf=0.2)
    named = r.association(y, cov, donor_ids=donors, min_maf=0.2, model="linear")
    assert all(same_records(u, v) and u.tobytes() == v.tobytes() for u, v in zip(lin, named))
    assert lin[0].dtype.names == FIELDS[:6] + ("beta", "se", "t", "p")
    with pytest.raises(ValueError):
        r.association(y, cov, donor_ids=donors, model="probit")
    with pytest.raises(ValueError):
        r.association(y + 1, cov, donor_ids=donors, model="logistic")
    # pcs = 1 is the component passed by hand
    pcs, _ = r.principal_components(1, donor_ids=donors, min_maf=0.2)
    a = r.association(y[:, 0], donor_ids=donors, min_maf=0.2, pcs=1, model="logistic")
    b = r.association(y[:, 0], pcs["pc1"][:, None], donor_ids=donors, min_maf=0.2, model="logistic")
    assert len(a) == 1 and same_records(a[0], b[0])
    # the CLI
    table = lambda who, cols, x: "#IID\t" + "\t".join(cols) + "\n" + "".join(
        d + "\t" + "\t".join("%.17g" % v for v in row) + "\n" for d, row in zip(who, x.tolist()))
    (tmp / "cc.tsv").write_text(table(donors, ["asthma", "t2d"], y))
    (tmp / "cc12.tsv").write_text(table(donors, ["asthma", "t2d"], y + 1))
    (tmp / "cc_covar.tsv").write_text(table(donors[::-1], ["pc", "height"], cov[::-1]))
    out = str(tmp / "logistic.tsv")
    base = ["--h5", path, "--covar", str(tmp / "cc_covar.tsv"), "--out", out, "--min_maf", "0.2", "--chromosome", str(CHROM3)]
    texts = {}
    for test, pheno, more in (("wald", "cc.tsv", []), ("score", "cc.tsv", []), ("wald", "cc12.tsv", ["--case_control_12"])):
        res = CliRunner().invoke(scan_main, base + ["--pheno", str(tmp / pheno), "--model", "logistic", "--test", test] + more)
        assert res.exit_code == 0, res.output
        want = r.association(y, cov, donor_ids=donors, min_maf=0.2, model="logistic", test=test)
        texts[test, pheno] = open(out).read()
        lines = texts[test, pheno].splitlines()
        assert lines[0] == "#CHROM\tPOS\tREF\tALT\tPHENO\tN\tAF\tBETA\tSE\tZ\tP\tSCORE_CHI2\tSCORE_P\tSTEPS\tSTATUS"
        assert len(lines) == 1 + 2 * len(want[0])
        cells = [ln.split("\t") for ln in lines[1:]]
        for k, name in enumerate(("asthma", "t2d")):
            mine = cells[k::2]
            assert all(c[4] == name for c in mine)
            assert np.array_equal(np.array([int(c[1]) for c in mine]), want[k]["pos"])
            assert np.array_equal(np.array([int(c[5]) for c in mine]), want[k]["n"])
            for col, f in zip(range(6, 13), ("af",) + FIELDS[6:12]):
                assert np.array_equal(np.array([float(c[col]) for c in mine]), want[k][f], equal_nan=True)     # %.17g round-trips
            assert np.array_equal(np.array([int(c[13]) for c in mine]), want[k]["steps"])
            assert [c[14] for c in mine] == [STATUS_NAMES[s] for s in want[k]["status"]]
    assert texts["wald", "cc12.tsv"] == texts["wald", "cc.tsv"] != texts["score", "cc.tsv"]
    # without --model the output is the linear scan's, as the embedded command writes it
    from haplohyped_varawareml_amd.assoc import main
    linear = []
    for command in (scan_main, main):
        res = CliRunner().invoke(command, base + ["--pheno", str(tmp / "cc.tsv")])
        assert res.exit_code == 0, res.output
        linear.append(open(out).read())
    assert linear[0] == linear[1] and linear[0].startswith("#CHROM\tPOS\tREF\tALT\tPHENO\tN\tAF\tBETA\tSE\tT\tP\n")
    # usage errors: a 2 without --case_control_12 (the message names the column), a 0 with it, a value that is no class, the
    # model's options without the model
    (tmp / "cc_bad.tsv").write_text(table(donors, ["asthma", "t2d"], np.where(np.arange(len(y))[:, None] == 3, 0.5, y)))
    for args, word in ((["--pheno", str(tmp / "cc12.tsv"), "--model", "logistic"], "asthma"),
                       (["--pheno", str(tmp / "cc.tsv"), "--model", "logistic", "--case_control_12"], "asthma"),
                       (["--pheno", str(tmp / "cc_bad.tsv"), "--model", "logistic"], "asthma"),
                       (["--pheno", str(tmp / "cc.tsv"), "--test", "score"], "logistic"),
                       (["--pheno", str(tmp / "cc.tsv"), "--case_control_12"], "logistic")):
        res = CliRunner().invoke(scan_main, base + args)
        assert res.exit_code != 0 and word in res.output, (args, res.output)
    r.close()
