"""`VCFH5Reader` — the reference's reader class (/root/reference/src/utils/h5_reader.py:5-46) over the
cohort store.  fetch_genotypes(donor_id, chromosome) returns the reference's per-donor compound records
(dtype of vcf_to_h5.py:119-127) whichever dataset name the caller meant: the reference's writer says
`snp_data` (vcf_to_h5.py:134), its reader says `genotype` (h5_reader.py:40) — both resolve here.
fetch_region(donor_id, chromosome, start, end) is the same for the variants with start <= pos < end only: a read of a
hyperslab, which decodes just the Blosc blocks of those variants (the reference's reader can only read whole datasets).
allele_frequencies(chromosome, start, end, donor_ids) gives per-variant allele counts and frequencies over the cohort or
a subset of it, counted on the device (GenotypeStore.allele_counts); sample_statistics(chromosomes, start, end, donor_ids,
min_maf, singletons) the same counters per donor, summed over the variants of a region or of a class of variants
(GenotypeStore.sample_counts): call rate, heterozygosity, singletons carried; relatedness(chromosomes, donor_ids, min_maf,
min_kinship) the pairwise counts and the KING-robust kinship of every pair of donors (GenotypeStore.pair_counts);
ld_prune(chromosomes, donor_ids, min_maf, window, r2) the variants a greedy LD pruning keeps (GenotypeStore.ld_prune);
genetic_relationship(chromosomes, donor_ids, min_maf, ld_window, ld_r2) the standardised genetic relationship matrix of the
donors over the variants that pass min_maf and, with ld_window, the LD pruning (GenotypeStore.grm_sums), and
principal_components(k, ...) its k largest eigenpairs, one record per donor (store.top_eigenpairs: numpy.linalg.eigh on the
host); association(phenotypes, covariates, chromosomes, donor_ids, min_maf, pcs, ...) a single-variant linear regression
scan of every variant against one or more phenotypes (GenotypeStore.assoc), or with model="logistic" the logistic one of
case / control phenotypes (GenotypeStore.assoc_logistic); polygenic_scores(variants, weights, ...) the
per-donor sums of per-allele effects over listed variants (GenotypeStore.score), and project_components(k,
train_donor_ids, donor_ids, ...) principal components fitted on some donors and the projection of others onto them
(GenotypeStore.project); feature_matrix(chromosomes, donor_ids, min_maf, ld_window, ..., train_donor_ids) donors x selected
variants as a model-ready device tensor with its variant records (GenotypeStore.feature_matrix); clump(variants, p, ...) the
LD clumps of a scan's p-values, one record per listed variant with its role and its index variant (GenotypeStore.ld_clump);
burden(regions, donor_ids, max_maf, ...) one score per donor and region — the rare variants of a gene collapsed into one
number (GenotypeStore.burden) — and burden_association(regions, phenotypes, ...) the regression or score test of phenotypes
on those scores.  The reference has no such queries."""
import numpy as np

from .store import (AC, AN, HET, HET1, HETHET, HOM_ALT, IBS0, NSNP, GenotypeStore, assoc_design,
                    check_components, clump_summary, dense_assoc, dense_logistic_score, grm_from_sums, kinship_from_counts,
                    logistic_design, logistic_score_design, loco_sums, mixed_null, top_eigenpairs, variant_columns)


def _span(starts, start, end):
    """the variants of a group (their 0-based starts, ascending) whose start lies in [start, end) (None: no bound) ->
    (lo, hi), indices"""
    starts = starts.astype(np.int64)
    lo = 0 if start is None else int(np.searchsorted(starts, start, side="left"))
    hi = len(starts) if end is None else max(int(np.searchsorted(starts, end, side="left")), lo)
    return lo, hi


class VCFH5Reader:
    def __init__(self, h5_file, ctx=None):
        self.h5_file = h5_file
        self.store = GenotypeStore(h5_file, ctx=ctx)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _group(self, donor_id, chromosome):
        group = f"chr_{chromosome}"
        if group not in self.store.meta["groups"] or donor_id not in self.store.samples:
            raise KeyError(f"No data found for donor_{donor_id}/chr_{chromosome}")     # h5_reader.py:42-43
        return group

    def _cohort(self, chromosomes, donor_ids):
        """what the queries ask for -> (the chromosomes' group names, donors, who): chromosomes one name, a list or None for
        every group; donor_ids a list or None for every sample, `who` being what GenotypeStore takes for them (None stays
        None).  KeyError, in the reference's words, for a chromosome or a donor the file does not have."""
        st = self.store
        if chromosomes is None:
            chroms = [g[len("chr_"):] for g in st.groups()]
        else:
            chroms = [chromosomes] if isinstance(chromosomes, (str, int)) else list(chromosomes)
        donors = list(st.samples) if donor_ids is None else list(donor_ids)
        for c in chroms:
            for d in (st.samples[:1] if donor_ids is None else donors) or st.samples[:1]:     # (the store's own are known)
                self._group(d, c)
        return [f"chr_{c}" for c in chroms], donors, None if donor_ids is None else donors

    def _variant_masks(self, names, who, spans=None, min_maf=None, singletons=False, ld_window=None, ld_r2=0.2):
        """which variants of the groups `names` a query over `who` takes -> {group: bool device tensor}, {} for all: those
        that pass min_maf / singletons (variant_mask over spans[group] = (lo, hi), default all), then ld_prune's of them"""
        st, masks, one = self.store, {}, 1 if singletons else None
        for g in names:
            if min_maf is not None or singletons:
                masks[g] = st.variant_mask(g, who, *(spans or {}).get(g, (0, None)), min_maf=min_maf, min_ac=one, max_ac=one)
            if ld_window is not None:
                masks[g] = st.ld_prune(g, who, variant_mask=masks.get(g), window=ld_window, r2=ld_r2)
        return masks

    _variant_columns = staticmethod(variant_columns)      # (GenotypeStore.snp_records fills its records with it too)

    def _donor_column(self, donors):
        """the names as bytes -> S{width} [len(donors)], width that of the longest encoded name, at least 1"""
        return np.array([x.encode() for x in donors], dtype=f"S{max([len(x.encode()) for x in donors] + [1])}")

    def fetch_genotypes(self, donor_id, chromosome):
        return self.store.snp_records(self._group(donor_id, chromosome), donor_id)

    def fetch_region(self, donor_id, chromosome, start, end):
        """the records of fetch_genotypes whose 0-based start lies in [start, end)"""
        group = self._group(donor_id, chromosome)
        tables = self.store.variants(group)
        lo, hi = _span(tables[0], start, end)
        return self.store.snp_records(group, donor_id, lo, hi, tables=tables)

    def allele_frequencies(self, chromosome, start=None, end=None, donor_ids=None):
        """per-variant allele counts of chr_{chromosome} over donor_ids (default: every sample), for the variants whose
        0-based start lies in [start, end) (None: no bound), as host numpy records: chrom (the group's CHROM runs),
        start, stop, ref, alt as in fetch_genotypes, then an (called alleles), ac (alleles equal to 1), af = ac / an
        (float32, NaN where an == 0), het, hom_alt"""
        [group], _, who = self._cohort([chromosome], donor_ids)
        tables = self.store.variants(group)
        lo, hi = _span(tables[0], start, end)
        c = self.store.allele_counts(group, who, lo, hi).cpu().numpy()
        width = max([len(r[1].encode()) for r in tables[3]] + [1])
        rec = np.zeros(hi - lo, dtype=[("chrom", f"S{width}"), ("start", np.uint32), ("stop", np.uint32), ("ref", "S10"),
                                       ("alt", "S10"), ("an", np.int32), ("ac", np.int32), ("af", np.float32),
                                       ("het", np.int32), ("hom_alt", np.int32)])
        self._variant_columns(rec, tables, width, lo=lo, hi=hi)
        rec["an"], rec["ac"], rec["het"], rec["hom_alt"] = c[:, AN], c[:, AC], c[:, HET], c[:, HOM_ALT]
        rec["af"] = np.where(c[:, AN] > 0, c[:, AC] / np.maximum(c[:, AN], 1), np.nan).astype(np.float32)
        return rec

    def sample_statistics(self, chromosomes=None, start=None, end=None, donor_ids=None, min_maf=None, singletons=False):
        """per-donor counts over the variants of chr_{N} for N in chromosomes (one name or a list; None: every group), as
        host numpy records, one per donor in the order asked (default: every sample): sample, n_variants (the variants
        counted, the same in every row), an (called alleles), ac (alleles equal to 1), het, hom_alt, missing (= 2 *
        n_variants - an), call_rate (float64 an / (2 * n_variants), NaN when n_variants = 0).  start / end: only the
        variants whose 0-based start lies in [start, end) — with exactly one chromosome.  min_maf / singletons: only the
        variants whose minor allele frequency is at least min_maf / whose alternate allele is carried exactly once, both
        taken over the donors asked for (GenotypeStore.variant_mask over them), computed and applied on the device."""
        st = self.store
        names, donors, who = self._cohort(chromosomes, donor_ids)
        if (start is not None or end is not None) and len(names) != 1:
            raise ValueError("sample_statistics: start / end need exactly one chromosome")
        spans = {g: (0, st.meta["groups"][g]["n_variants"]) for g in names}
        if start is not None or end is not None:
            spans[names[0]] = _span(st.variants(names[0])[0], start, end)
        masks = self._variant_masks(names, who, spans, min_maf, singletons)
        n_variants = sum(int(masks[g].sum()) if g in masks else spans[g][1] - spans[g][0] for g in names)
        lo, hi = spans[names[0]] if len(names) == 1 else (0, None)
        c = st.sample_counts(names, who, lo, hi, variant_mask=masks or None).cpu().numpy().astype(np.int64)
        sample = self._donor_column(donors)
        rec = np.zeros(len(donors), dtype=[("sample", sample.dtype), ("n_variants", np.int64), ("an", np.int64),
                                           ("ac", np.int64), ("het", np.int64), ("hom_alt", np.int64),
                                           ("missing", np.int64), ("call_rate", np.float64)])
        rec["sample"], rec["n_variants"] = sample, n_variants
        rec["an"], rec["ac"], rec["het"], rec["hom_alt"] = c[:, AN], c[:, AC], c[:, HET], c[:, HOM_ALT]
        rec["missing"] = 2 * n_variants - c[:, AN]
        rec["call_rate"] = c[:, AN] / (2.0 * n_variants) if n_variants else np.nan
        return rec

    def relatedness(self, chromosomes=None, donor_ids=None, min_maf=None, min_kinship=None):
        """the pairs i < j of donor_ids (default: every sample, store order) over the variants of chr_{N} for N in
        chromosomes (one name or a list; None: every group), as host numpy records: sample1, sample2, nsnp (variants at
        which both calls are complete: both alleles 0 or 1), hethet (both heterozygous), ibs0 (opposite homozygotes), het1
        / het2 (sample1 / sample2 heterozygous, the other complete), kinship (float64: store.kinship_from_counts, the
        KING-robust estimator as defined there — not checked against plink2; NaN where neither has such a heterozygote).
        min_maf: only the variants whose minor allele frequency over the donors asked for is at least that
        (GenotypeStore.variant_mask per group, computed and applied on the device).  min_kinship: only the pairs at or above
        it (NaN pairs are then dropped)."""
        st = self.store
        names, donors, who = self._cohort(chromosomes, donor_ids)
        table = st.pair_counts(names, who, variant_mask=self._variant_masks(names, who, min_maf=min_maf) or None)
        phi = kinship_from_counts(table).cpu().numpy()
        t = table.cpu().numpy().astype(np.int64)
        i, j = np.triu_indices(len(donors), 1)
        if min_kinship is not None:
            with np.errstate(invalid="ignore"):
                keep = phi[i, j] >= float(min_kinship)
            i, j = i[keep], j[keep]
        enc = self._donor_column(donors)
        rec = np.zeros(len(i), dtype=[("sample1", enc.dtype), ("sample2", enc.dtype), ("nsnp", np.int64),
                                      ("hethet", np.int64), ("ibs0", np.int64), ("het1", np.int64), ("het2", np.int64),
                                      ("kinship", np.float64)])
        rec["sample1"], rec["sample2"] = enc[i], enc[j]
        rec["nsnp"], rec["hethet"], rec["ibs0"] = t[i, j, NSNP], t[i, j, HETHET], t[i, j, IBS0]
        rec["het1"], rec["het2"] = t[i, j, HET1], t[j, i, HET1]
        rec["kinship"] = phi[i, j]
        return rec

    def ld_prune(self, chromosomes=None, donor_ids=None, min_maf=None, window=50, r2=0.2):
        """greedy LD pruning of chr_{N} for N in chromosomes (one name or a list; None: every group), each group on its own
        (no LD across groups), over donor_ids (default: every sample), as host numpy records, one per variant of the
        chosen groups in the order asked: chrom, start (0-based), ref, alt, counted (the variant took part: it passed
        min_maf, the minor allele frequency over the donors asked for — GenotypeStore.variant_mask, computed and applied
        on the device; without min_maf every variant), keep (counted, and no kept variant among the `window` counted
        variants before it has r^2 > r2 with it: GenotypeStore.ld_prune, whose rule is this project's, not plink2's
        --indep-pairwise)."""
        st = self.store
        names, donors, who = self._cohort(chromosomes, donor_ids)
        parts, tables = [], [st.variants(g) for g in names]
        width = max([len(r[1].encode()) for t in tables for r in t[3]] + [1])
        dtype = [("chrom", f"S{width}"), ("start", np.uint32), ("ref", "S10"), ("alt", "S10"), ("counted", bool), ("keep", bool)]
        for g, t in zip(names, tables):
            mask = self._variant_masks([g], who, min_maf=min_maf).get(g)
            keep = st.ld_prune(g, who, variant_mask=mask, window=window, r2=r2).cpu().numpy()
            rec = np.zeros(len(t[0]), dtype=dtype)
            self._variant_columns(rec, t, width)
            rec["counted"], rec["keep"] = True if mask is None else mask.cpu().numpy(), keep
            parts.append(rec)
        return np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)

    def genetic_relationship(self, chromosomes=None, donor_ids=None, min_maf=None, ld_window=None, ld_r2=0.2):
        """the standardised genetic relationship matrix of donor_ids (default: every sample, store order) over the
        variants of chr_{N} for N in chromosomes (one name or a list; None: every group) -> (donors, grm float64 [n, n],
        nsnp int32 [n, n]), host numpy: store.grm_from_sums of GenotypeStore.grm_sums — per pair, the mean over the variants
        at which both calls are complete (nsnp of them) of the product of the two standardised dosages, NaN where there is
        none; the formulas there are the contract, not GCTA's or plink2's files.  min_maf: only the variants whose minor
        allele frequency over the donors asked for is at least that (GenotypeStore.variant_mask per group); ld_window: of
        those, only the variants a greedy LD pruning keeps (GenotypeStore.ld_prune per group, `ld_window` counted variants,
        r^2 > ld_r2 drops).  Every mask is computed and applied on the device."""
        names, donors, who = self._cohort(chromosomes, donor_ids)
        masks = self._variant_masks(names, who, min_maf=min_maf, ld_window=ld_window, ld_r2=ld_r2)
        sums, nsnp = self.store.grm_sums(names, who, variant_mask=masks or None)
        return donors, grm_from_sums(sums, nsnp).cpu().numpy(), nsnp.cpu().numpy()

    def feature_matrix(self, chromosomes=None, donor_ids=None, min_maf=None, ld_window=None, ld_r2=0.2, coding="dosage",
                       dtype=None, impute="mean", train_donor_ids=None):
        """donors x selected variants as a model-ready tensor -> (donors, X, variant records): X is
        GenotypeStore.feature_matrix's device tensor (coding, dtype and impute mean what they mean there), row i for
        donor_ids[i] in the order asked (default: every sample, store order), its columns the variants of chr_{N} for N in
        chromosomes (one name or a list; None: every group) that pass min_maf and, with ld_window, the LD pruning, as in
        genetic_relationship; the records, host numpy, one per column: chrom, start (0-based), ref, alt.  With
        train_donor_ids the masks AND the frequencies behind the imputed and standardised values are computed over the
        training donors only, so held-out donors leak into neither; without it, over the donors asked for."""
        names, donors, who = self._cohort(chromosomes, donor_ids)
        train = who if train_donor_ids is None else self._cohort(chromosomes, list(train_donor_ids))[2]
        masks = self._variant_masks(names, train, min_maf=min_maf, ld_window=ld_window, ld_r2=ld_r2)
        X, columns = self.store.feature_matrix(names, who, variant_mask=masks or None, coding=coding, dtype=dtype,
                                               impute=impute, freq_samples=train)
        tables = {g: self.store.variants(g) for g, _ in columns}
        width = max([len(r[1].encode()) for t in tables.values() for r in t[3]] + [1])
        dtype = [("chrom", f"S{width}"), ("start", np.uint32), ("ref", "S10"), ("alt", "S10")]
        parts = []
        for g, at in columns:
            rec = np.zeros(int(at.numel()), dtype=dtype)
            self._variant_columns(rec, tables[g], width, at=at.cpu().numpy())
            parts.append(rec)
        return donors, X, np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)

    def principal_components(self, k=10, chromosomes=None, donor_ids=None, min_maf=None, ld_window=None, ld_r2=0.2):
        """the k largest principal components of genetic_relationship (same arguments after k) -> (records, values):
        host numpy records, one per donor in the order asked — sample, pc1 .. pck (float64: the donor's component of each
        unit eigenvector, whose component of largest magnitude is positive) —, and the eigenvalues float64 [k], descending
        (store.top_eigenpairs: numpy.linalg.eigh on the host).  ValueError if k is outside 1..n or a pair of donors has
        no jointly complete variant."""
        k = check_components(k, len(self.store.samples) if donor_ids is None else len(list(donor_ids)))
        donors, grm, _ = self.genetic_relationship(chromosomes, donor_ids, min_maf, ld_window, ld_r2)
        values, vectors = top_eigenpairs(grm, k)
        return self._component_records(donors, vectors), values

    def _component_records(self, donors, vectors):
        """float64 [len(donors), k] -> principal_components' records: sample, pc1 .. pck"""
        sample, k = self._donor_column(donors), vectors.shape[1]
        rec = np.zeros(len(donors), dtype=[("sample", sample.dtype)] + [(f"pc{c + 1}", np.float64) for c in range(k)])
        rec["sample"] = sample
        for c in range(k):
            rec[f"pc{c + 1}"] = vectors[:, c]
        return rec

    def project_components(self, k, train_donor_ids, donor_ids=None, chromosomes=None, min_maf=None, ld_window=None, ld_r2=0.2):
        """principal components fitted on train_donor_ids and the projection of donor_ids onto them -> (training records,
        projected records, values), records as principal_components returns them.  The variant masks (min_maf, ld_window,
        ld_r2), the relationship matrix and its k largest eigenpairs run over the training donors exactly as
        principal_components(k, chromosomes, train_donor_ids, ...) runs them, so the held-out donors touch neither; they are
        then projected (GenotypeStore.project: the components' variant loadings from the training donors, applied to each
        donor's complete calls).  donor_ids: default every sample that is not a training donor, in store order.  A
        training donor listed in donor_ids gets its projection, which is its fitted entry only up to its incomplete
        calls (GenotypeStore.project says how far)."""
        train = list(train_donor_ids)
        k = check_components(k, len(train))
        names, train, who = self._cohort(chromosomes, train)
        if donor_ids is None:
            fitted = set(train)
            donor_ids = [s for s in self.store.samples if s not in fitted]
        _, donors, _ = self._cohort(chromosomes, list(donor_ids))
        masks = self._variant_masks(names, who, min_maf=min_maf, ld_window=ld_window, ld_r2=ld_r2)
        sums, nsnp = self.store.grm_sums(names, who, variant_mask=masks or None)
        values, vectors = top_eigenpairs(grm_from_sums(sums, nsnp).cpu().numpy(), k)
        projected = np.zeros((0, k))
        if donors:
            projected = self.store.project(vectors, values, who, donors, names, variant_mask=masks or None).cpu().numpy()
        return self._component_records(train, vectors), self._component_records(donors, projected), values

    @staticmethod
    def _listed_keys(variants):
        """listed variants — a numpy record array with chrom, pos (1-based), ref, alt, or a sequence of such 4-tuples; str
        or bytes — -> their keys, a list of (chrom without a leading "chr", pos, ref, alt)"""
        if isinstance(variants, np.ndarray) and variants.dtype.names:
            columns = [variants[f].tolist() for f in ("chrom", "pos", "ref", "alt")]
        else:
            columns = [list(c) for c in zip(*(tuple(x) for x in variants))] or [[], [], [], []]
        text = lambda col: [x.decode() if isinstance(x, bytes) else str(x) for x in col]                       # noqa: E731
        chrom, ref, alt = text(columns[0]), text(columns[2]), text(columns[3])
        pos = np.array([int(p) for p in columns[1]], dtype=np.int64)
        return list(zip((c[3:] if c.startswith("chr") else c for c in chrom), pos.tolist(), ref, alt))

    def _match_listed(self, who, keys, groups):
        """the listed variants (_listed_keys) matched to the store's, for `who` in the message: by (group chr_{N} of the
        chrom, pos, REF base, ALT base) — one base each, no flipping; the first of a store's equal keys is the match —
        -> {group: (listed, where, n_var)} for the groups of `groups` with a match, in their order: the indices into keys of
        the matched variants, the offsets of their matches in the group, the group's number of variants.  ValueError for
        a key listed twice."""
        if len(set(keys)) != len(keys):
            seen = set()
            twice = next(k for k in keys if k in seen or seen.add(k))
            raise ValueError(f"{who}: chr{twice[0]}:{twice[1]} {twice[2]}>{twice[3]} is listed twice")
        out = {}
        for g in groups:
            mine = [i for i, k in enumerate(keys) if "chr_" + k[0] == g and len(k[2]) == 1 and len(k[3]) == 1]
            if not mine:
                continue
            start, s_ref, s_alt, _ = self.store.variants(g)
            # one int64 per variant: (0-based start, REF base, ALT base); the first of a store's equal keys is the match
            code = (start.astype(np.int64) << 16) | (s_ref.astype(np.int64) << 8) | s_alt.astype(np.int64)
            order = np.argsort(code, kind="stable")
            want = np.array([((keys[i][1] - 1) << 16) | (ord(keys[i][2]) << 8) | ord(keys[i][3]) for i in mine], dtype=np.int64)
            at = np.searchsorted(code[order], want)
            hit = (at < len(code)) & (code[order][np.minimum(at, len(code) - 1)] == want) if len(code) else np.zeros(len(mine), bool)
            if hit.any():
                out[g] = (np.array(mine)[hit], order[at[hit]], len(start))
        return out

    def clump(self, variants, p, chromosomes=None, donor_ids=None, p1=1e-4, p2=1e-2, r2=0.5, window=1024, kb=250.0):
        """LD clumping of the listed variants by their p-values -> (records, info).  variants: n records with chrom, pos
        (1-based), ref, alt, matched to the store's exactly as polygenic_scores matches its weights (no flipping; a key
        listed twice: ValueError); p: float64 [n], NaN for a variant that takes no part.  Each group of chromosomes (one
        name or a list; None: every group) is clumped on its own, over donor_ids (default: every sample), by
        GenotypeStore.ld_clump (p1, p2, r2, window, kb mean what they mean there; its rule is this project's, not plink's
        .clumped file).  records: host numpy, one per matched listed variant with p <= p2, in group and file order — chrom,
        start (0-based), ref, alt, p, role (store_stats.CLUMP_NONE, CLUMP_INDEX, CLUMP_CLUMPED), index (the row, within
        these records, of its index variant: its own row for an index, -1 for none), n_clumped (the members an index
        variant claimed; 0 otherwise), listed (its row in `variants`).  info: matched, unmatched (listed variants the
        store does not have) and window_short (GenotypeStore.stats["clump_window_short"] of the calls: variants where
        `window`, not kb, ended the search)."""
        st = self.store
        groups, _, who = self._cohort(chromosomes, donor_ids)
        keys = self._listed_keys(variants)
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if len(p) != len(keys):
            raise ValueError(f"clump: {len(p)} p-values for {len(keys)} variants")
        matches = self._match_listed("clump", keys, groups)
        tables = {g: st.variants(g) for g in matches}
        width = max([len(r[1].encode()) for t in tables.values() for r in t[3]] + [1])
        dtype = [("chrom", f"S{width}"), ("start", np.uint32), ("ref", "S10"), ("alt", "S10"), ("p", np.float64),
                 ("role", np.int8), ("index", np.int64), ("n_clumped", np.int64), ("listed", np.int64)]
        parts, base, short0 = [], 0, st.stats["clump_window_short"]
        for g, (listed, where, n_var) in matches.items():
            pg = np.full(n_var, np.nan)
            pg[where] = p[listed]
            row_of = np.full(n_var, -1, np.int64)
            row_of[where] = listed
            owner = st.ld_clump(g, pg, who, p1=p1, p2=p2, r2=r2, window=window, kb=kb).cpu().numpy()
            with np.errstate(invalid="ignore"):
                at = np.flatnonzero(pg <= p2)
            rec = np.zeros(len(at), dtype=dtype)
            self._variant_columns(rec, tables[g], width, at=at)
            local = np.full(n_var, -1, np.int64)            # offsets into the group -> rows of this group's records
            local[at] = np.arange(len(at))
            own = np.where(owner[at] >= 0, local[np.maximum(owner[at], 0)], -1)
            s = clump_summary(own, pg[at])
            rec["p"], rec["listed"], rec["role"] = pg[at], row_of[at], s["role"]
            rec["index"] = np.where(own >= 0, base + own, -1)
            rec["n_clumped"][s["index"]] = s["n_clumped"]
            parts.append(rec)
            base += len(at)
        matched = sum(len(m[0]) for m in matches.values())
        info = dict(matched=matched, unmatched=len(keys) - matched, window_short=st.stats["clump_window_short"] - short0)
        return (np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)), info

    def polygenic_scores(self, variants, weights, names=None, donor_ids=None, chromosomes=None, impute="mean", freq_donor_ids=None):
        """polygenic scores of donor_ids (default: every sample, store order) -> (records, info).  variants: n records with
        chrom, pos (1-based, the VCF's POS), ref, alt (a numpy record array with those fields, or a sequence of such
        4-tuples; str or bytes); weights: float64 [n, K] (or [n]), the effect per ALT allele of variant i in score c; names: the K field
        names (default score1 .. scoreK).  A listed variant is matched to the store's by (group chr_{N} of its chrom, with
        or without a leading "chr"; pos; REF base; ALT base): the store holds one base each, so a longer allele matches
        nothing, and there is no allele or strand flipping.  chromosomes: only those groups (one name or a list; None:
        every group); a variant of another chromosome is unmatched.  A key listed twice: ValueError.  The matched variants
        go to GenotypeStore.score (impute "mean" or "none"; freq_donor_ids: the donors of the allele frequencies, default
        the scored ones), whose formulas are the contract.  records: host numpy, one per donor in the order asked —
        sample, n_variants (the variants that took part: the same in every row), one float64 field per name; info: a dict
        of matched, unmatched (listed variants the store does not have) and unused (matched, but without a called allele
        among the frequency donors)."""
        st = self.store
        groups, donors, who = self._cohort(chromosomes, donor_ids)
        freq = None if freq_donor_ids is None else self._cohort(chromosomes, list(freq_donor_ids))[2]
        keys = self._listed_keys(variants)
        w = np.asarray(weights, dtype=np.float64)
        w = w[:, None] if w.ndim == 1 else w
        if w.ndim != 2 or w.shape[0] != len(keys) or not 1 <= w.shape[1] <= 64:
            raise ValueError(f"polygenic_scores: weights {list(w.shape)} for {len(keys)} variants ([n, K], 1 <= K <= 64)")
        names = [f"score{c + 1}" for c in range(w.shape[1])] if names is None else [str(x) for x in names]
        if len(names) != w.shape[1] or len(set(names)) != len(names) or set(names) & {"sample", "n_variants"}:
            raise ValueError(f"polygenic_scores: {w.shape[1]} distinct names other than sample and n_variants, not {names}")
        betas, masks, matched = {}, {}, 0
        for g, (listed, where, n_var) in self._match_listed("polygenic_scores", keys, groups).items():
            betas[g] = np.zeros((n_var, w.shape[1]))
            betas[g][where] = w[listed]
            masks[g] = np.zeros(n_var, bool)
            masks[g][where] = True
            matched += len(listed)
        scores, used = np.zeros((len(donors), w.shape[1])), {}
        if betas:
            scores, used = st.score(betas, list(betas), who, variant_mask=masks, impute=impute, freq_samples=freq)
            scores = scores.cpu().numpy()
        sample = self._donor_column(donors)
        rec = np.zeros(len(donors), dtype=[("sample", sample.dtype), ("n_variants", np.int64)] + [(n, np.float64) for n in names])
        rec["sample"], rec["n_variants"] = sample, sum(used.values())
        for c, n in enumerate(names):
            rec[n] = scores[:, c]
        return rec, dict(matched=matched, unmatched=len(keys) - matched, unused=matched - sum(used.values()))

    def association(self, phenotypes, covariates=None, chromosomes=None, donor_ids=None, min_maf=None, pcs=0,
                    ld_window=None, ld_r2=0.2, model="linear", test="wald"):
        """single-variant linear regression scan of chr_{N} for N in chromosomes (one name or a list; None: every group)
        over donor_ids (default: every sample, store order; each donor once) -> a list with one host numpy record array
        per phenotype, one record per scanned variant in group and variant order: chrom, pos (1-based, the VCF's POS),
        ref, alt, n (complete calls among the donors), af (mean dosage of the complete calls / 2; NaN without one), beta,
        se, t, p (float64: store.assoc_from_sums, whose formulas are the contract — the coefficient of the dosage in the
        fit of the phenotype on [1 | covariates | dosage], a call that is not complete imputed to the variant's mean; NaN
        where the variant is not tested).  phenotypes is [n] or [n, P], covariates [n, q0] or None, both aligned with the
        donors.  pcs = K appends the K components of principal_components over the same donors and chromosomes, with
        min_maf, ld_window and ld_r2, to the covariates.  The scan itself runs over the variants that pass min_maf (the
        minor allele frequency over the donors: GenotypeStore.variant_mask), not over the LD-pruned set.
        model = "logistic": the phenotypes are 0 / 1 and every variant gets a logistic regression
        (GenotypeStore.assoc_logistic; store.logistic_fit_reference is the contract): after af the records carry beta (the
        log odds ratio per ALT allele), se, z, p (the Wald test), score_chi2, score_p (the score test at the null model),
        steps (Newton steps) and status (store.LOGIT_TESTED ... LOGIT_NOT_CONVERGED; the six statistics are NaN unless
        tested).  test = "score" skips the fits: the score test alone, the Wald columns NaN."""
        if model not in ("linear", "logistic"):
            raise ValueError(f"association: model {model!r} (\"linear\" or \"logistic\")")
        st = self.store
        names, donors, who = self._cohort(chromosomes, donor_ids)
        y = np.asarray(phenotypes, dtype=np.float64)
        P = 1 if y.ndim == 1 else y.shape[1]
        cov = None if covariates is None else np.asarray(covariates, dtype=np.float64)
        if int(pcs):
            rec, _ = self.principal_components(int(pcs), chromosomes, donor_ids, min_maf, ld_window, ld_r2)
            pc = np.stack([rec[f"pc{c + 1}"] for c in range(int(pcs))], axis=1)
            cov = pc if cov is None else np.concatenate([cov, pc], axis=1)
        tables = [st.variants(g) for g in names]
        width = max([len(r[1].encode()) for t in tables for r in t[3]] + [1])
        floats = ("beta", "se", "t", "p") if model == "linear" else ("beta", "se", "z", "p", "score_chi2", "score_p")
        dtype = [("chrom", f"S{width}"), ("pos", np.uint32), ("ref", "S10"), ("alt", "S10"), ("n", np.int64),
                 ("af", np.float64)] + [(f, np.float64) for f in floats]
        if model == "logistic":
            dtype += [("steps", np.int64), ("status", np.int64)]
        parts = [[] for _ in range(P)]
        for g, t in zip(names, tables):
            mask = self._variant_masks([g], who, min_maf=min_maf).get(g)
            if model == "linear":
                stats, calls = (x.cpu().numpy() for x in st.assoc(g, y, cov, who, variant_mask=mask))
            else:
                stats, calls, info = (x.cpu().numpy() for x in st.assoc_logistic(g, y, cov, who, variant_mask=mask, test=test))
            at = np.arange(len(t[0])) if mask is None else np.flatnonzero(mask.cpu().numpy())
            shared = np.zeros(len(at), dtype=dtype)             # what every phenotype's records say alike
            self._variant_columns(shared, t, width, at=at, pos=True)
            shared["n"] = calls[:, 0]
            with np.errstate(divide="ignore", invalid="ignore"):
                shared["af"] = (calls[:, 1] + 2.0 * calls[:, 2]) / calls[:, 0] / 2.0
            for k in range(P):
                rec = shared.copy()
                for c, f in enumerate(floats):       # (the statistics' columns in the records' order: ASSOC_*, LOGIT_*)
                    rec[f] = stats[:, k, c]
                if model == "logistic":
                    rec["steps"], rec["status"] = info[:, k, 0], info[:, k, 1]
                parts[k].append(rec)
        return [np.concatenate(p) if p else np.zeros(0, dtype=dtype) for p in parts]

    def mixed_association(self, phenotypes, covariates=None, chromosomes=None, donor_ids=None, min_maf=None, grm_min_maf=None,
                          ld_window=None, ld_r2=0.2, loco=False):
        """mixed-model association scan of chr_{N} for N in chromosomes (one name or a list; None: every group) over
        donor_ids (default: every sample, store order; each donor once) -> (records, nulls).  records is association's
        list — one host numpy record array per phenotype, one record per scanned variant: chrom, pos, ref, alt, n, af, beta,
        se, z, p —, the statistics those of store_stats.mixed_from_forms: the generalised least-squares effect of the
        dosage in y = [1 | covariates] alpha + dosage beta + u + e with Var(u) = sg2 K, the variance components fixed at
        the null model (store_stats.mixed_null; the formulas there are the contract, not GCTA's .mlma file).  K is the
        relationship matrix of genetic_relationship over the same donors and chromosomes, with grm_min_maf, ld_window and
        ld_r2 as its min_maf, ld_window and ld_r2; the scan itself runs over the variants that pass min_maf.  loco = True:
        every scanned chromosome is tested against the K of the other chosen chromosomes (GenotypeStore.grm_sums once per
        group, store_stats.loco_sums, a null fit per chromosome and phenotype) — ValueError if only one is chosen.  nulls is
        a list with one record array per phenotype: chrom, h2, sigma2 — one record with chrom "*" without loco, one per
        scanned chromosome with it."""
        from .store_mixed import scan_under_null
        st = self.store
        names, donors, who = self._cohort(chromosomes, donor_ids)
        y = np.asarray(phenotypes, dtype=np.float64)
        y = y[:, None] if y.ndim == 1 else y
        cov = None if covariates is None else np.asarray(covariates, dtype=np.float64)
        grm_masks = self._variant_masks(names, who, min_maf=grm_min_maf, ld_window=ld_window, ld_r2=ld_r2)
        tables = [st.variants(g) for g in names]
        width = max([len(r[1].encode()) for t in tables for r in t[3]] + [1])
        if loco:
            by_group = {g: st.grm_sums([g], who, variant_mask={g: grm_masks[g]} if g in grm_masks else None) for g in names}
            sums, nsnp = {g: x[0] for g, x in by_group.items()}, {g: x[1] for g, x in by_group.items()}
            kin = {g: grm_from_sums(*loco_sums(sums, nsnp, g)).cpu().numpy() for g in names}
        else:
            kin = dict.fromkeys(names, grm_from_sums(*st.grm_sums(names, who, variant_mask=grm_masks or None)).cpu().numpy())
        fitted = {}                                              # (id of the matrix, phenotype) -> its null model

        def null_of(g, k):
            key = (id(kin[g]), k)
            if key not in fitted:
                fitted[key] = mixed_null(kin[g], y[:, k], cov)
            return fitted[key]
        floats = ("beta", "se", "z", "p")
        dtype = [("chrom", f"S{width}"), ("pos", np.uint32), ("ref", "S10"), ("alt", "S10"), ("n", np.int64),
                 ("af", np.float64)] + [(f, np.float64) for f in floats]
        null_dtype = [("chrom", f"S{width}"), ("h2", np.float64), ("sigma2", np.float64)]
        parts, nulls = [[] for _ in range(y.shape[1])], [[] for _ in range(y.shape[1])]
        for g, t in zip(names, tables):
            mask = self._variant_masks([g], who, min_maf=min_maf).get(g)
            at = np.arange(len(t[0])) if mask is None else np.flatnonzero(mask.cpu().numpy())
            for k in range(y.shape[1]):
                null = null_of(g, k)
                stats, calls = (x.cpu().numpy() for x in scan_under_null(st, g, null, who, variant_mask=mask))
                rec = np.zeros(len(at), dtype=dtype)
                self._variant_columns(rec, t, width, at=at, pos=True)
                rec["n"] = calls[:, 0]
                with np.errstate(divide="ignore", invalid="ignore"):
                    rec["af"] = (calls[:, 1] + 2.0 * calls[:, 2]) / calls[:, 0] / 2.0
                for c, f in enumerate(floats):                   # (the statistics' columns in the records' order: MIXED_*)
                    rec[f] = stats[:, c]
                parts[k].append(rec)
                if loco or not nulls[k]:
                    chrom = (t[3][0][1] if t[3] else g).encode() if loco else b"*"
                    nulls[k].append(np.array([(chrom, null["h2"], null["sigma2"])], dtype=null_dtype))
        return ([np.concatenate(p) if p else np.zeros(0, dtype=dtype) for p in parts],
                [np.concatenate(x) if x else np.zeros(0, dtype=null_dtype) for x in nulls])

    def _burden_regions(self, who, regions):
        """regions (chrom, start, end, name), 0-based and half-open, any order -> (records, {group: rows}): one record per
        region in the order asked — name, chrom (without a leading "chr"), start, end, lo, hi (its variants [lo, hi) of the
        group: those whose start lies inside it) — and per group the rows of its regions.  KeyError for a chromosome the file
        lacks, ValueError for a region that is not four fields with 0 <= start <= end"""
        rows = []
        for k, r in enumerate(regions):
            r = tuple(r)
            if len(r) != 4:
                raise ValueError(f"{who}: region {k} is not (chrom, start, end, name)")
            chrom = r[0].decode() if isinstance(r[0], bytes) else str(r[0])
            name = r[3].decode() if isinstance(r[3], bytes) else str(r[3])
            start, end = int(r[1]), int(r[2])
            if not 0 <= start <= end:
                raise ValueError(f"{who}: region {name} [{start}, {end}) on {chrom}: need 0 <= start <= end")
            rows.append((chrom[3:] if chrom.startswith("chr") else chrom, start, end, name))
        wn = max([len(r[3].encode()) for r in rows] + [1])
        wc = max([len(r[0].encode()) for r in rows] + [1])
        rec = np.zeros(len(rows), dtype=[("name", f"S{wn}"), ("chrom", f"S{wc}"), ("start", np.int64), ("end", np.int64),
                                         ("lo", np.int64), ("hi", np.int64)])
        groups = {}
        for k, (chrom, start, end, name) in enumerate(rows):
            rec[k] = (name.encode(), chrom.encode(), start, end, 0, 0)
            groups.setdefault(self._group(self.store.samples[0] if self.store.samples else None, chrom), []).append(k)
        for g, at in groups.items():
            starts = self.store.variants(g)[0]
            for k in at:
                rec["lo"][k], rec["hi"][k] = _span(starts, rec["start"][k], rec["end"][k])
        return rec, groups

    def _burden(self, who_says, regions, donor_ids, max_maf, min_ac, weights, coding, impute, train_donor_ids, carriers=False):
        """burden's work -> (donors, B, records, carriers float64 device tensor [R] or None): per chromosome the mask of the
        regions' hull, GenotypeStore.burden, and with `carriers` the donors that carry an ALT allele in each region"""
        import torch
        st = self.store
        if weights is not None and weights != "beta":
            raise ValueError(f"{who_says}: weights {weights!r} (None: 1 per ALT allele, or \"beta\")")
        rec, groups = self._burden_regions(who_says, regions)
        _, donors, who = self._cohort([g[len("chr_"):] for g in groups], donor_ids)
        train = who if train_donor_ids is None else self._cohort([g[len("chr_"):] for g in groups], list(train_donor_ids))[2]
        ctx = st._context()
        B = torch.zeros((len(donors), len(rec)), dtype=torch.float64, device=ctx.device)
        n_used = np.zeros(len(rec), np.int64)
        carry = torch.zeros(len(rec), dtype=torch.float64, device=ctx.device) if carriers else None
        for g, at in groups.items():
            intervals = np.stack([rec["lo"][at], rec["hi"][at]], axis=1)
            full = intervals[intervals[:, 0] < intervals[:, 1]]
            mask = torch.zeros(st.meta["groups"][g]["n_variants"], dtype=torch.bool, device=ctx.device)
            if len(full):                                       # the mask of the regions' hull: nothing else is read
                lo, hi = int(full[:, 0].min()), int(full[:, 1].max())
                mask[lo:hi] = st.variant_mask(g, train, lo, hi, min_ac=min_ac, max_maf=max_maf)
            cols = self.store._to_device(np.array(at))
            scores, used = st.burden(g, intervals, weights, who, mask, coding, impute, freq_samples=train)
            B[:, cols] = scores[:, :, 0]
            n_used[at] = used.cpu().numpy()
            if carriers:
                c = scores if coding == "carrier" else st.burden(g, intervals, None, who, mask, "carrier", freq_samples=train)[0]
                carry[cols] = c[:, :, 0].sum(0)
        out = np.zeros(len(rec), dtype=[("name", rec.dtype["name"]), ("chrom", rec.dtype["chrom"]), ("start", np.int64),
                                        ("end", np.int64), ("n_variants", np.int64), ("n_used", np.int64)])
        for f in ("name", "chrom", "start", "end"):
            out[f] = rec[f]
        out["n_variants"], out["n_used"] = rec["hi"] - rec["lo"], n_used
        return donors, B, out, carry

    def burden(self, regions, donor_ids=None, max_maf=0.01, min_ac=1, weights=None, coding="additive", impute="mean",
               train_donor_ids=None):
        """region burden scores: one number per donor and region -> (donors, B, records).  regions: (chrom, start, end, name)
        rows, 0-based and half-open (a BED file's), in any order, overlapping or not; a region's variants are those whose
        start lies inside it; a chromosome the file lacks: KeyError.  B is a float64 device tensor [len(donors), R], row i
        for donor_ids[i] in the order asked (default: every sample, store order), column r for regions[r]:
        GenotypeStore.burden of the region's variants that pass variant_mask(max_maf=, min_ac=) — the rare ones: at most
        max_maf minor allele frequency and at least min_ac ALT alleles (None: no bound) —, with weights None (1 per ALT
        allele) or "beta" (SKAT's 25 (1 - maf)^24), coding "additive" or "carrier" and impute "mean" or "none" as there.
        With train_donor_ids the mask AND the frequencies (the weights' and the imputed calls') come from the training donors
        only, so held-out donors leak into neither; without it, from the donors asked for.  records: host numpy, one per
        region in the order asked: name, chrom, start, end, n_variants (variants inside the region), n_used (of them, those
        that pass the mask and have a called allele among the frequency donors)."""
        return self._burden("burden", regions, donor_ids, max_maf, min_ac, weights, coding, impute, train_donor_ids)[:3]

    def burden_association(self, regions, phenotypes, covariates=None, pcs=0, model="linear", donor_ids=None, max_maf=0.01,
                           min_ac=1, weights=None, coding="additive", impute="mean", train_donor_ids=None, pc_min_maf=None,
                           ld_window=None, ld_r2=0.2):
        """the test of every phenotype on every region's burden score -> a list with one host numpy record array per
        phenotype, one record per region in the order asked: burden's region columns (name, chrom, start, end, n_variants,
        n_used), carriers (the donors with a complete call that carries an ALT allele at a used variant of the region),
        then with model = "linear" beta, se, t, p — store.dense_assoc: the coefficient of the score in the least-squares
        fit of the phenotype on [1 | covariates | score] — and with model = "logistic" (0 / 1 phenotypes) score_chi2,
        score_p — store.dense_logistic_score: the score test at the null model; there is no Wald or Firth fit of a burden
        column.  NaN where the score is constant or explained by the covariates.  phenotypes is [n] or [n, P], covariates
        [n, q0] or None, both aligned with the donors; pcs = K appends the K components of principal_components over the
        donors and the regions' chromosomes (pc_min_maf, ld_window, ld_r2: its min_maf and LD pruning), as association
        does.  The other arguments are burden's."""
        self._check_burden_model(model)
        donors, B, rec, carriers = self._burden("burden_association", regions, donor_ids, max_maf, min_ac, weights, coding, impute,
                                                train_donor_ids, carriers=True)
        return self._burden_tests(donors, B, rec, carriers, phenotypes, covariates, pcs, model, donor_ids, pc_min_maf, ld_window, ld_r2)

    @staticmethod
    def _check_burden_model(model):
        if model not in ("linear", "logistic"):
            raise ValueError(f"burden_association: model {model!r} (\"linear\" or \"logistic\")")

    def _burden_tests(self, donors, B, rec, carriers, phenotypes, covariates=None, pcs=0, model="linear", donor_ids=None,
                      pc_min_maf=None, ld_window=None, ld_r2=0.2):
        """burden_association behind the scores: _burden's (donors, B, records, carriers) -> its list of record arrays"""
        self._check_burden_model(model)
        y = np.asarray(phenotypes, dtype=np.float64)
        y = y[:, None] if y.ndim == 1 else y
        cov = None if covariates is None else np.asarray(covariates, dtype=np.float64)
        if y.ndim != 2 or y.shape[0] != len(donors):
            raise ValueError(f"burden_association: phenotypes {list(y.shape)} for {len(donors)} donors ([n] or [n, P])")
        if int(pcs):
            chroms = list(dict.fromkeys(c.decode() for c in rec["chrom"]))
            pc_rec, _ = self.principal_components(int(pcs), chroms, donor_ids, pc_min_maf, ld_window, ld_r2)
            pc = np.stack([pc_rec[f"pc{c + 1}"] for c in range(int(pcs))], axis=1)
            cov = pc if cov is None else np.concatenate([cov, pc], axis=1)
        up = self.store._to_device
        if model == "linear":
            floats = ("beta", "se", "t", "p")
            W, q, yy = assoc_design(y, cov)
            stats = dense_assoc(B, up(W), q, up(yy)).cpu().numpy()                     # [R, P, 4]
        else:
            floats = ("score_chi2", "score_p")
            per = []
            for k in range(y.shape[1]):
                X, beta0 = logistic_design(y[:, k], cov)
                W, XWX = logistic_score_design(X, y[:, k], beta0)
                per.append(dense_logistic_score(B, up(W), X.shape[1], up(XWX)))
            stats = np.stack([x.cpu().numpy() for x in per], axis=1)                   # [R, P, 2]
        dtype = rec.dtype.descr + [("carriers", np.int64)] + [(f, np.float64) for f in floats]
        out = []
        for k in range(y.shape[1]):
            r = np.zeros(len(rec), dtype=dtype)
            for f in rec.dtype.names:
                r[f] = rec[f]
            r["carriers"] = carriers.cpu().numpy().astype(np.int64)
            for c, f in enumerate(floats):
                r[f] = stats[:, k, c]
            out.append(r)
        return out

    def close(self):
        pass
