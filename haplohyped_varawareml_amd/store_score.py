"""GenotypeStore's per-sample sums of per-variant weights: polygenic scores, PC projection, region sums, burden scores."""
import numpy as np

from .store_plan import REGION_MAX_COLS, plan_regions
from .store_stats import (AN, SCORE_MAX_COLS, beta_density_weights, burden_class_weights, loadings_from_sums,
                          projection_class_weights, region_totals, score_class_weights)


def _weights_arg(text, weights, lead, max_cols, optional=False, shown=True, same=None):
    """weights, host array or tensor, checked -> (w, K): float64 lead + (K,), 1 <= K <= max_cols, K == same if given; optional:
    a missing last axis means K = 1 and w gets it (shown: and so does the shape in the message).  Else ValueError(text ...)."""
    import torch
    w = weights if torch.is_tensor(weights) else np.asarray(weights)
    given = shape = tuple(int(x) for x in w.shape)
    if optional and len(shape) == len(lead):
        w, shape = w[..., None], shape + (1,)
    if (str(w.dtype).split(".")[-1] != "float64" or len(shape) != len(lead) + 1 or shape[:-1] != tuple(lead)
            or not 1 <= shape[-1] <= max_cols or same not in (None, shape[-1])):
        raise ValueError(f"{text}, not {w.dtype} {list(shape if shown else given)}")
    return w, shape[-1]


class ScoreQueries:
    """Methods of GenotypeStore, stateless; planes from _plane_walk: cached chunks used, the read cache neither filled nor evicted."""

    def _score_weights(self, who, weights, groups, samples, v_lo, v_hi, variant_mask, inner):
        """score_sums' and score's (`who`) start: `weights` — one array for one group or a dict group -> array (groups = None:
        its keys, in order), each float64 with the axes `inner` ("3VK" or "VK": V the group's range) — against _query ->
        (idx, queries, {group: host array or tensor}, K); KeyError for a listed group without weights; no device work."""
        if isinstance(weights, dict) and groups is None:
            groups = list(weights)
        idx, queries = self._query(who, groups, samples, v_lo, v_hi, variant_mask)
        if not isinstance(weights, dict):
            if len(queries) != 1:
                raise ValueError(f"{who}: one array of weights needs a single group (several: a dict group -> array)")
            weights = {queries[0][0]: weights}
        out, K = {}, None
        for group, lo, hi, _, _ in queries:
            if group not in weights:
                raise KeyError(group)
            want = (3, hi - lo) if inner == "3VK" else (hi - lo,)
            out[group], K = _weights_arg(f"{who}: the weights of {group} must be float64 {list(want)} + [K], 1 <= K <= "
                                         f"{SCORE_MAX_COLS}, the same K in every group", weights[group], want, SCORE_MAX_COLS,
                                         optional=inner == "VK", same=K)
        if K is None:
            raise ValueError(f"{who}: no group")
        return idx, queries, out, K

    def score_sums(self, weights, groups=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None,
                   plane_bytes=None):
        """per-sample sums of per-variant weights over the variants of `groups`: a float64 device tensor [len(samples), K],
        row i for samples[i] (names or indices; None = every sample in store order; a sample named twice gets its row
        twice) — the sum over the counted variants v at which the sample's call is complete, of weights[d, v, :] for the
        call's dosage d (0 HOM_REF, 1 HET, 2 HOM_ALT); a call that is not complete contributes nothing.  weights: float64
        [3, v_hi - v_lo, K], host or device, 1 <= K <= 64, for one group, or a dict group -> such an array over the whole
        group (groups = None: the dict's keys, in order); KeyError for a listed group without weights, ValueError for a
        shape or dtype that does not fit, before anything is allocated.  groups, samples, v_lo / v_hi, variant_mask,
        slab_bytes and plane_bytes mean what they mean in pair_counts; a variant the mask leaves out has no bit and its
        weights are not read, the others' must be finite.  Per plane window (_plane_walk: hhgt_genotype_planes under the
        packed mask) the window's weights are scattered to its bit positions and one hhgt_score_sums call (the f64 MFMA;
        include/hhgt.h states its arithmetic: sums of exactly representable partial sums are exact) adds to one table
        [plane rows, K]; groups, windows and slabs add into it and the samples' rows are picked at the end.  No genotype
        and no dosage is written anywhere."""
        import torch
        idx, queries, weights, K = self._score_weights("score_sums", weights, groups, samples, v_lo, v_hi, variant_mask, "3VK")
        ctx = self._context()
        n_rows, rows = self._plane_rows(idx)
        table = torch.zeros((n_rows, K), dtype=torch.float64, device=ctx.device)
        for group, lo, hi, n_var, mask in queries if len(idx) else ():
            w, mask, packed = self._masked(self._to_device(weights[group]), mask, lo, n_var)
            for a, b, words, planes in self._plane_walk(group, idx, lo, hi, n_var, "score_plane_blocks", slab_bytes,
                                                        plane_bytes, packed):
                ctx.score_sums(planes, self._window_values(w, lo, a, b, words), 0, words, sums=table)
            self.stats["score_variants"] += hi - lo if mask is None else int(mask.sum())
        return table[self._to_device(rows)]

    def score(self, betas, groups=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None, plane_bytes=None,
              impute="mean", freq_samples=None):
        """polygenic scores of `samples` -> (scores, used): scores a float64 device tensor [len(samples), K], used a dict
        group -> the number of its variants that took part.  betas: float64 [v_hi - v_lo, K] (or [v_hi - v_lo]: K = 1), host
        or device, the effect per ALT allele, for one group, or a dict group -> such an array over the whole group; the
        other arguments up to plane_bytes mean what they mean in score_sums.  Per group, allele_counts over freq_samples
        (default: the scored samples, each once) and score_class_weights (impute "mean" or "none") give the class weights,
        the offset and the variants used; scores = score_sums of the weights + the offsets.  With "mean" that is, per
        sample, the sum over the used variants of beta x (the dosage, or twice the ALT frequency among freq_samples where
        the call is not complete); a variant without a called allele among freq_samples is not used.  A variant the mask
        leaves out takes part in nothing.  score_class_weights' formulas are the contract: these are sums, not plink2
        --score's per-allele averages."""
        import torch
        idx, queries, betas, K = self._score_weights("score", betas, groups, samples, v_lo, v_hi, variant_mask, "VK")
        if impute not in ("mean", "none"):
            raise ValueError(f"score: impute {impute!r} (\"mean\" or \"none\")")
        freq = self._freq_samples("score", idx, queries[0][0], freq_samples)
        weights, masks, used_n = {}, {}, {}     # masks: group -> bool device tensor or None, a dict as score_sums takes it
        offset = torch.zeros(K, dtype=torch.float64, device=self._context().device)
        for group, lo, hi, n_var, mask in queries:
            beta, masks[group], _ = self._masked(self._to_device(betas[group]), mask)
            weights[group], off, used = score_class_weights(beta, self.allele_counts(group, freq, lo, hi, slab_bytes), impute)
            offset += off
            used_n[group] = int((used if mask is None else used & masks[group]).sum())
        lo, hi = queries[0][1:3] if len(queries) == 1 else (0, None)
        sums = self.score_sums(weights, [q[0] for q in queries], idx, lo, hi, masks, slab_bytes, plane_bytes)
        return sums + offset[None, :], used_n

    def _regions_arg(self, who, group, regions):
        """`regions` as int64 [R, 2] variant intervals [lo, hi) of a group, clipped to it (an interval the wrong way round
        is empty) -> (regions, lo, hi): the hull [lo, hi) of the non-empty ones, (0, 0) without one"""
        n_var = self.meta["groups"][group]["n_variants"]
        r = np.asarray(regions)
        if r.ndim != 2 or r.shape[1] != 2 or r.dtype.kind not in "iu":
            raise ValueError(f"{who}: regions must be integer [R, 2] variant intervals [lo, hi), not {r.dtype} {list(r.shape)}")
        r = np.clip(r.astype(np.int64), 0, n_var)
        full = r[r[:, 0] < r[:, 1]]
        return r, (int(full[:, 0].min()), int(full[:, 1].max())) if len(full) else (0, 0)

    def region_sums(self, group, regions, weights, samples=None, variant_mask=None, slab_bytes=None, plane_bytes=None,
                    max_table_bytes=None):
        """score_sums cut at the boundaries of regions: a float64 device tensor [len(samples), R, K], entry [i, r] the
        sum over the counted variants v of region r at which samples[i]'s call is complete, of weights[d, v, :] for the
        call's dosage d — one number per sample and region (a gene, a window of a tiling) and column, from ONE pass over
        the planes however many regions there are.  regions: integer [R, 2] variant intervals [lo, hi) of `group`, in
        any order, overlapping, repeated or empty (an empty one gives zeros), clipped to the group.  weights: float64
        [3, n_variants, K], or [3, n_variants] for K = 1, host or device, 1 <= K <= 16, over the whole group; finite at
        the counted variants of the regions.  samples, variant_mask (one mask over the whole group), slab_bytes and
        plane_bytes mean what they mean in score_sums; a sample named twice gets its row twice.  ValueError before
        anything is allocated for a shape or dtype that does not fit and for a table [plane rows, R, K] of more than
        max_table_bytes (default MAX_PAIR_TABLE_BYTES).  Per plane window of the regions' hull (_plane_walk under the
        packed mask) the weights are scattered to their bit positions, zeros where the mask leaves a variant out, the
        regions become pieces (store_plan.plan_regions: cut every REGION_SPAN words from a region's own first word, so a
        region's sums do not depend on the others) and one hhgt_region_sums call adds into the table; a region across
        two windows adds from both.  include/hhgt.h states the arithmetic: exact where every partial sum is representable."""
        import torch
        idx, [(group, _, _, n_var, mask)] = self._query("region_sums", group, samples, 0, None, variant_mask, single=True)
        regions, (lo, hi) = self._regions_arg("region_sums", group, regions)
        w, K = _weights_arg(f"region_sums: the weights of {group} must be float64 [3, {n_var}] + [K], 1 <= K <= {REGION_MAX_COLS}",
                            weights, (3, n_var), REGION_MAX_COLS, optional=True)
        R = len(regions)
        n_rows, rows = self._plane_rows(idx)
        self._table_budget("region_sums", f"a table of {n_rows} rows x {R} regions x {K} columns ({{}} bytes) exceeds",
                           n_rows * R * K * 8, max_table_bytes)
        ctx = self._context()
        table = torch.zeros((n_rows, R, K), dtype=torch.float64, device=ctx.device)
        if len(idx) and hi > lo:
            full = regions[regions[:, 0] < regions[:, 1]]
            covered = np.zeros(hi - lo + 1, np.int64)           # the variants of the hull that lie in at least one region
            np.add.at(covered, full[:, 0] - lo, 1)
            np.add.at(covered, full[:, 1] - lo, -1)
            covered = self._to_device(np.cumsum(covered)[:-1] > 0)
            w, mask, packed = self._masked(self._to_device(w[:, lo:hi]), None if mask is None else self._device_bool(mask)[lo:hi],
                                           lo, n_var)
            bs = self._blocksize()
            for a, b, words, planes in self._plane_walk(group, idx, lo, hi, n_var, "region_plane_blocks", slab_bytes,
                                                        plane_bytes, packed):
                pieces, runs, n_slots = plan_regions(regions, a, b, bs)
                ctx.region_sums(planes, self._window_values(w, lo, a, b, words), pieces, runs, n_slots, R, sums=table, wait=False)
                self.stats["region_pieces"] += len(pieces)
            self.stats["region_variants"] += int((covered if mask is None else covered & mask).sum())
        return table[self._to_device(rows)]

    def burden(self, group, regions, weights=None, samples=None, variant_mask=None, coding="additive", impute="mean",
               freq_samples=None, slab_bytes=None, plane_bytes=None, max_table_bytes=None):
        """region burden scores of `samples` -> (B, used): B a float64 device tensor [len(samples), R, K], one number per
        sample, region and weight column — the (rare) variants of a region collapsed into one score, which has far more
        carriers than any of them —, used an int64 device tensor [R]: the variants of each region that variant_mask marks
        and that have a called allele (AN > 0) among freq_samples (default: the scored samples, each once).  regions,
        samples, variant_mask and the budgets as in region_sums.  weights, per ALT allele: None — 1; a float64 array [V]
        or [V, K] over the whole group, host or device, K <= 16; "beta" — 25 (1 - maf)^24, SKAT's Beta(1, 25) density at
        maf = min(p, 1 - p), p = AC / AN among freq_samples (store_stats.beta_density_weights).
        coding "additive": store_stats.burden_class_weights (impute "mean" or "none") gives the class weights Wd and the
        per-variant offsets o, and B = region_sums(Wd) + region_totals(o): per sample and region the sum over the used,
        marked variants of weight x (the ALT dosage, or 2p where the call is not complete — p from freq_samples alone, so
        rows held out of them leak nothing); with "none" a call that is not complete counts 0.  coding "carrier": the CMC
        collapse, 1.0 where the sample has a complete call with an ALT allele at a used, marked variant of the region and
        0.0 elsewhere; it takes no weights (ValueError).  The counted alleles are ALT alleles: nothing is flipped to the
        minor one.  Those formulas are the contract, not REGENIE's or plink2's files."""
        import torch
        if coding not in ("additive", "carrier"):
            raise ValueError(f"burden: coding {coding!r} (\"additive\" or \"carrier\")")
        if impute not in ("mean", "none"):
            raise ValueError(f"burden: impute {impute!r} (\"mean\" or \"none\")")
        if coding == "carrier" and weights is not None:
            raise ValueError("burden: coding \"carrier\" takes no weights")
        idx, [(group, _, _, n_var, mask)] = self._query("burden", group, samples, 0, None, variant_mask, single=True)
        regions, (lo, hi) = self._regions_arg("burden", group, regions)
        named, K = isinstance(weights, str), 1
        if named and weights != "beta":
            raise ValueError(f"burden: weights {weights!r} (None, \"beta\" or an array)")
        if weights is not None and not named:
            w, K = _weights_arg(f"burden: the weights of {group} must be float64 [{n_var}] or [{n_var}, K], 1 <= K <= "
                                f"{REGION_MAX_COLS}", weights, (n_var,), REGION_MAX_COLS, optional=True, shown=False)
        n_rows = self._plane_rows(idx)[0]
        self._table_budget("burden", f"a table of {n_rows} rows x {len(regions)} regions x {K} columns ({{}} bytes) exceeds",
                           n_rows * len(regions) * K * 8, max_table_bytes)
        freq = self._freq_samples("burden", idx, group, freq_samples)
        ctx = self._context()
        # the allele counts of the regions' hull, zeros (AN == 0: not used) in the rest of the group
        counts = torch.zeros((n_var, 4), dtype=torch.int32, device=ctx.device)
        if hi > lo:
            counts[lo:hi] = self.allele_counts(group, freq, lo, hi, slab_bytes)
        marked, mask, _ = self._masked((counts[:, AN] > 0).to(torch.float64)[:, None], mask)     # [V, 1]: used and marked
        used = region_totals(marked, regions)[:, 0].to(torch.int64)
        if coding == "carrier":
            Wd = torch.stack([torch.zeros(n_var, dtype=torch.float64, device=ctx.device)] + [marked[:, 0]] * 2)
            sums = self.region_sums(group, regions, Wd, idx, mask, slab_bytes, plane_bytes, max_table_bytes)
            return (sums > 0).to(torch.float64), used
        if weights is None:
            w = torch.ones((n_var, 1), dtype=torch.float64, device=ctx.device)
        elif named:
            w = beta_density_weights(counts)[:, None]
        Wd, o, _ = burden_class_weights(self._to_device(w), counts, impute)
        sums = self.region_sums(group, regions, Wd.contiguous(), idx, mask, slab_bytes, plane_bytes, max_table_bytes)
        return sums + region_totals(self._masked(o, mask)[0], regions)[None], used

    def projection_weights(self, vectors, values, groups=None, samples=None, variant_mask=None, slab_bytes=None,
                           plane_bytes=None):
        """the class weights that project a sample onto principal components fitted on `samples` (the TRAINING samples:
        names or indices, distinct; None = every sample) -> a dict group -> float64 device tensor [3, n_variants, k], what
        score_sums takes.  vectors float64 [len(samples), k] and values [k] are pca's (or top_eigenpairs') over the same
        samples, groups and variant_mask.  Per group: allele_counts over the samples -> standardized_dosages' z and used;
        assoc_sums of the vectors over the variants that are used and that the mask marks -> loadings_from_sums, with
        n_variants the number of such variants over all groups -> projection_class_weights, scattered to the group's
        variants (zeros elsewhere).  ValueError if no variant is used, an eigenvalue is not positive or the shapes
        disagree."""
        import torch
        idx, queries = self._query("projection_weights", groups, samples, 0, None, variant_mask)
        vectors = np.ascontiguousarray(vectors.detach().cpu().numpy() if torch.is_tensor(vectors) else vectors)
        if vectors.dtype != np.float64 or vectors.ndim != 2 or vectors.shape[0] != len(idx) or len(np.reshape(values, -1)) != vectors.shape[1]:
            raise ValueError(f"projection_weights: vectors must be float64 [{len(idx)}, k] with k values, "
                             f"not {vectors.dtype} {list(vectors.shape)}")
        fitted = [self._dosages(group, idx, lo, hi, mask, slab_bytes) for group, lo, hi, _, mask in queries]
        n_variants = sum(int(used.sum()) for _, used in fitted)
        if n_variants == 0:
            raise ValueError("projection_weights: no variant is used")
        out = {}
        for (group, lo, hi, n_var, _), (z, used) in zip(queries, fitted):
            T = self.assoc_sums(group, vectors, idx, lo, hi, used, slab_bytes, plane_bytes)
            counted = torch.nonzero(used).reshape(-1)
            zc = z[:, counted]
            Wd = torch.zeros((3, n_var, vectors.shape[1]), dtype=torch.float64, device=T.device)
            Wd[:, counted] = projection_class_weights(zc, loadings_from_sums(T, zc, values, n_variants))
            out[group] = Wd
        return out

    def project(self, vectors, values, train_samples, samples, groups=None, variant_mask=None, slab_bytes=None, plane_bytes=None):
        """the components of `samples` on principal components fitted on train_samples: score_sums(projection_weights(
        vectors, values, groups, train_samples, variant_mask), samples = samples, variant_mask = variant_mask) -> a float64
        device tensor [len(samples), k].  This is how held-out samples get components without entering the fit: fit
        (pca) on the training samples, project the rest.  A training sample with no incomplete call gets back its own
        eigenvector entry, up to the relationship matrix's f32-chain error (hhgt_grm) passed through the decomposition.
        With incomplete calls it differs, in the order of the missing rate, because the relationship matrix divides each
        pair's sum by the number of its jointly complete variants while the loadings divide by the number of variants; no
        shrinkage correction is attempted either."""
        Wd = self.projection_weights(vectors, values, groups, train_samples, variant_mask, slab_bytes, plane_bytes)
        return self.score_sums(Wd, list(Wd), samples, 0, None, variant_mask, slab_bytes, plane_bytes)
