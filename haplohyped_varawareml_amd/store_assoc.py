"""GenotypeStore's association scans: the sums over samples behind them, the linear scan, the case / control scan."""
import numpy as np

from .store_stats import (ASSOC_MAX_COLS, LOGIT_REC, assoc_design, assoc_from_sums, logistic_design, logistic_from_fit,
                          logistic_score_design, logistic_score_from_sums)


class AssocQueries:
    """Methods of GenotypeStore, stateless; rows from _variant_rows: cached chunks used, the read cache neither filled nor evicted."""

    def _design_rows(self, who, idx):
        """the samples idx as the rows of `who`'s design: ValueError unless they are distinct -> (rows: the plane row of
        each, on the host; sw: the words of a row of bits; scattered(a): a [n, ...], host or device -> float64 zeros
        [32 sw, ...] on the device with a's rows at those plane rows).  Called behind the other checks: it uses the device."""
        import torch
        if len(np.unique(idx)) != len(idx):
            raise ValueError(f"{who}: a sample is listed twice")
        n_rows, rows = self._plane_rows(idx)
        sw, d_rows = -(-n_rows // 32), self._to_device(rows)

        def scattered(a):
            out = torch.zeros((32 * sw,) + tuple(a.shape[1:]), dtype=torch.float64, device=d_rows.device)
            out[d_rows] = self._to_device(a if torch.is_tensor(a) else np.asarray(a, dtype=np.float64))
            return out
        return rows, sw, scattered

    def assoc_sums(self, group, W, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None, plane_bytes=None):
        """the sums over samples behind an association scan of a group: a float64 device tensor [n_counted, 3, C] — for
        counted variant v (those of [v_lo, v_hi) that variant_mask marks, in order, as in ld_counts), plane k (ASSOC_HET,
        ASSOC_COMPLETE, ASSOC_ALT: the call is HET, complete, HOM_ALT) and column c, the sum of W[i, c] over the samples i
        whose call at v is of that class.  W: float64 [len(samples), C], host or device, 1 <= C <= 64, row i for
        samples[i] (names or indices; None: every sample, store order).  The samples must be distinct — a regression has
        no use for a row counted twice —: ValueError before anything is allocated.  W is scattered once to the plane
        rows of the samples (zeros elsewhere); the rows of bits come as in ld_counts (hhgt_genotype_planes, then
        hhgt_variant_planes per plane window: slab_bytes and plane_bytes mean what they mean there), and every window is
        reduced by one hhgt_assoc_sums call (the f64 MFMA; include/hhgt.h states its arithmetic: sums of exactly
        representable partial sums are exact).  No genotype and no dosage is written anywhere."""
        import torch
        idx = self._query("assoc_sums", group, samples, v_lo, v_hi, variant_mask, single=True)[0]
        W = W if torch.is_tensor(W) else torch.from_numpy(np.ascontiguousarray(W))
        if W.dtype != torch.float64 or W.dim() != 2 or W.shape[0] != len(idx) or not 1 <= W.shape[1] <= ASSOC_MAX_COLS:
            raise ValueError(f"assoc_sums: W must be float64 [{len(idx)}, 1 to {ASSOC_MAX_COLS}], not {W.dtype} {list(W.shape)}")
        _, _, scattered = self._design_rows("assoc_sums", idx)
        _, _, _, n, vrows = self._variant_rows("assoc_sums", group, idx, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes,
                                               "assoc_plane_blocks")
        d_w = scattered(W)
        parts = [self._context().assoc_sums(v, d_w) for v in vrows]
        self.stats["assoc_variants"] += n
        # (without a sample there is no row of bits: every sum is 0)
        return torch.cat(parts) if parts else torch.zeros((n, 3, W.shape[1]), dtype=torch.float64, device=d_w.device)

    def assoc(self, group, y, covariates=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None,
              plane_bytes=None):
        """single-variant linear regression scan of a group -> (stats, calls) on the device: assoc_design(y, covariates)
        on the host (y [n] or [n, P], covariates [n, q0] or None, row i for samples[i]), assoc_sums of its W (same
        remaining arguments), assoc_from_sums.  stats is float64 [n_counted, P, 4] — ASSOC_BETA, ASSOC_SE, ASSOC_T, ASSOC_P
        of the dosage's coefficient in the fit of each phenotype on [1 | covariates | dosage], a call that is not
        complete imputed to the variant's mean dosage; NaN where the variant is not tested —, calls int64 [n_counted, 3]:
        complete, HET, HOM_ALT calls.  The formulas of assoc_from_sums are the contract; plink2's .glm.linear is not."""
        W, q, yy = assoc_design(y, covariates)
        T = self.assoc_sums(group, W, samples, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes)
        return assoc_from_sums(T, self._to_device(W.sum(axis=0)), q, self._to_device(yy))

    def assoc_logistic(self, group, y, covariates=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, test="wald",
                       slab_bytes=None, plane_bytes=None):
        """case / control scan of a group: per counted variant and phenotype, the logistic regression of a 0 / 1 phenotype
        on [1 | covariates | dosage] -> (stats, calls, info) on the device.  y is [n] or [n, P] (every value 0 or 1),
        covariates [n, q0] or None, row i for samples[i]; every phenotype gets its own logistic_design (host), and the
        planes of a window — produced as in assoc_sums: same samples, v_lo / v_hi, variant_mask, slab_bytes, plane_bytes,
        the read cache neither filled nor evicted — are made once and fitted P times.  test = "wald": hhgt_logistic_fit
        (Newton's method per variant on the device; logistic_fit_reference is the contract) and logistic_from_fit;
        test = "score": hhgt_assoc_sums of logistic_score_design's columns and logistic_score_from_sums — the score test
        alone, no iteration, the four Wald columns NaN.  stats is float64 [n_counted, P, 6], columns LOGIT_BETA, LOGIT_SE,
        LOGIT_Z, LOGIT_P, LOGIT_SCORE_CHI2, LOGIT_SCORE_P, a call that is not complete imputed to the variant's mean dosage,
        NaN where the variant is not tested; calls int64 [n_counted, 3]: complete, HET, HOM_ALT calls; info int64
        [n_counted, P, 2]: Newton steps and status (LOGIT_TESTED ... LOGIT_NOT_CONVERGED).  The samples must be distinct:
        ValueError before anything is allocated, as for a y that is not 0 / 1 or a design logistic_design refuses."""
        import torch
        if test not in ("wald", "score"):
            raise ValueError(f"assoc_logistic: test {test!r} (\"wald\" or \"score\")")
        idx = self._query("assoc_logistic", group, samples, v_lo, v_hi, variant_mask, single=True)[0]
        Y = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
        Y = Y[:, None] if Y.ndim == 1 else Y
        if Y.ndim != 2 or Y.shape[0] != len(idx):
            raise ValueError(f"assoc_logistic: y of shape {Y.shape} for {len(idx)} samples ([n] or [n, P])")
        designs = [logistic_design(Y[:, p], covariates) for p in range(Y.shape[1])]
        rows, sw, scattered = self._design_rows("assoc_logistic", idx)
        ctx = self._context()
        _, _, _, n, vrows = self._variant_rows("assoc_logistic", group, idx, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes,
                                               "assoc_plane_blocks")
        if test == "wald":
            bits = np.zeros(32 * sw, dtype=np.uint8)
            bits[rows] = 1
            valid = self._to_device(np.packbits(bits, bitorder="little").view(np.int32))
            args = [(valid, scattered(X), scattered(Y[:, p]), self._to_device(beta0)) for p, (X, beta0) in enumerate(designs)]
            fit = lambda v, a: ctx.logistic_fit(v, *a)
            finish = [logistic_from_fit] * len(designs)
        else:
            score = [logistic_score_design(X, Y[:, p], beta0) for p, (X, beta0) in enumerate(designs)]
            args = [scattered(W) for W, _ in score]
            fit = ctx.assoc_sums
            finish = [lambda T, W=W, XWX=XWX: logistic_score_from_sums(T, self._to_device(W.sum(axis=0)), XWX.shape[0],
                                                                        self._to_device(XWX)) for W, XWX in score]
        parts = [[fit(v, a) for a in args] for v in vrows]
        self.stats["logistic_variants"] += n * len(designs)
        if not parts:               # (no counted variant: a design has samples, so every counted variant has a row of bits)
            shape = (0, LOGIT_REC) if test == "wald" else (0, 3, args[0].shape[1])
            parts = [[torch.zeros(shape, dtype=torch.float64, device=ctx.device)] * len(designs)]
        out = [finish[p](torch.cat([w[p] for w in parts])) for p in range(len(designs))]
        return torch.stack([o[0] for o in out], 1), out[0][1], torch.stack([o[2] for o in out], 1)
