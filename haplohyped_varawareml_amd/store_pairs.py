"""GenotypeStore's queries over pairs of samples: pairwise counts and kinship, the relationship matrix and its components."""
from .store_stats import NSNP, check_components, grm_from_sums, kinship_from_counts, top_eigenpairs


class PairQueries:
    """Methods of GenotypeStore, stateless; planes from _plane_walk: cached chunks used, the read cache neither filled nor evicted."""

    def _pair_query(self, who, groups, samples, v_lo, v_hi, variant_mask, bytes_per_pair, max_table_bytes):
        """pair_counts' and grm_sums' (`who`) start: _query, the plane rows, the budget of their tables of bytes_per_pair
        per pair of plane rows -> (idx, queries, n_rows, pick: a table [n_rows, n_rows, ...] -> the samples' part of it)"""
        idx, queries = self._query(who, groups, samples, v_lo, v_hi, variant_mask)
        n_rows, rows = self._plane_rows(idx)
        what = ("a table of {0} x {0} pairs ({{}} bytes) exceeds" if bytes_per_pair == 16 else
                "tables of {0} x {0} pairs ({{}} bytes) exceed").format(n_rows)
        self._table_budget(who, what, n_rows * n_rows * bytes_per_pair, max_table_bytes)
        rows = self._to_device(rows)
        return idx, queries, n_rows, lambda table: table[rows][:, rows].contiguous()

    def pair_counts(self, groups=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None,
                    plane_bytes=None, max_table_bytes=None):
        """pairwise counts over the variants of `groups`: an int32 device tensor [n, n, 4], columns NSNP, HETHET, IBS0, HET1
        (module constants) for the ordered pair (samples[i], samples[j]) — variants at which both calls are complete
        (both alleles 0 or 1), both heterozygous, opposite homozygotes, i heterozygous and j complete; a sample named twice
        appears twice and pairs with itself as a duplicate.  groups, samples, v_lo / v_hi, variant_mask and slab_bytes mean
        what they mean in sample_counts, and the chunks are handled the same way (cached ones used, the read cache neither
        filled nor evicted).  Two kernels: hhgt_genotype_planes decodes the selected rows' Blosc blocks into three bits per
        call (HET, HOM_REF, HOM_ALT planes; no genotype is written), hhgt_pair_counts reduces the planes pair by pair.  A
        group's range is walked in windows of whole Blosc blocks whose plane buffer is at most plane_bytes (default 1 GiB);
        groups, windows and slabs add into one table.  Plane rows are kept for the chunk rows that hold a listed sample
        only.  ValueError, before anything is allocated, if the table (16 bytes per pair of plane rows) would exceed
        max_table_bytes (default 2 GiB)."""
        import torch
        idx, queries, n_rows, pick = self._pair_query("pair_counts", groups, samples, v_lo, v_hi, variant_mask, 16, max_table_bytes)
        ctx = self._context()
        table = torch.zeros((n_rows, n_rows, 4), dtype=torch.int32, device=ctx.device)
        for group, lo, hi, n_var, mask in queries:
            for _, _, words, planes in self._plane_walk(group, idx, lo, hi, n_var, "pair_plane_blocks", slab_bytes,
                                                        plane_bytes, self._device_mask(mask, lo, n_var)):
                ctx.pair_counts(planes, 0, words, table=table)
                self.stats["pair_words"] += words
        return pick(table)

    def kinship(self, groups=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None, plane_bytes=None,
                max_table_bytes=None):
        """KING-robust kinship of every pair of `samples` from pair_counts (same arguments): a float64 device tensor [n, n],
        kinship_from_counts' formula — NaN where a pair has no heterozygous call to divide by, exactly 0.5 for a sample
        against itself or a duplicate.  The formula there is the contract; plink2's KINSHIP column is not."""
        return kinship_from_counts(self.pair_counts(groups, samples, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes,
                                                    max_table_bytes))

    def grm_sums(self, groups=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None, plane_bytes=None,
                 max_table_bytes=None):
        """the sums behind the genetic relationship matrix of `samples` over the variants of `groups` -> (S, N) on the
        device: S float64 [n, n], the sum over the variants of x_i * x_j, and N int32 [n, n], the variants at which both
        calls are complete (pair_counts' NSNP).  Every argument means what it means in pair_counts, a sample named twice
        included.  Per group, allele_counts over the listed samples (each counted once, as variant_mask counts them)
        gives standardized_dosages' z and `used`; the variants that take part are those variant_mask marks and that are
        used (ANDed on the device, and handed to the plane walk as its packed mask); a complete call of dosage d contributes
        x = z[d] of its variant, any other call 0.  Each plane window is reduced twice while it is resident, by
        hhgt_pair_counts and by hhgt_grm (the f32-input MFMA over the planes, z scattered to the window's bit positions:
        include/hhgt.h states its arithmetic and error bound); groups, windows and slabs add into the same two tables.
        ValueError, before anything is allocated, if the two tables (16 + 8 bytes per pair of plane rows) would exceed
        max_table_bytes (default 2 GiB)."""
        import torch
        idx, queries, n_rows, pick = self._pair_query("grm_sums", groups, samples, v_lo, v_hi, variant_mask, 24, max_table_bytes)
        ctx = self._context()
        counts = torch.zeros((n_rows, n_rows, 4), dtype=torch.int32, device=ctx.device)
        sums = torch.zeros((n_rows, n_rows), dtype=torch.float64, device=ctx.device)
        for group, lo, hi, n_var, mask in queries if n_rows else ():
            z, used = self._dosages(group, idx, lo, hi, mask, slab_bytes)
            for a, b, words, planes in self._plane_walk(group, idx, lo, hi, n_var, "grm_plane_blocks", slab_bytes,
                                                        plane_bytes, self._device_mask(used, lo, n_var)):
                d_z = self._window_values(z, lo, a, b, words)
                ctx.pair_counts(planes, 0, words, table=counts)
                ctx.grm(planes, d_z, 0, words, table=sums)
                self.stats["grm_words"] += words
        return pick(sums), pick(counts[..., NSNP])

    def grm(self, groups=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None, plane_bytes=None,
            max_table_bytes=None):
        """the standardised genetic relationship matrix of `samples`: grm_from_sums of grm_sums (same arguments) — a
        float64 device tensor [n, n], exactly symmetric, NaN where a pair has no jointly complete variant.  The formulas
        there are the contract; GCTA's and plink2 --make-rel's files are not."""
        return grm_from_sums(*self.grm_sums(groups, samples, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes,
                                            max_table_bytes))

    def pca(self, k, groups=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None, plane_bytes=None,
            max_table_bytes=None):
        """the k largest principal components of grm (same arguments after k) -> (values float64 [k], vectors float64
        [n, k]), host numpy arrays: top_eigenpairs of the host copy of the matrix — numpy.linalg.eigh, descending, unit
        vectors whose component of largest magnitude is positive.  The decomposition runs on the host on purpose: it is
        n^3 on an n x n matrix, not the hot path, and needs no solver library on the device.  ValueError if k is outside
        1..n (before anything is computed) or a pair of samples has no jointly complete variant."""
        samples = None if samples is None else list(samples)
        check_components(k, len(self.samples) if samples is None else len(samples))
        g = self.grm(groups, samples, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes, max_table_bytes)
        return top_eigenpairs(g.cpu().numpy(), k)
