"""GenotypeStore's queries over nearby variants: LD counts and r^2, greedy LD pruning, LD clumping."""
import numpy as np

from .store_plan import LD_MIN_TILE
from .store_stats import clump_rank, r2_from_counts


class LdQueries:
    """Methods of GenotypeStore, stateless; rows from _variant_rows: cached chunks used, the read cache neither filled nor evicted."""

    def _ld_rows(self, who, group, window, r2, *selection):
        """what the LD queries (`who`, for the messages) do alike.  The checks, in this order: r2 in 0..1 (None: the query
        takes none), the group a string and a group of this store, window in 1..1024 -> (int(window), float(r2) or None)
        and, given a selection (samples, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes), what _variant_rows returns"""
        window, r2 = int(window), None if r2 is None else float(r2)
        if r2 is not None and not 0.0 <= r2 <= 1.0:
            raise ValueError(f"{who}: r2 {r2} (0 to 1)")
        if not isinstance(group, str) or group not in self.meta["groups"]:
            raise KeyError(group)
        if not 1 <= window <= 1024:
            raise ValueError(f"{who}: window {window} (1 to 1024)")
        return (window, r2) + (self._variant_rows(who, group, *selection, "ld_plane_blocks") if selection else ())

    @staticmethod
    def _ld_pairs(n, window):
        """pairs (k, k + 1 + d), d < window, among n variants"""
        return n * (n - 1) // 2 if n <= window else n * window - window * (window + 1) // 2

    def _ld_tiles(self, rows, window, plane_bytes):
        """the tile loop of ld_prune's docstring over _variant_rows' generator: yields (buf, table, m) per tile — buf int32
        [3, window + m, sw], the `window` rows before the tile (before the first variant: rows without a bit) and its m rows,
        carried on behind the caller, across plane windows too; table int32 [window + m, window, 8], hhgt_ld_counts over buf,
        reused: the caller's until it asks for the next tile, and one table at the peak if it holds no reference by then."""
        import torch
        ctx = self._context()
        tile = max(self._plane_budget(plane_bytes) // (window * 32) - window, LD_MIN_TILE)
        carry, hold = None, [None]
        for new in rows:
            if carry is None:
                carry = torch.zeros((3, window, new.shape[2]), dtype=torch.int32, device=ctx.device)
            for t0 in range(0, int(new.shape[1]), tile):
                buf = torch.cat([carry, new[:, t0:t0 + tile]], dim=1)
                ctx.ld_counts(buf, window, table=self._zeroed(hold, (buf.shape[1], window, 8)))
                carry = buf[:, -window:].contiguous()
                yield buf, hold[0], int(buf.shape[1]) - window

    def ld_counts(self, group, samples=None, v_lo=0, v_hi=None, variant_mask=None, window=50, slab_bytes=None,
                  plane_bytes=None, max_table_bytes=None):
        """LD counts between nearby variants of a group: an int32 device tensor [n_counted, window, 8], columns LD_N, LD_HM,
        LD_AM, LD_MH, LD_MA, LD_HH, LD_HA, LD_AA (module constants).  The counted variants are those of [v_lo, v_hi) that
        variant_mask marks (a bool tensor or array [v_hi - v_lo]; None: all of them), in order; entry [k, d] belongs to the
        ordered pair (u, v) = (counted variant k, counted variant k + 1 + d) — neighbours are counted variants: a variant
        outside the mask takes no place in a window — and counts, over `samples` (names or indices, each counted once
        however often it is named; None: every sample), the samples at which both calls are complete (both alleles 0 or
        1), u is HET / HOM_ALT and v complete, v is HET / HOM_ALT and u complete, both are HET, one is HET and the other
        HOM_ALT, both are HOM_ALT.  Entries with k + 1 + d >= n_counted are 0.  ld_sums / r2_from_counts / ld_exceeds read
        the table.  Three kernels: hhgt_genotype_planes decodes the selected rows' Blosc blocks into three bits per call
        (chunks handled as in pair_counts: slab_bytes, plane_bytes mean what they mean there), hhgt_variant_planes
        transposes each window of planes, hhgt_ld_counts reduces the counted variants' rows pair by pair; the last `window`
        rows of one plane window are carried into the next, so no pair is lost or counted twice at a seam.  ValueError,
        before the table is allocated, if it (32 bytes per entry) would exceed max_table_bytes (default 2 GiB)."""
        import torch
        window, _, lo, hi, _, n, rows = self._ld_rows("ld_counts", group, window, None, samples, v_lo, v_hi, variant_mask,
                                                      slab_bytes, plane_bytes)
        self._table_budget("ld_counts", f"a table of {n} x {window} pairs ({{}} bytes) exceeds", n * window * 32, max_table_bytes)
        ctx = self._context()
        table = torch.zeros((n, window, 8), dtype=torch.int32, device=ctx.device)
        carry, k0 = None, 0                 # the last rows of the windows so far; the counted index of the next new row
        for new in rows:
            c = 0 if carry is None else int(carry.shape[1])
            buf = new if carry is None else torch.cat([carry, new], dim=1)
            part = table[k0 - c:k0 - c + buf.shape[1]]
            # an entry is one pair: both variants carried (complete since the last window) or the second one new (still 0)
            old = part[:c].clone()
            ctx.ld_counts(buf, window, table=part)
            if c:
                k, d = torch.arange(c, device=ctx.device)[:, None], torch.arange(window, device=ctx.device)[None, :]
                part[:c] = torch.where((k + 1 + d < c)[..., None], old, part[:c])
            carry = buf[:, -window:].contiguous()
            k0 += int(new.shape[1])
        self.stats["ld_pairs"] += self._ld_pairs(n, window)
        return table

    def ld_r2(self, group, samples=None, v_lo=0, v_hi=None, variant_mask=None, window=50, slab_bytes=None,
              plane_bytes=None, max_table_bytes=None):
        """r^2 between nearby variants: r2_from_counts of ld_counts (same arguments) — a float64 device tensor
        [n_counted, window], the squared correlation of the unphased dosages over the jointly complete samples, NaN where
        it is undefined and in the entries past the last variant.  The formula there is the contract; plink2's
        --r2-unphased column is not."""
        return r2_from_counts(self.ld_counts(group, samples, v_lo, v_hi, variant_mask, window, slab_bytes, plane_bytes,
                                             max_table_bytes))

    def ld_prune(self, group, samples=None, v_lo=0, v_hi=None, variant_mask=None, window=50, r2=0.2, slab_bytes=None,
                 plane_bytes=None):
        """greedy LD pruning of the counted variants of a group (group, samples, v_lo / v_hi, variant_mask, window,
        slab_bytes as in ld_counts): a bool device tensor [v_hi - v_lo], False outside variant_mask, that sample_counts,
        pair_counts and kinship take as variant_mask.  Walking the counted variants in order, a variant is kept iff no
        already-kept variant among the `window` counted variants before it has ld_exceeds with it (r^2 > r2, decided from
        the integer counts).  So the first variant is kept, a monomorphic variant is kept, of two duplicates the second
        goes.  This is our rule, simpler than plink2's --indep-pairwise (which slides its window in steps and drops the
        variant with the lower minor allele frequency): the two select different sets.  The work goes tile by tile —
        at least LD_MIN_TILE counted variants, and as many as keep the tile's table within plane_bytes (default 1 GiB) —:
        hhgt_ld_counts over the tile and the `window` rows before it, hhgt_ld_prune over that table with the keep flags of
        those rows carried in.  The whole table never exists, and no genotype, LD count or keep flag goes to the host (with
        a variant_mask, how many variants it marks per plane window does: they size the buffers).  plane_bytes bounds the
        plane window and the tile's table each, not their sum: at its peak a call holds a window's planes, their
        transposed copy, the gathered rows of the counted variants (each up to plane_bytes) and one tile's table (up to
        plane_bytes again): about 4 GiB at the default with every variant counted, less in proportion under a mask."""
        import torch
        window, r2, lo, hi, counted, n, rows = self._ld_rows("ld_prune", group, window, r2, samples, v_lo, v_hi, variant_mask,
                                                             slab_bytes, plane_bytes)
        ctx = self._context()
        carry_keep = torch.zeros(window, dtype=torch.uint8, device=ctx.device)      # before the first variant: flags of 0
        flags = []
        for _, table, m in self._ld_tiles(rows, window, plane_bytes):
            keep = torch.cat([carry_keep, torch.zeros(m, dtype=torch.uint8, device=ctx.device)])
            ctx.ld_prune(table, r2, keep=keep)
            flags.append(keep[window:])
            carry_keep = keep[-window:].contiguous()
            del table                       # (so that a tile of another size replaces it, not stands beside it)
        self.stats["ld_pairs"] += self._ld_pairs(n, window)
        # (without a sample no pair exceeds: every counted variant stays)
        kept = torch.cat(flags).to(torch.bool) if flags else torch.ones(n, dtype=torch.bool, device=ctx.device)
        if counted is None:
            return kept
        out = torch.zeros(hi - lo, dtype=torch.bool, device=ctx.device)
        out[counted] = kept
        return out

    def ld_clump(self, group, p, samples=None, v_lo=0, v_hi=None, variant_mask=None, p1=1e-4, p2=1e-2, r2=0.5, window=1024,
                 kb=250.0, slab_bytes=None, plane_bytes=None):
        """LD clumping of association results over the variants [v_lo, v_hi) of a group (group, samples, v_lo / v_hi,
        variant_mask, slab_bytes, plane_bytes as in ld_prune): p is float64 [v_hi - v_lo], a host array or a device tensor,
        NaN for a variant that takes no part (a finite value outside [0, 1]: ValueError).  -> an int64 device tensor
        [v_hi - v_lo]: per variant the offset into the range of its index variant — its own offset for an index variant —,
        -1 where it has none and outside the counted set.  The counted variants are those variant_mask marks whose p is
        finite and <= p2, in order; neighbours are counted variants.  Two of them are linked iff they are at most `window`
        counted variants apart, ld_exceeds holds between them (r^2 > r2, strictly, from the integer counts) and, unless kb
        is None, their starts are at most int(kb * 1000) bp apart.  Walking the counted variants by ascending p (ties to
        the earlier one), a variant with p <= p1 that is not yet claimed becomes an index variant and claims every linked
        variant that is neither an index nor claimed: store_stats.clump_reference is the contract.  With p1 = p2 = 1, no
        distance limit and p ascending in file order the index variants are the variants ld_prune keeps.  This is our
        rule, not plink's .clumped file column for column: no --clump-replicate, no ranges, no secondary lists, and
        neighbours are counted in variants first, then cut by distance — stats["clump_window_short"] counts the variants
        whose `window`-th follower is still within the distance, where `window`, not kb, ended the search.  The tile loop
        is ld_prune's with hhgt_ld_decisions in place of the walk: each tile's link bits go into one tensor [n_counted,
        ceil(window / 64)] (128 bytes per variant at window 1024), which one hhgt_ld_clump call resolves in parallel
        rounds (stats["clump_rounds"]; at most n_counted).  No genotype, count, bit or owner goes to the host; what does:
        the counted numbers per plane window, the rounds' counters and the window-short count."""
        import torch
        lo, hi, counted, bits, pc = self._clump_links(group, p, samples, v_lo, v_hi, variant_mask, p1, p2, r2, window, kb,
                                                      slab_bytes, plane_bytes)
        out = torch.full((hi - lo,), -1, dtype=torch.int64, device=self._context().device)
        if pc.numel():
            owner, rounds = self._context().ld_clump(bits, int(window), clump_rank(pc).to(torch.int32),
                                                     (pc <= float(p1)).to(torch.uint8))
            self.stats["clump_rounds"] += rounds
            own = owner.to(torch.int64)
            out[counted] = torch.where(own >= 0, counted[own.clamp(min=0)], own)
        return out

    def _clump_links(self, group, p, samples, v_lo, v_hi, variant_mask, p1, p2, r2, window, kb, slab_bytes, plane_bytes):
        """ld_clump up to the link bits: the arguments checked, the counted variants, the tile loop -> (lo, hi, counted — the
        offsets into the range of the counted variants, an int64 device tensor —, bits int64 [n_counted, ceil(window / 64)],
        the counted variants' p float64 [n_counted]); tools/clump_bench.py resolves the same bits on the host"""
        import torch
        window, r2 = self._ld_rows("ld_clump", group, window, r2)
        p1, p2 = float(p1), float(p2)
        if not 0.0 <= p1 <= p2 <= 1.0:
            raise ValueError(f"ld_clump: p1 {p1}, p2 {p2} (0 <= p1 <= p2 <= 1)")
        if kb is not None and not 0.0 <= float(kb) < 1e12:
            raise ValueError(f"ld_clump: kb {kb} (at least 0, or None)")
        max_dist = None if kb is None else int(float(kb) * 1000)
        _, [(group, lo, hi, _, mask)] = self._query("ld_clump", group, samples, v_lo, v_hi, variant_mask, single=True)
        ctx = self._context()
        p = p if torch.is_tensor(p) else torch.from_numpy(np.ascontiguousarray(p, dtype=np.float64))
        if p.dtype != torch.float64 or tuple(p.shape) != (hi - lo,):
            raise ValueError(f"ld_clump: p {list(p.shape)} {p.dtype}, expected float64 [{hi - lo}]")
        p = self._to_device(p)
        finite = torch.isfinite(p)
        if bool((finite & ((p < 0.0) | (p > 1.0))).any()) or bool(torch.isinf(p).any()):
            raise ValueError("ld_clump: a p-value outside [0, 1]")
        take = finite & (p <= p2)
        if mask is not None:
            take &= self._device_bool(mask)
        lo, hi, counted, n, rows = self._variant_rows("ld_clump", group, samples, lo, hi, take, slab_bytes, plane_bytes,
                                                      "ld_plane_blocks")
        self.stats["ld_pairs"] += self._ld_pairs(n, window)
        bits = torch.empty((n, -(-window // 64)), dtype=torch.int64, device=ctx.device)
        pos = None
        if max_dist is not None:        # laid out like a tile's rows: `window` places in front of the first variant
            start = self._to_device(self.variants(group)[0][lo:hi].astype(np.int64))[counted]
            pos = torch.cat([torch.zeros(window, dtype=torch.int64, device=ctx.device), start])
            if n > window:
                self.stats["clump_window_short"] += int((start[window:] - start[:-window] <= max_dist).sum())
        k0 = 0                              # the counted index of the tile's first row
        for _, table, m in self._ld_tiles(rows, window, plane_bytes):
            ctx.ld_decisions(table, r2, None if pos is None else pos[k0:k0 + window + m], max_dist, bits=bits[k0:k0 + m])
            k0 += m
            del table                       # (as in ld_prune)
        bits[k0:].zero_()                   # (without a sample there are no rows, and nothing is linked)
        return lo, hi, counted, bits, p[counted]
