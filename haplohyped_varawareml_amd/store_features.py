"""GenotypeStore's feature matrix: samples x selected variants as a model-ready device tensor."""
import numpy as np

from .store_plan import MAX_FEATURE_BYTES, plan_gather
from .store_stats import call_class_values, cast_class_values


class FeatureQueries:
    """Method of GenotypeStore (no state of its own)."""

    def feature_matrix(self, groups=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, coding="dosage", dtype=None,
                       impute="mean", freq_samples=None, out=None, slab_bytes=None, max_bytes=None):
        """samples x selected variants as a model-ready device tensor -> (X, columns).  X is [len(samples), M] of `dtype`,
        or [len(samples), M, 2] int8 for coding = "haplotypes" (the calls themselves, phase kept); row i is samples[i] in
        the order listed (names or indices; None = every sample in store order; a sample named twice gets its row twice:
        the kernel writes the first occurrence, the others are copied from it).  columns: a list of (group, int64 device
        tensor of the group's variant indices), in column order, the groups concatenated in the order given.  groups, v_lo /
        v_hi, variant_mask and slab_bytes mean what they mean in sample_counts.  coding "dosage" or "standardized" with
        impute "mean" or "missing": call_class_values of allele_counts over freq_samples (default: the listed samples,
        each counted once; give the TRAINING samples to keep held-out ones out of the frequencies) is the value of every
        call class at every variant, cast_class_values to dtype — int8, float16, bfloat16, float32 or float64; default
        float32 for "standardized", int8 otherwise — the table hhgt_gather_calls copies from; "mean" with int8 is a
        ValueError.  The columns are the variants the mask marks and call_class_values uses.  The count pass is skipped
        when the coding needs no frequencies ("haplotypes", "dosage" with "missing").  One hhgt_gather_calls launch per
        slab decodes the selected rows' Blosc blocks and writes the masked variants as dense columns: no [V, 2] range is
        written anywhere.  Chunks are handled as _run_plan says.  out: a tensor of the right dtype and shape with dense rows
        (a row stride of at least M: a slice of a wider batch buffer will do), filled in place and returned.  ValueError
        before X is allocated if it would exceed max_bytes (default MAX_FEATURE_BYTES, 4 GiB)."""
        import torch
        from .device import GATHER_SEL_DTYPE
        raw = coding == "haplotypes"
        if coding not in ("dosage", "standardized", "haplotypes"):
            raise ValueError(f"feature_matrix: coding {coding!r} (\"dosage\", \"standardized\" or \"haplotypes\")")
        if dtype is None:
            dtype = torch.float32 if coding == "standardized" else torch.int8
        if dtype not in ((torch.int8,) if raw else (torch.int8, torch.float16, torch.bfloat16, torch.float32, torch.float64)):
            raise ValueError(f"feature_matrix: dtype {dtype} for coding {coding!r}")
        if not raw:
            call_class_values(np.zeros((0, 4), np.int64), coding, impute, dtype)        # (the argument checks, before any work)
        ctx = self._context()
        sc, vc, bs = self.meta["sc"], self.meta["vc"], self._blocksize()
        vb = bs // 2
        idx, queries = self._query("feature_matrix", groups, samples, v_lo, v_hi, variant_mask)
        need_counts = not raw and not (coding == "dosage" and impute == "missing")
        if need_counts:
            freq = self._freq_samples("feature_matrix", idx, queries[0][0], freq_samples)
        columns, tables, plans, col0 = [], [], [], 0
        for group, lo, hi, n_var, mask in queries:
            keep = None if mask is None else self._device_bool(mask)
            if not raw:
                counts = (self.allele_counts(group, freq, lo, hi, slab_bytes) if need_counts else
                          torch.zeros((hi - lo, 4), dtype=torch.int32, device=ctx.device))
                values, used = call_class_values(counts, coding, impute)
                if need_counts:
                    keep = used if keep is None else used & keep
            counted = (torch.arange(lo, hi, dtype=torch.int64, device=ctx.device) if keep is None else
                       torch.nonzero(keep).reshape(-1) + lo)
            n_blocks = (hi - 1) // vb - lo // vb + 1 if hi > lo else 0
            block_counts = torch.bincount(counted // vb - lo // vb, minlength=n_blocks).cpu().numpy()
            if not raw:
                tables.append(values[:, counted - lo])
            columns.append((group, counted))
            plans.append((group, keep, block_counts, col0))
            col0 += int(counted.numel())
        n, M = len(idx), col0
        nbytes = n * M * (2 if raw else torch.empty(0, dtype=dtype).element_size())
        limit = MAX_FEATURE_BYTES if max_bytes is None else int(max_bytes)
        if nbytes > limit:
            raise ValueError(f"feature_matrix: a matrix of {n} x {M} ({nbytes} bytes) exceeds max_bytes = {limit}")
        shape = (n, M, 2) if raw else (n, M)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=ctx.device)
        elif not torch.is_tensor(out) or out.dtype != dtype or tuple(out.shape) != shape or out.device != torch.device(ctx.device):
            raise ValueError(f"feature_matrix: out must be a {dtype} device tensor {list(shape)}")
        if n == 0 or M == 0:
            return out, columns
        # one row map per call: the entry of a sample is the row of its first occurrence in the list
        first = {}
        for i, s in enumerate(idx.tolist()):
            first.setdefault(s, i)
        row_map = np.zeros(-(-len(self.samples) // sc) * sc, np.uint32)
        row_map[list(first)] = list(first.values())
        d_map = self._to_device(row_map.view(np.int32))
        table = None if raw else cast_class_values(torch.cat(tables, dim=1), dtype).contiguous()
        for (group, lo, hi, n_var, _), (_, keep, block_counts, c0) in zip(queries, plans):
            vmask = self._device_mask(keep, lo, n_var)
            plan = plan_gather(idx, len(self.samples), sc, vc, n_var, lo, hi, block_counts, blocksize=bs, col0=c0)
            self._run_plan(group, plan, slab_bytes, GATHER_SEL_DTYPE, "gather_blocks", lambda dsel: ctx.gather_calls(
                dsel, sc, vc, values=table, out=out, n_cols=M, row_map=d_map, vmask=vmask, typesize=self.meta["typesize"],
                blocksize=bs))
        again = [i for i, s in enumerate(idx.tolist()) if first[s] != i]
        if again:
            out[self._to_device(np.array(again))] = out[self._to_device(np.array([first[int(idx[i])] for i in again]))]
        return out, columns
