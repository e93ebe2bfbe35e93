"""On-disk container for the cohort genotype matrix: a directory of Blosc2-framed chunks + index.

The reference writes one HDF5 file of per-donor compound datasets `donor_{id}/chr_{N}/snp_data` that repeat the variant
columns for every donor; here every chunk is exactly the byte string an HDF5 filter-32001 pipeline would store for a
(64 x 8192 x 2) int8 chunk, so exporting the cohort .h5 (store_h5) copies chunks, and GenotypeStore reads either.

    <store>/meta.json                       samples, donor list, geometry, codec, groups
    <store>/<group>/chunks.bin              framed chunks, vcol-major then scol
    <store>/<group>/offsets.npy             uint64[n_chunks + 1]
    <store>/<group>/start.npy ref.npy alt.npy chrom_runs.json
group = "chr_{N}" (the reference's group naming, vcf_to_h5.py:132).
"""
import json
import os
from collections import OrderedDict

import numpy as np

# (every public name of the split modules stays importable from here; by name: what this module uses itself)
from .h5file import ParallelWrite
from .store_assoc import AssocQueries
from .store_features import FeatureQueries
from .store_h5 import (DONOR_CHUNK_ROWS, CohortWriter, H5CohortWriter, _h5_group_datasets, _h5_strings, export_h5,  # noqa: F401
                       group_record, writer_meta)
from .store_ld import LdQueries
from .store_pairs import PairQueries
from .store_plan import *  # noqa: F401,F403
from .store_plan import (DEFAULT_PLANE_BYTES, MAX_PAIR_TABLE_BYTES, default_blocksize, mask_words_per_block, pack_variant_mask,
                         plan_counts, plan_planes, plan_sample_counts, plan_windows, plane_positions, plane_rows, plane_windows,
                         query_args)
from .store_score import ScoreQueries
from .store_stats import *  # noqa: F401,F403
from .store_stats import AC, AN, standardized_dosages

# the reference's per-donor record (vcf_to_h5.py:119-127): packed, 35 bytes
SNP_DTYPE = np.dtype([("chrom", "S5"), ("start", np.uint32), ("stop", np.uint32), ("ref", "S10"),
                      ("alt", "S10"), ("phase1", np.int8), ("phase2", np.int8)])
assert SNP_DTYPE.itemsize == 35

# default budget of GenotypeStore's device cache of compressed chunks: a 2504-sample cohort's chunk of 64 x 8192 calls
# compresses to ~0.1-0.2 MiB, so this holds about one chr1-sized group of such a cohort (the cache only grows with use)
DEFAULT_CACHE_BYTES = 256 << 20


def chrom_column(runs, n, lo, hi, width):
    """the CHROM column of the variants [lo, hi) of a group of n variants whose CHROM values come in `runs` ((first variant,
    name), in order) -> S{width} [hi - lo], a longer name cut to width"""
    col = np.zeros(hi - lo, dtype=f"S{width}")
    bounds = [r[0] for r in runs] + [n]
    for (a, name), b in zip(runs, bounds[1:]):
        a, b = max(a, lo), min(b, hi)
        if a < b:
            col[a - lo:b - lo] = name.encode()[:width]
    return col


def variant_columns(rec, tables, width, at=None, lo=0, hi=None, pos=False):
    """fills rec's variant columns from a group's variants() `tables`, for its variants [lo, hi) or those at the indices
    `at`: chrom (the CHROM runs, cut to width), start (pos=True: pos = start + 1), stop if rec has one, ref, alt"""
    start, ref, alt, runs = tables
    n, hi = len(start), len(start) if hi is None else hi
    pick = slice(lo, hi) if at is None else at
    rec["chrom"] = chrom_column(runs, n, lo, hi, width) if at is None else chrom_column(runs, n, 0, n, width)[at]
    rec["pos" if pos else "start"] = start[pick] + int(pos)
    if "stop" in rec.dtype.names:
        rec["stop"] = start[pick] + 1
    rec["ref"], rec["alt"] = ref[pick].view("S1"), alt[pick].view("S1")


def _table_budget(who, what, nbytes, max_table_bytes):
    """ValueError if tables of nbytes exceed max_table_bytes (None: MAX_PAIR_TABLE_BYTES); what: the message's middle"""
    limit = MAX_PAIR_TABLE_BYTES if max_table_bytes is None else int(max_table_bytes)
    if nbytes > limit:
        raise ValueError(f"{who}: {what.format(nbytes)} max_table_bytes = {limit}")


class StoreWriter(CohortWriter):
    """CohortWriter into the store directory: a group's chunk bytes go into its chunks.bin as they arrive (add_chunks has
    written them when it returns), its index and tables at end_group, meta.json at close"""

    def __init__(self, path, samples, sc, vc, typesize=2, cohort_name="", donor_ids=None, chunk_format="blosc2"):
        assert chunk_format in ("blosc1", "blosc2")
        super().__init__(samples, sc, vc, typesize, cohort_name, donor_ids, chunk_format)
        self.path = path
        os.makedirs(path, exist_ok=True)
        self._f = None                      # the running group's chunks.bin
        self._par = ParallelWrite()

    def _open_group(self, group):
        self._dir = os.path.join(self.path, group)
        os.makedirs(self._dir, exist_ok=True)
        self._f = open(os.path.join(self._dir, "chunks.bin"), "wb", buffering=0)

    def _put(self, data, at, release):
        self._par.write(self._f.fileno(), data, at)

    def _write_group(self, c, g):
        self._f.close()
        self._f = None
        np.save(os.path.join(self._dir, "offsets.npy"), np.asarray(c.offsets, np.uint64))
        for k, arr in zip(("start", "ref", "alt"), c.columns()):
            np.save(os.path.join(self._dir, k + ".npy"), arr)
        json.dump(c.runs, open(os.path.join(self._dir, "chrom_runs.json"), "w"))

    def _finish(self):
        json.dump(self.meta, open(os.path.join(self.path, "meta.json"), "w"), indent=1)

    def _free(self):
        if self._f is not None:
            self._f.close()
            self._f = None
        self._par.close()


# GenotypeStore.stats: host counters, all from 0
STAT_KEYS = (
    # read_windows: chunks and compressed bytes read from the file, Blosc blocks decoded and their decoded size (the kernel
    # decodes a block whole and writes the selected range of it)
    "chunks_read", "compressed_bytes_read", "blocks_decoded", "bytes_decoded",
    # allele_counts: Blosc blocks it decoded, compressed bytes it read from the file (cache hits not included)
    "count_blocks", "count_compressed_bytes_read",
    "sample_count_blocks",                      # sample_counts (shares count_compressed_bytes_read): Blosc blocks it decoded
    # the plane queries: Blosc blocks their plane stage decoded, and what they reduced
    "pair_plane_blocks", "pair_words",          # pair_counts: plane words per row
    "ld_plane_blocks", "ld_pairs",              # ld_counts / ld_prune / ld_clump: pairs of counted variants
    # ld_clump: rounds that decided a variant; counted variants whose window-th follower is still within the distance limit
    "clump_rounds", "clump_window_short",
    "grm_plane_blocks", "grm_words",            # grm_sums: plane words per row, read by its two reductions
    "assoc_plane_blocks", "assoc_variants",     # assoc_sums: counted variants
    "logistic_variants",                        # assoc_logistic: counted variants (per phenotype)
    "score_plane_blocks", "score_variants",     # score_sums: counted variants whose weights it summed
    "gather_blocks",                            # feature_matrix: Blosc blocks its gather decoded
    # region_sums: pieces its windows gave hhgt_region_sums; counted variants that lie in at least one region
    "region_plane_blocks", "region_pieces", "region_variants",
)


class GenotypeStore(PairQueries, LdQueries, AssocQueries, ScoreQueries, FeatureQueries):
    """Reader.  Opens either the working store directory or the HDF5 file the converter exports
    (`OUT/{cohort}.h5`: read natively through h5file.H5Reader — metadata and raw chunks only).  Decoding runs on the
    GPU (hhgt_decompress_blocks: only the Blosc blocks a read touches); there is no CPU decode path in the product.
    Here: the container, the chunk cache, the walks every query stands on (_run_plan, _plane_walk) and the counts per variant
    and per sample; the other queries are inherited, one module per family (store_pairs, _ld, _assoc, _score, _features)."""

    _table_budget = staticmethod(_table_budget)

    def __init__(self, path, ctx=None, cache_bytes=DEFAULT_CACHE_BYTES):
        """cache_bytes: budget of the device-side cache of compressed chunks (read_windows), least recently used first out"""
        self.path = path
        self._ctx = ctx
        self._h5 = None
        self._files = {}                 # group -> (offsets, memmap of chunks.bin): directory store
        self.cache_bytes = int(cache_bytes)
        self._cache = OrderedDict()      # (group, chunk id) -> device uint8 tensor of the framed chunk
        self._cache_used = 0
        self.stats = dict.fromkeys(STAT_KEYS, 0)
        if os.path.isdir(path):
            self.meta = json.load(open(os.path.join(path, "meta.json")))
        else:
            self._open_h5(path)
        self.samples = self.meta["samples"]
        self._idx = {s: i for i, s in enumerate(self.samples)}

    def _open_h5(self, path):
        from .h5file import FILTER_BLOSC, H5Reader
        r = H5Reader(path)
        root = r.group()
        if "samples" not in root:
            raise ValueError(f"{path}: no /samples dataset — not a cohort file written by vcf_to_h5")
        samples = [x.decode() for x in r.read_array("samples")]
        donors = [x.decode() for x in r.read_array("donor_ids")] if "donor_ids" in root else list(samples)
        meta = dict(format="hhgt-h5", samples=samples, donor_ids=donors, groups={}, chunk_format="blosc1")
        self._h5_info = {}
        for name in sorted(root):
            try:
                members = r.group(root[name])
            except KeyError:
                continue
            if not name.startswith("chr_") or "genotype" not in members:
                continue
            info = r.dataset(f"{name}/genotype")
            if not info["filters"] or info["filters"][0][0] != FILTER_BLOSC:
                raise ValueError(f"{path}:{name}/genotype is not a filter-32001 dataset")
            sc, vc = int(info["chunk_shape"][0]), int(info["chunk_shape"][1])
            # typesize from the filter's client data (h5file.blosc_cd_values); the Blosc block size only exists in the
            # chunk headers, so it comes from the first group that has a chunk (a group without kept SNPs has none)
            meta.update(sc=sc, vc=vc, typesize=int(info["filters"][0][1][2]))
            meta.setdefault("blocksize", default_blocksize(vc))
            if info["chunks"] and "_blocksize_seen" not in meta:
                first = r.read_chunk(info, (0, 0, 0))
                meta.update(blocksize=int(first[8:12].view("<u4")[0]), _blocksize_seen=True)
            meta["groups"][name] = dict(n_variants=int(info["shape"][1]), n_vcol=-(-int(info["shape"][1]) // vc),
                                        n_scol=-(-max(len(samples), 1) // sc), n_chunks=len(info["chunks"]))
            self._h5_info[name] = info
        meta.pop("_blocksize_seen", None)
        self.meta = meta
        self._h5 = r

    def close(self):
        self._cache.clear()
        self._cache_used = 0
        self._files.clear()
        if self._h5 is not None:
            self._h5.close()
            self._h5 = None

    def _context(self):
        if self._ctx is None:
            from .device import Context
            self._ctx = Context(0)
        return self._ctx

    def groups(self):
        return list(self.meta["groups"])

    def variants(self, group):
        if self._h5 is not None:
            r = self._h5
            runs = list(zip((int(x) for x in r.read_array(f"{group}/chrom_run_first")),
                            (x.decode() for x in r.read_array(f"{group}/chrom_run_name"))))
            return (r.read_array(f"{group}/start"), r.read_array(f"{group}/ref").view(np.uint8),
                    r.read_array(f"{group}/alt").view(np.uint8), [list(x) for x in runs])
        d = os.path.join(self.path, group)
        return (np.load(os.path.join(d, "start.npy")), np.load(os.path.join(d, "ref.npy")),
                np.load(os.path.join(d, "alt.npy")), json.load(open(os.path.join(d, "chrom_runs.json"))))

    def _chunk_id(self, group, vcol, scol):
        return vcol * self.meta["groups"][group]["n_scol"] + scol       # vcol-major, then scol (module docstring)

    def _read_chunk(self, group, vcol, scol):
        """framed chunk (vcol, scol) of a group, as host uint8 (the .h5 through H5Reader, the directory store through a
        memmap of chunks.bin and the group's offsets, both opened once per group)"""
        if self._h5 is not None:
            sc, vc = self.meta["sc"], self.meta["vc"]
            return self._h5.read_chunk(self._h5_info[group], (scol * sc, vcol * vc, 0))
        if group not in self._files:
            d = os.path.join(self.path, group)
            self._files[group] = (np.load(os.path.join(d, "offsets.npy")),
                                  np.memmap(os.path.join(d, "chunks.bin"), dtype=np.uint8, mode="r"))
        off, mm = self._files[group]
        i = self._chunk_id(group, vcol, scol)
        return np.asarray(mm[int(off[i]):int(off[i + 1])])

    def _chunk_row(self, group, scol):
        """framed chunks (vcol = 0 .. n_vcol-1) of sample-chunk row `scol`, as a list of uint8 arrays"""
        return [self._read_chunk(group, v, scol) for v in range(self.meta["groups"][group]["n_vcol"])]

    def _sample_index(self, sample):
        s = self._idx[sample] if isinstance(sample, str) else int(sample)
        if not 0 <= s < len(self.samples):
            raise IndexError(f"sample {sample} out of range (0..{len(self.samples) - 1})")
        return s

    def _blocksize(self):
        """the Blosc block size the chunks were written with, clamped to the chunk as c-blosc (and the decoder) clamp it"""
        ts, nbytes = self.meta["typesize"], self.meta["sc"] * self.meta["vc"] * 2
        bs = int(self.meta["blocksize"])
        if bs > nbytes:
            bs = nbytes - (nbytes % ts if ts > 1 and nbytes >= ts else 0)
        return max(bs, 1)

    def _query(self, who, groups, samples=None, v_lo=0, v_hi=None, variant_mask=None, single=False):
        """query_args over this store: -> (sample indices, [(group, lo, hi, n_var, mask)])"""
        return query_args(self.meta, self._idx, who, groups, samples, v_lo, v_hi, variant_mask, single)

    def _upload(self, host):
        """host: key -> the framed chunk as read from the file (uint8 array), any number but none -> (key -> device uint8
        tensor, the bytes copied): the chunks concatenated, sent up in one copy, and each a view into that buffer"""
        cat = np.concatenate(list(host.values()))
        dev = self._to_device(cat)
        ends = np.cumsum([a.size for a in host.values()]).tolist()
        return {k: dev[e - a.size:e] for (k, a), e in zip(host.items(), ends)}, int(cat.size)

    def read_windows(self, requests):
        """genotypes of (group, sample, v_lo, v_hi) requests: -> one int8 device tensor [v_hi - v_lo, 2] per request (views
        into one buffer, the requests' rows end to end).  Only the Blosc blocks the ranges touch are decoded, in one
        hhgt_decompress_blocks launch; only the chunks they lie in are read, the missing ones uploaded in one copy and
        kept in the device-side chunk cache.  Nothing is copied back to the host."""
        import torch
        from .device import SEL_DTYPE
        ctx = self._context()
        sc, vc = self.meta["sc"], self.meta["vc"]
        norm = []
        for group, sample, v_lo, v_hi in requests:
            idx, [(group, lo, hi, _, _)] = self._query("read_windows", group, [sample], v_lo, v_hi, single=True)
            norm.append((group, int(idx[0]), lo, hi))
        sel, out_off = plan_windows([r[1:] for r in norm], sc, vc, self._blocksize())
        keys = [(norm[q][0], self._chunk_id(norm[q][0], int(vcol), int(scol)))
                for q, vcol, scol in zip(sel["req"], sel["vcol"], sel["scol"])]
        # chunks: cache hits, then the misses read on the host and uploaded in one copy
        chunks, missing = {}, {}
        for k, vcol, scol in zip(keys, sel["vcol"], sel["scol"]):
            if k in chunks or k in missing:
                continue
            if k in self._cache:
                self._cache.move_to_end(k)
                chunks[k] = self._cache[k]
            else:
                missing[k] = self._read_chunk(k[0], int(vcol), int(scol))
        if missing:
            # every cached chunk gets its own allocation (a device copy of its part of the upload), so evicting a chunk
            # frees its bytes and the cache holds no more than its budget
            up, n_bytes = self._upload(missing)
            fresh = {k: t if len(up) == 1 else t.clone() for k, t in up.items()}
            del up
            chunks.update(fresh)
            self._cache.update(fresh)
            self._cache_used += n_bytes
            self.stats["chunks_read"] += len(missing)
            self.stats["compressed_bytes_read"] += n_bytes
        # (an evicted chunk of this call stays alive in `chunks` until the launch is done: decompress_blocks syncs)
        while self._cache_used > self.cache_bytes and self._cache:
            _, t = self._cache.popitem(last=False)
            self._cache_used -= t.numel()
        dsel = np.zeros(len(sel), dtype=SEL_DTYPE)
        dsel["src_ptr"] = [chunks[k].data_ptr() for k in keys]
        dsel["src_bytes"] = [chunks[k].numel() for k in keys]
        for f in ("dst_off", "block", "lo", "hi"):
            dsel[f] = sel[f]
        total = int(out_off[-1])
        out = torch.empty(max(total, 16), dtype=torch.uint8, device=ctx.device)
        if len(sel):
            chunk_nbytes, bs = sc * vc * 2, self._blocksize()
            _, bad = ctx.decompress_blocks(dsel, chunk_nbytes, typesize=self.meta["typesize"], blocksize=bs, dst=out)
            if bad:
                raise RuntimeError(f"{bad} corrupt chunk(s) in {', '.join(sorted({r[0] for r in norm}))}")
            self.stats["blocks_decoded"] += len(sel)
            self.stats["bytes_decoded"] += int(np.minimum(bs, chunk_nbytes - sel["block"].astype(np.int64) * bs).sum())
        g8 = out.view(torch.int8)
        return [g8[int(out_off[q]):int(out_off[q + 1])].view(-1, 2) for q in range(len(norm))]

    def _run_plan(self, group, plan, slab_bytes, sel_dtype, stat_key, call):
        """runs the selections `plan` of a group (vcol / scol per selection, plan order: chunk columns in order) through a
        row kernel, slab by slab: chunks in the read cache are used as they are, the rest read from the file and uploaded
        in slabs of at most slab_bytes (default: the cache budget; a larger chunk goes alone), one copy per slab (_upload).
        A slab's selections become sel_dtype records — the chunk's address and size from the slab, every other field the
        plan has from the plan —, call(records) -> (_, n_bad) launches them and must synchronise, for the slab is freed
        behind it; RuntimeError if a selection was bad.  stats[stat_key] counts the blocks decoded (one per selected row
        and selection).  So for every query but read_windows: cached chunks used, the read cache neither filled nor evicted."""
        budget = self.cache_bytes if slab_bytes is None else int(slab_bytes)
        keys = [(group, self._chunk_id(group, int(v), int(c))) for v, c in zip(plan["vcol"], plan["scol"])]
        fields = [f for f in sel_dtype.names if f in plan.dtype.names]
        blocks = np.array([bin(int(m)).count("1") for m in plan["row_mask"]], np.int64)

        def launch(slab, host, rows):
            if host:
                up, n_bytes = self._upload(host)
                slab.update(up)
                self.stats["count_compressed_bytes_read"] += n_bytes
            if rows:
                dsel = np.zeros(len(rows), sel_dtype)
                dsel["src_ptr"] = [slab[keys[i]].data_ptr() for i in rows]
                dsel["src_bytes"] = [slab[keys[i]].numel() for i in rows]
                for f in fields:
                    dsel[f] = plan[f][rows]
                _, bad = call(dsel)         # (synchronises: the slab's memory is free to go when this returns)
                if bad:
                    raise RuntimeError(f"{bad} corrupt chunk(s) in {group}")
                self.stats[stat_key] += int(blocks[rows].sum())

        slab, host, rows, size = {}, {}, [], 0      # cached chunks; chunks read, to upload; selections; bytes of `host`
        for i, k in enumerate(keys):
            if k not in slab and k not in host:
                if k in self._cache:
                    slab[k] = self._cache[k]
                else:
                    a = self._read_chunk(group, int(plan["vcol"][i]), int(plan["scol"][i]))
                    if host and size + a.size > budget:
                        launch(slab, host, rows)
                        slab, host, rows, size = {}, {}, [], 0
                    host[k] = a
                    size += a.size
            rows.append(i)
        launch(slab, host, rows)

    def _device_mask(self, mask, lo, n_var):
        """a group's variant mask over [lo, lo + len(mask)) as the row kernels read it: packed (pack_variant_mask) and on
        the device — a host mask goes up once, not with every slab; None stays None"""
        import torch
        if mask is None:
            return None
        vmask = pack_variant_mask(mask, lo, n_var, self.meta["vc"], self._blocksize())
        return vmask if torch.is_tensor(vmask) else self._to_device(vmask.view(np.int32))

    def _device_bool(self, mask):
        """a variant mask, host array or tensor -> a bool tensor on the device"""
        import torch
        return self._to_device(mask if torch.is_tensor(mask) else np.asarray(mask, dtype=bool)).to(torch.bool)

    def _to_device(self, x):
        """host array or tensor -> a contiguous tensor on the device"""
        import torch
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        return x.to(self._context().device).contiguous()

    def _masked(self, w, mask, lo=None, n_var=None):
        """device values w [..., n, K] under a variant mask [n], host or device, or None -> (w with zeros at the variants the
        mask leaves out, the mask as a bool device tensor or None, _device_mask(mask, lo, n_var) or None: also without lo)"""
        import torch
        if mask is None:
            return w, None, None
        mask = self._device_bool(mask)
        return (torch.where(mask[:, None], w, torch.zeros_like(w)), mask,
                None if lo is None else self._device_mask(mask, lo, n_var))

    def _freq_samples(self, who, idx, group, freq_samples):
        """the samples whose allele counts give `who` its frequencies: freq_samples, by default those of idx, each once"""
        return np.unique(idx) if freq_samples is None else self._query(who, group, freq_samples, single=True)[0]

    def _zeroed(self, hold, shape):
        """hold: a list of one int32 device tensor, the buffer of the call before, or None -> hold[0]: zeros of `shape`, the
        same buffer if it has that shape (callers reach it through hold[0] and bind no name of their own)"""
        import torch
        if hold[0] is not None and tuple(hold[0].shape) == tuple(shape):
            return hold[0].zero_()
        hold[0] = None                      # dropped before the new one is allocated: the peak is one buffer, not two
        hold[0] = torch.zeros(tuple(shape), dtype=torch.int32, device=self._context().device)
        return hold[0]

    def allele_counts(self, group, samples=None, v_lo=0, v_hi=None, slab_bytes=None):
        """per-variant allele counts of the variants [v_lo, v_hi) of a group over `samples` (names or indices, each counted
        once; None = every sample): an int32 device tensor [v_hi - v_lo, 4], columns AN, AC, HET, HOM_ALT (module
        constants) — called alleles, alleles equal to 1, heterozygous calls (two called, different alleles), calls 1/1.
        Missing alleles are 2 * n_samples - AN.  hhgt_count_alleles decodes the selected rows' Blosc blocks and counts in
        LDS; no genotype is written anywhere.  The chunks are handled as _run_plan says (slab_bytes: its slabs)."""
        import torch
        from .device import COUNT_SEL_DTYPE
        ctx = self._context()
        sc, vc, bs = self.meta["sc"], self.meta["vc"], self._blocksize()
        idx, [(group, lo, hi, n_var, _)] = self._query("allele_counts", group, samples, v_lo, v_hi, single=True)
        plan = plan_counts(idx, len(self.samples), sc, vc, n_var, lo, hi, blocksize=bs)
        counts = torch.zeros((hi - lo, 4), dtype=torch.int32, device=ctx.device)
        self._run_plan(group, plan, slab_bytes, COUNT_SEL_DTYPE, "count_blocks", lambda dsel: ctx.count_alleles(
            dsel, sc, vc, typesize=self.meta["typesize"], blocksize=bs, counts=counts))
        return counts

    def sample_counts(self, groups=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None):
        """per-sample counts over the variants of `groups` (one name, a list, None = every group): an int32 device tensor
        [len(samples), 4], columns AN, AC, HET, HOM_ALT as in allele_counts, row i for samples[i] (names or indices; None
        = every sample in store order; a sample named twice gets the same row twice).  v_lo / v_hi: the variants
        [v_lo, v_hi) only — with a single group.  variant_mask: count only the variants it marks: a bool tensor or array
        [v_hi - v_lo] (single group), or a dict group -> mask over the whole group (a group it does not name is counted
        whole); a device tensor (variant_mask()) never leaves the device.  Missing alleles of a sample are 2 * (variants
        counted) - AN.  hhgt_count_samples decodes the selected rows' Blosc blocks and reduces each in LDS; no genotype is
        written anywhere, the groups accumulate into one counter table.  The chunks are handled as _run_plan says."""
        import torch
        from .device import SAMPLE_SEL_DTYPE
        ctx = self._context()
        sc, vc, bs = self.meta["sc"], self.meta["vc"], self._blocksize()
        idx, queries = self._query("sample_counts", groups, samples, v_lo, v_hi, variant_mask)
        table = torch.zeros((-(-max(len(self.samples), 1) // sc) * sc, 4), dtype=torch.int32, device=ctx.device)
        for group, lo, hi, n_var, mask in queries:
            vmask = self._device_mask(mask, lo, n_var)
            plan = plan_sample_counts(idx, len(self.samples), sc, vc, n_var, lo, hi, blocksize=bs)
            self._run_plan(group, plan, slab_bytes, SAMPLE_SEL_DTYPE, "sample_count_blocks",
                           lambda dsel: ctx.count_samples(dsel, sc, vc, typesize=self.meta["typesize"], blocksize=bs,
                                                          vmask=vmask, counts=table))
        return table[self._to_device(idx)]

    def _plane_rows(self, idx):
        """the plane rows of the samples idx (store_plan.plane_rows) -> (their number, the plane row of each of idx, on the host)"""
        scols, rows = plane_rows(idx, self.meta["sc"])
        return len(scols) * self.meta["sc"], rows

    @staticmethod
    def _plane_budget(plane_bytes):
        """the bound of a plane window's buffer (and of ld_prune's table), default 1 GiB"""
        return DEFAULT_PLANE_BYTES if plane_bytes is None else int(plane_bytes)

    def _window_values(self, x, lo, a, b, words):
        """x [k, n, ...]: a value per variant of a range that begins at variant lo -> zeros [k, 32 * words, ...] of x's dtype
        with those of the variants [a, b), a plane window of `words` words, at their bit positions (plane_positions)"""
        import torch
        out = torch.zeros((x.shape[0], 32 * words) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
        out[:, self._to_device(plane_positions(a, b, self._blocksize()))] = x[:, a - lo:b - lo]
        return out

    def _dosages(self, group, idx, lo, hi, mask, slab_bytes):
        """standardized_dosages of allele_counts over the samples idx -> (z, used), used ANDed with the variant mask"""
        z, used = standardized_dosages(self.allele_counts(group, idx, lo, hi, slab_bytes))
        return z, used if mask is None else used & self._device_bool(mask)

    def _plane_walk(self, group, idx, lo, hi, n_var, stat_key, slab_bytes, plane_bytes, vmask=None):
        """the genotype planes of the samples idx over the variants [lo, hi) of a group, window by window: yields (a, b,
        words, planes) per window [a, b) of plane_windows (whole Blosc blocks whose plane buffer is at most plane_bytes,
        default 1 GiB) — planes: an int32 device tensor [3, plane rows of idx, words], zeroed and then filled by
        hhgt_genotype_planes over the window's selections (plan_planes; _run_plan with slab_bytes, its blocks counted in
        stats[stat_key]; vmask: the group's packed variant mask on the device, or None).  The buffer is reused from one
        window to the next and so belongs to the caller only until it asks for the next.  Nothing for no sample."""
        from .device import PLANE_SEL_DTYPE
        ctx = self._context()
        sc, vc, bs = self.meta["sc"], self.meta["vc"], self._blocksize()
        n_rows = self._plane_rows(idx)[0]
        if n_rows == 0:
            return
        vb, wpb = bs // 2, mask_words_per_block(bs)
        hold = [None]
        for a, b in plane_windows(lo, hi, bs, n_rows, self._plane_budget(plane_bytes)):
            words = ((b - 1) // vb - a // vb + 1) * wpb
            self._zeroed(hold, (3, n_rows, words))          # (the last window of a range may be shorter)
            plan = plan_planes(idx, len(self.samples), sc, vc, n_var, a, b, blocksize=bs)
            self._run_plan(group, plan, slab_bytes, PLANE_SEL_DTYPE, stat_key, lambda dsel: ctx.genotype_planes(
                dsel, sc, vc, typesize=self.meta["typesize"], blocksize=bs, vmask=vmask, planes=hold[0]))
            yield a, b, words, hold[0]

    def _variant_rows(self, who, group, samples, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes, stat_key):
        """the counted variants of a group as rows of bits, for `who` (in the messages), the plane stage's blocks counted in
        stats[stat_key] -> (lo, hi, counted, n_counted, rows): the range, checked; the offsets into it of the variants the
        mask marks, an int64 device tensor, or None; the number of counted variants (with a mask it comes from the device,
        together with the number of counted variants per plane window: one small copy per call, whatever the number of
        windows); and a generator of int32 device tensors [3, m, sw], the variant-major planes (HET, COMPLETE, HOM_ALT over
        the plane rows of `samples`) of the counted variants, in order, plane window by plane window: the planes come from
        _plane_walk (no variant mask there), each window is transposed (hhgt_variant_planes) and the rows at
        plane_positions of the counted variants gathered, which leaves out block padding and masked variants in one step."""
        import torch
        ctx, bs = self._context(), self._blocksize()
        idx, [(group, lo, hi, n_var, variant_mask)] = self._query(who, group, samples, v_lo, v_hi, variant_mask, single=True)
        if variant_mask is None:
            n_counted, counted, cuts = hi - lo, None, None
        else:
            # the counted variants (offsets into the range) stay on the device; what comes back, in one copy for the whole
            # call, is how many of them lie before each plane window's end
            counted = torch.nonzero(self._device_bool(variant_mask)).reshape(-1)
            n_rows = self._plane_rows(idx)[0]
            windows = plane_windows(lo, hi, bs, n_rows, self._plane_budget(plane_bytes)) if n_rows else []
            ends = torch.tensor([0] + [b - lo for _, b in windows] + [hi - lo], dtype=torch.int64, device=ctx.device)
            cuts = torch.searchsorted(counted, ends).cpu().tolist()
            n_counted = cuts[-1]

        def rows():
            walk = self._plane_walk(group, idx, lo, hi, n_var, stat_key, slab_bytes, plane_bytes)
            for w, (a, b, words, planes) in enumerate(walk):
                pos = self._to_device(plane_positions(a, b, bs))
                if counted is not None:
                    pos = pos.index_select(0, counted[cuts[w]:cuts[w + 1]] - (a - lo))
                if pos.numel():
                    yield ctx.variant_planes(planes, 0, words).index_select(1, pos)

        return lo, hi, counted, n_counted, rows()

    def variant_mask(self, group, samples=None, v_lo=0, v_hi=None, min_maf=None, max_ac=None, min_ac=None, max_maf=None):
        """a class of the variants [v_lo, v_hi) of a group, from allele_counts over `samples` (same arguments), as a bool
        device tensor [v_hi - v_lo] that sample_counts takes as variant_mask; nothing is copied to the host.  A variant
        is kept iff it passes every bound given: min_maf — AN > 0 and min(AC, AN - AC) >= min_maf * AN, compared as
        float64 —; max_maf — AN > 0 and min(AC, AN - AC) <= max_maf * AN, likewise (the rare variants of a burden score) —;
        min_ac <= AC; AC <= max_ac (integers; singletons: min_ac = max_ac = 1).  No bound: every variant."""
        import torch
        c = self.allele_counts(group, samples, v_lo, v_hi)
        an, ac = c[:, AN].to(torch.int64), c[:, AC].to(torch.int64)
        keep = torch.ones(c.shape[0], dtype=torch.bool, device=c.device)
        if min_maf is not None:
            keep &= (an > 0) & (torch.minimum(ac, an - ac).double() >= float(min_maf) * an.double())
        if max_maf is not None:
            keep &= (an > 0) & (torch.minimum(ac, an - ac).double() <= float(max_maf) * an.double())
        if min_ac is not None:
            keep &= ac >= int(min_ac)
        if max_ac is not None:
            keep &= ac <= int(max_ac)
        return keep

    def allele_frequencies(self, group, samples=None, v_lo=0, v_hi=None, slab_bytes=None):
        """AC / AN of allele_counts (same arguments): a float32 device tensor [v_hi - v_lo], NaN where AN == 0"""
        import torch
        c = self.allele_counts(group, samples, v_lo, v_hi, slab_bytes)
        an = c[:, AN].to(torch.float32)
        return torch.where(an > 0, c[:, AC].to(torch.float32) / an, torch.full_like(an, float("nan")))

    def sample_row(self, group, sample):
        """int8 [n_variants, 2] for one sample: decodes the sample's blocks on the GPU (read_windows)."""
        g = self.meta["groups"][group]
        if g["n_vcol"] == 0:
            return np.zeros((0, 2), np.int8)
        return self.read_windows([(group, sample, 0, g["n_variants"])])[0].cpu().numpy()

    def snp_records(self, group, sample, v_lo=0, v_hi=None, tables=None):
        """the reference's per-donor compound records (vcf_to_h5.py:119-129), synthesised on demand; v_lo / v_hi: those
        of the group's variants [v_lo, v_hi) only (a windowed read); tables: variants(group), when the caller has it"""
        tables = tables if tables is not None else self.variants(group)
        v_hi = len(tables[0]) if v_hi is None else v_hi
        if v_lo == 0 and v_hi == len(tables[0]):
            ph = self.sample_row(group, sample)
        else:
            ph = self.read_windows([(group, sample, v_lo, v_hi)])[0].cpu().numpy()
        rec = np.zeros(v_hi - v_lo, dtype=SNP_DTYPE)
        variant_columns(rec, tables, 5, lo=v_lo, hi=v_hi)
        rec["phase1"], rec["phase2"] = ph[:, 0], ph[:, 1]
        return rec
