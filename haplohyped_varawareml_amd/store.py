"""On-disk container for the cohort genotype matrix: a directory of Blosc2-framed chunks + index.

The reference writes one HDF5 file with S x 22 compound datasets `donor_{id}/chr_{N}/snp_data`
(/root/reference/src/haplohyped/vcf_to_h5.py:131-135,154-180), each repeating chrom/start/stop/ref/alt
for every donor.  h5py/hdf5plugin are not available in this image (SURVEY.md §7 hard part 6), so the
primary artefact is this directory; every chunk in it is exactly the byte string an HDF5 filter-32001
pipeline would store for a (64 x 8192 x 2) int8 chunk, so `write_direct_chunk` assembly is a copy.

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

# (every public name of the split modules stays importable from here)
from .h5file import ParallelWrite
from .store_h5 import (DONOR_CHUNK_ROWS, CohortWriter, H5CohortWriter, _h5_group_datasets, _h5_strings, export_h5,  # noqa: F401
                       group_record, writer_meta)
from .store_plan import (COUNT_PLAN_DTYPE, DEFAULT_PLANE_BYTES, GATHER_PLAN_DTYPE, LD_MIN_TILE, MAX_FEATURE_BYTES,  # noqa: F401
                         MAX_PAIR_TABLE_BYTES, PLAN_DTYPE, PLANE_PLAN_DTYPE, ROW_PLAN_DTYPE, SAMPLE_PLAN_DTYPE,
                         default_blocksize, mask_words_per_block, pack_variant_mask, plan_counts, plan_gather, plan_planes,
                         plan_rows, plan_sample_counts, plan_windows, plane_positions, plane_rows, plane_windows, query_args,
                         sample_index)
from .store_plan import REGION_MAX_COLS, REGION_SPAN, plan_regions  # noqa: F401
from .store_stats import (AC, AN, ASSOC_ALT, ASSOC_BETA, ASSOC_COMPLETE, ASSOC_HET, ASSOC_MAX_COLS, ASSOC_P,  # noqa: F401
                          ASSOC_SE, ASSOC_T, GRM_SPAN, HET, HET1, HETHET, HOM_ALT, IBS0, LD_AA, LD_AM, LD_HA, LD_HH,
                          LD_HM, LD_MA, LD_MH, LD_N, LOGIT_BETA, LOGIT_COLLINEAR, LOGIT_MAX_COLS, LOGIT_NO_CALL, LOGIT_NOT_CONVERGED,
                          LOGIT_ONE_CLASS, LOGIT_P, LOGIT_REC, LOGIT_SCORE_CHI2, LOGIT_SCORE_P, LOGIT_SE, LOGIT_STATUS_NAMES,
                          LOGIT_TESTED, LOGIT_Z, NSNP, REC_ALT, REC_COMPLETE, REC_GAMMA, REC_HET, REC_HINV, REC_HINV0, REC_STATUS,
                          REC_STEPS, REC_U0, assoc_design, assoc_from_sums, grm_from_sums, ibs_counts, logistic_design,
                          logistic_fit_reference, logistic_from_fit, logistic_score_design, logistic_score_from_sums,
                          normal_two_sided,
                          check_components, clump_rank, clump_reference, clump_summary, kinship_from_counts, ld_exceeds, ld_sums, r2_from_counts,
                          standardized_dosages, student_t_two_sided, top_eigenpairs)
from .store_stats import (SCORE_MAX_COLS, SCORE_SLICE, SCORE_SPAN, call_class_values, cast_class_values,  # noqa: F401
                          loadings_from_sums, projection_class_weights, score_class_weights)
from .store_stats import (beta_density_weights, burden_class_weights, dense_assoc, dense_logistic_score,  # noqa: F401
                          region_totals)

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


class GenotypeStore:
    """Reader.  Opens either the working store directory or the HDF5 file the converter exports
    (`OUT/{cohort}.h5`: read natively through h5file.H5Reader — metadata and raw chunks only).  Decoding runs on the
    GPU (hhgt_decompress_blocks: only the Blosc blocks a read touches); there is no CPU decode path in the product."""

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
        import torch
        cat = np.concatenate(list(host.values()))
        dev = torch.from_numpy(cat).to(self._context().device)
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
        and selection).  The cache is neither filled nor evicted."""
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
        return vmask if torch.is_tensor(vmask) else torch.from_numpy(vmask.view(np.int32)).to(self._context().device)

    def _device_bool(self, mask):
        """a variant mask, host array or tensor -> a bool tensor on the device"""
        import torch
        mask = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(mask, dtype=bool))
        return mask.to(self._context().device).to(torch.bool)

    def allele_counts(self, group, samples=None, v_lo=0, v_hi=None, slab_bytes=None):
        """per-variant allele counts of the variants [v_lo, v_hi) of a group over `samples` (names or indices, each counted
        once; None = every sample): an int32 device tensor [v_hi - v_lo, 4], columns AN, AC, HET, HOM_ALT (module
        constants) — called alleles, alleles equal to 1, heterozygous calls (two called, different alleles), calls 1/1.
        Missing alleles are 2 * n_samples - AN.  hhgt_count_alleles decodes the selected rows' Blosc blocks and counts in
        LDS; no genotype is written anywhere.  Chunks already in the read cache are used as they are, the rest read from the
        file and uploaded in slabs of at most slab_bytes (default: the cache budget; a chunk larger than that goes alone),
        each freed after its launch: the scan neither adds chunks to the cache nor evicts any."""
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
        written anywhere, the groups accumulate into one counter table.  Chunks are handled as in allele_counts: cached
        ones used, the rest uploaded in slabs of at most slab_bytes, the read cache neither filled nor evicted."""
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
        return table[torch.from_numpy(idx).to(ctx.device)]

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
        out[:, torch.from_numpy(plane_positions(a, b, self._blocksize())).to(x.device)] = x[:, a - lo:b - lo]
        return out

    def _dosages(self, group, idx, lo, hi, mask, slab_bytes):
        """standardized_dosages of allele_counts over the samples idx -> (z, used), used ANDed with the variant mask"""
        z, used = standardized_dosages(self.allele_counts(group, idx, lo, hi, slab_bytes))
        return z, used if mask is None else used & self._device_bool(mask)

    @staticmethod
    def _zero_outside(w, mask):
        """w [..., n, K] with zeros at the variants a bool device tensor [n] leaves out"""
        import torch
        return torch.where(mask[:, None], w, torch.zeros_like(w))

    def _plane_walk(self, group, idx, lo, hi, n_var, stat_key, slab_bytes, plane_bytes, vmask=None):
        """the genotype planes of the samples idx over the variants [lo, hi) of a group, window by window: yields (a, b,
        words, planes) per window [a, b) of plane_windows (whole Blosc blocks whose plane buffer is at most plane_bytes,
        default 1 GiB) — planes: an int32 device tensor [3, plane rows of idx, words], zeroed and then filled by
        hhgt_genotype_planes over the window's selections (plan_planes; _run_plan with slab_bytes, its blocks counted in
        stats[stat_key]; vmask: the group's packed variant mask on the device, or None).  The buffer is reused from one
        window to the next and so belongs to the caller only until it asks for the next.  Nothing for no sample."""
        import torch
        from .device import PLANE_SEL_DTYPE
        ctx = self._context()
        sc, vc, bs = self.meta["sc"], self.meta["vc"], self._blocksize()
        n_rows = self._plane_rows(idx)[0]
        if n_rows == 0:
            return
        vb, wpb = bs // 2, mask_words_per_block(bs)
        planes = None
        for a, b in plane_windows(lo, hi, bs, n_rows, self._plane_budget(plane_bytes)):
            words = ((b - 1) // vb - a // vb + 1) * wpb
            if planes is None or planes.shape[2] != words:
                planes = None                       # (the last window of a range may be shorter)
                planes = torch.zeros((3, n_rows, words), dtype=torch.int32, device=ctx.device)
            else:
                planes.zero_()
            plan = plan_planes(idx, len(self.samples), sc, vc, n_var, a, b, blocksize=bs)
            self._run_plan(group, plan, slab_bytes, PLANE_SEL_DTYPE, stat_key, lambda dsel: ctx.genotype_planes(
                dsel, sc, vc, typesize=self.meta["typesize"], blocksize=bs, vmask=vmask, planes=planes))
            yield a, b, words, planes

    def _pair_query(self, who, groups, samples, v_lo, v_hi, variant_mask, bytes_per_pair, max_table_bytes):
        """pair_counts' and grm_sums' (`who`) start: _query, the plane rows, the budget of their tables of bytes_per_pair
        per pair of plane rows -> (idx, queries, n_rows, pick: a table [n_rows, n_rows, ...] -> the samples' part of it)"""
        idx, queries = self._query(who, groups, samples, v_lo, v_hi, variant_mask)
        n_rows, rows = self._plane_rows(idx)
        what = ("a table of {0} x {0} pairs ({{}} bytes) exceeds" if bytes_per_pair == 16 else
                "tables of {0} x {0} pairs ({{}} bytes) exceed").format(n_rows)
        _table_budget(who, what, n_rows * n_rows * bytes_per_pair, max_table_bytes)
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

    def _ld_rows(self, who, group, samples, v_lo, v_hi, variant_mask, window, slab_bytes, plane_bytes):
        """what ld_counts and ld_prune (`who`, for the messages) do alike: the group and the window, checked, then
        _variant_rows"""
        if not isinstance(group, str) or group not in self.meta["groups"]:
            raise KeyError(group)
        if not 1 <= int(window) <= 1024:
            raise ValueError(f"{who}: window {int(window)} (1 to 1024)")
        return self._variant_rows(who, group, samples, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes, "ld_plane_blocks")

    def _variant_rows(self, who, group, samples, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes, stat_key):
        """the counted variants of a group as rows of bits, for `who` (in the messages), the plane stage's blocks counted in
        stats[stat_key] -> (lo, hi, counted, n_counted, rows): the range, checked; the offsets into it of the variants the
        mask marks, an int64 device tensor, or None; the number of counted
        variants (with a mask it comes from the device, together with the number of counted variants per plane window: one
        small copy per call, whatever the number of windows); and a generator of int32 device tensors [3, m, sw], the
        variant-major planes (HET, COMPLETE, HOM_ALT over the plane rows of `samples`) of the counted variants, in order,
        plane window by plane window: the planes come as in pair_counts (_plane_walk: cached chunks used, the read cache
        neither filled nor evicted; no variant mask there), each window is transposed (hhgt_variant_planes) and the rows at
        plane_positions of the counted variants gathered, which leaves out block padding and masked variants in one step."""
        import torch
        ctx = self._context()
        bs = self._blocksize()
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
                pos = torch.from_numpy(plane_positions(a, b, bs)).to(ctx.device)
                if counted is not None:
                    pos = pos.index_select(0, counted[cuts[w]:cuts[w + 1]] - (a - lo))
                if pos.numel():
                    yield ctx.variant_planes(planes, 0, words).index_select(1, pos)

        return lo, hi, counted, n_counted, rows()

    @staticmethod
    def _ld_pairs(n, window):
        """pairs (k, k + 1 + d), d < window, among n variants"""
        return n * (n - 1) // 2 if n <= window else n * window - window * (window + 1) // 2

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
        window = int(window)
        lo, hi, _, n, rows = self._ld_rows("ld_counts", group, samples, v_lo, v_hi, variant_mask, window, slab_bytes,
                                              plane_bytes)
        _table_budget("ld_counts", f"a table of {n} x {window} pairs ({{}} bytes) exceeds", n * window * 32, max_table_bytes)
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
        window, r2 = int(window), float(r2)
        if not 0.0 <= r2 <= 1.0:
            raise ValueError(f"ld_prune: r2 {r2} (0 to 1)")
        lo, hi, counted, n, rows = self._ld_rows("ld_prune", group, samples, v_lo, v_hi, variant_mask, window, slab_bytes,
                                              plane_bytes)
        ctx = self._context()
        tile = max(self._plane_budget(plane_bytes) // (window * 32) - window, LD_MIN_TILE)
        carry = carry_keep = table = None
        flags = []
        for new in rows:
            if carry is None:               # before the first variant: rows without a bit, flags of 0
                carry = torch.zeros((3, window, new.shape[2]), dtype=torch.int32, device=ctx.device)
                carry_keep = torch.zeros(window, dtype=torch.uint8, device=ctx.device)
            for t0 in range(0, int(new.shape[1]), tile):
                buf = torch.cat([carry, new[:, t0:t0 + tile]], dim=1)
                if table is None or table.shape[0] != buf.shape[1]:
                    table = None
                    table = torch.zeros((buf.shape[1], window, 8), dtype=torch.int32, device=ctx.device)
                else:
                    table.zero_()
                ctx.ld_counts(buf, window, table=table)
                keep = torch.cat([carry_keep, torch.zeros(buf.shape[1] - window, dtype=torch.uint8, device=ctx.device)])
                ctx.ld_prune(table, r2, keep=keep)
                flags.append(keep[window:])
                carry, carry_keep = buf[:, -window:].contiguous(), keep[-window:].contiguous()
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
        window, r2, p1, p2 = int(window), float(r2), float(p1), float(p2)
        if not 0.0 <= r2 <= 1.0:
            raise ValueError(f"ld_clump: r2 {r2} (0 to 1)")
        if not 0.0 <= p1 <= p2 <= 1.0:
            raise ValueError(f"ld_clump: p1 {p1}, p2 {p2} (0 <= p1 <= p2 <= 1)")
        if kb is not None and not 0.0 <= float(kb) < 1e12:
            raise ValueError(f"ld_clump: kb {kb} (at least 0, or None)")
        max_dist = None if kb is None else int(float(kb) * 1000)
        if not isinstance(group, str) or group not in self.meta["groups"]:
            raise KeyError(group)
        if not 1 <= window <= 1024:
            raise ValueError(f"ld_clump: window {window} (1 to 1024)")
        _, [(group, lo, hi, _, mask)] = self._query("ld_clump", group, samples, v_lo, v_hi, variant_mask, single=True)
        ctx = self._context()
        p = p if torch.is_tensor(p) else torch.from_numpy(np.ascontiguousarray(p, dtype=np.float64))
        if p.dtype != torch.float64 or tuple(p.shape) != (hi - lo,):
            raise ValueError(f"ld_clump: p {list(p.shape)} {p.dtype}, expected float64 [{hi - lo}]")
        p = p.to(ctx.device)
        finite = torch.isfinite(p)
        if bool((finite & ((p < 0.0) | (p > 1.0))).any()) or bool(torch.isinf(p).any()):
            raise ValueError("ld_clump: a p-value outside [0, 1]")
        take = finite & (p <= p2)
        if mask is not None:
            take &= self._device_bool(mask)
        lo, hi, counted, n, rows = self._ld_rows("ld_clump", group, samples, lo, hi, take, window, slab_bytes, plane_bytes)
        self.stats["ld_pairs"] += self._ld_pairs(n, window)
        nq = -(-window // 64)
        bits = torch.empty((n, nq), dtype=torch.int64, device=ctx.device)
        pos = None
        if max_dist is not None:        # laid out like a tile's rows: `window` places in front of the first variant
            start = torch.from_numpy(self.variants(group)[0][lo:hi].astype(np.int64)).to(ctx.device)[counted]
            pos = torch.cat([torch.zeros(window, dtype=torch.int64, device=ctx.device), start])
            if n > window:
                self.stats["clump_window_short"] += int((start[window:] - start[:-window] <= max_dist).sum())
        tile = max(self._plane_budget(plane_bytes) // (window * 32) - window, LD_MIN_TILE)
        carry = table = None
        k0 = 0                              # the counted index of the next new row
        for new in rows:
            if carry is None:               # before the first variant: rows without a bit
                carry = torch.zeros((3, window, new.shape[2]), dtype=torch.int32, device=ctx.device)
            for t0 in range(0, int(new.shape[1]), tile):
                buf = torch.cat([carry, new[:, t0:t0 + tile]], dim=1)
                m = int(buf.shape[1]) - window
                if table is None or table.shape[0] != buf.shape[1]:
                    table = None
                    table = torch.zeros((buf.shape[1], window, 8), dtype=torch.int32, device=ctx.device)
                else:
                    table.zero_()
                ctx.ld_counts(buf, window, table=table)
                ctx.ld_decisions(table, r2, None if pos is None else pos[k0:k0 + window + m], max_dist, bits=bits[k0:k0 + m])
                carry = buf[:, -window:].contiguous()
                k0 += m
        bits[k0:].zero_()                   # (without a sample there are no rows, and nothing is linked)
        return lo, hi, counted, bits, p[counted]

    def assoc_sums(self, group, W, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None, plane_bytes=None):
        """the sums over samples behind an association scan of a group: a float64 device tensor [n_counted, 3, C] — for
        counted variant v (those of [v_lo, v_hi) that variant_mask marks, in order, as in ld_counts), plane k (ASSOC_HET,
        ASSOC_COMPLETE, ASSOC_ALT: the call is HET, complete, HOM_ALT) and column c, the sum of W[i, c] over the samples i
        whose call at v is of that class.  W: float64 [len(samples), C], host or device, 1 <= C <= 64, row i for
        samples[i] (names or indices; None: every sample, store order).  The samples must be distinct — a regression has
        no use for a row counted twice —: ValueError before anything is allocated.  W is scattered once to the plane
        rows of the samples (zeros elsewhere); the rows of bits come as in ld_counts (hhgt_genotype_planes, then
        hhgt_variant_planes per plane window: slab_bytes and plane_bytes mean what they mean there; cached chunks used,
        the read cache neither filled nor evicted), and every window is reduced by one hhgt_assoc_sums call (the f64
        MFMA; include/hhgt.h states its arithmetic: sums of exactly representable partial sums are exact).  No genotype
        and no dosage is written anywhere."""
        import torch
        idx = self._query("assoc_sums", group, samples, v_lo, v_hi, variant_mask, single=True)[0]
        if len(np.unique(idx)) != len(idx):
            raise ValueError("assoc_sums: a sample is listed twice")
        W = W if torch.is_tensor(W) else torch.from_numpy(np.ascontiguousarray(W))
        if W.dtype != torch.float64 or W.dim() != 2 or W.shape[0] != len(idx) or not 1 <= W.shape[1] <= ASSOC_MAX_COLS:
            raise ValueError(f"assoc_sums: W must be float64 [{len(idx)}, 1 to {ASSOC_MAX_COLS}], not {W.dtype} {list(W.shape)}")
        ctx = self._context()
        n_rows, rows = self._plane_rows(idx)
        sw = -(-n_rows // 32)
        _, _, _, n, vrows = self._variant_rows("assoc_sums", group, idx, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes,
                                               "assoc_plane_blocks")
        d_w = torch.zeros((32 * sw, W.shape[1]), dtype=torch.float64, device=ctx.device)
        d_w[self._to_device(rows)] = W.to(ctx.device)
        parts = [ctx.assoc_sums(v, d_w) for v in vrows]
        self.stats["assoc_variants"] += n
        # (without a sample there is no row of bits: every sum is 0)
        return torch.cat(parts) if parts else torch.zeros((n, 3, W.shape[1]), dtype=torch.float64, device=ctx.device)

    def assoc(self, group, y, covariates=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None,
              plane_bytes=None):
        """single-variant linear regression scan of a group -> (stats, calls) on the device: assoc_design(y, covariates)
        on the host (y [n] or [n, P], covariates [n, q0] or None, row i for samples[i]), assoc_sums of its W (same
        remaining arguments), assoc_from_sums.  stats is float64 [n_counted, P, 4] — ASSOC_BETA, ASSOC_SE, ASSOC_T, ASSOC_P
        of the dosage's coefficient in the fit of each phenotype on [1 | covariates | dosage], a call that is not
        complete imputed to the variant's mean dosage; NaN where the variant is not tested —, calls int64 [n_counted, 3]:
        complete, HET, HOM_ALT calls.  The formulas of assoc_from_sums are the contract; plink2's .glm.linear is not."""
        import torch
        W, q, yy = assoc_design(y, covariates)
        T = self.assoc_sums(group, W, samples, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes)
        return assoc_from_sums(T, torch.from_numpy(W.sum(axis=0)).to(T.device), q, torch.from_numpy(yy).to(T.device))

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
        if len(np.unique(idx)) != len(idx):
            raise ValueError("assoc_logistic: a sample is listed twice")
        Y = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
        Y = Y[:, None] if Y.ndim == 1 else Y
        if Y.ndim != 2 or Y.shape[0] != len(idx):
            raise ValueError(f"assoc_logistic: y of shape {Y.shape} for {len(idx)} samples ([n] or [n, P])")
        designs = [logistic_design(Y[:, p], covariates) for p in range(Y.shape[1])]
        ctx = self._context()
        n_rows, rows = self._plane_rows(idx)
        sw = -(-n_rows // 32)
        _, _, _, n, vrows = self._variant_rows("assoc_logistic", group, idx, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes,
                                               "assoc_plane_blocks")
        d_rows = self._to_device(rows)

        def scattered(a):
            """a [n, ...] on the host -> zeros [32 sw, ...] on the device with a's rows at the samples' plane rows"""
            out = torch.zeros((32 * sw,) + a.shape[1:], dtype=torch.float64, device=ctx.device)
            out[d_rows] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(ctx.device)
            return out

        if test == "wald":
            bits = np.zeros(32 * sw, dtype=np.uint8)
            bits[rows] = 1
            valid = self._to_device(np.packbits(bits, bitorder="little").view(np.int32))
            args = [(valid, scattered(X), scattered(Y[:, p].astype(np.float64)), self._to_device(beta0))
                    for p, (X, beta0) in enumerate(designs)]
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

    def _score_weights(self, who, weights, groups, samples, v_lo, v_hi, variant_mask, inner):
        """score_sums' and score's (`who`) start: `weights` — one array for one group or a dict group -> array, each
        float64 with the axes `inner` ("3VK" or "VK": V the group's range) — against _query -> (idx, queries, {group: host
        array or tensor}, K).  groups = None with a dict: its keys, in order.  KeyError for a listed group without weights,
        ValueError for a shape or dtype that does not fit; nothing is allocated on the device."""
        import torch
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
            w = weights[group] if torch.is_tensor(weights[group]) else np.asarray(weights[group])
            shape = tuple(int(x) for x in w.shape)
            if inner == "VK" and len(shape) == 1:
                w, shape = w[:, None], shape + (1,)
            want = (3, hi - lo) if inner == "3VK" else (hi - lo,)
            if (str(w.dtype).split(".")[-1] != "float64" or len(shape) != len(want) + 1 or shape[:-1] != want
                    or not 1 <= shape[-1] <= SCORE_MAX_COLS or K not in (None, shape[-1])):
                raise ValueError(f"{who}: the weights of {group} must be float64 {list(want)} + [K], 1 <= K <= {SCORE_MAX_COLS}, "
                                 f"the same K in every group, not {w.dtype} {list(shape)}")
            out[group], K = w, shape[-1]
        if K is None:
            raise ValueError(f"{who}: no group")
        return idx, queries, out, K

    def _to_device(self, x):
        """host array or tensor -> a contiguous tensor on the device"""
        import torch
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        return x.to(self._context().device).contiguous()

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
        packed mask; cached chunks used, the read cache neither filled nor evicted) the window's weights are scattered to
        its bit positions and one hhgt_score_sums call (the f64 MFMA; include/hhgt.h states its arithmetic: sums of
        exactly representable partial sums are exact) adds to one table [plane rows, K]; groups, windows and slabs add
        into it and the samples' rows are picked at the end.  No genotype and no dosage is written anywhere."""
        import torch
        idx, queries, weights, K = self._score_weights("score_sums", weights, groups, samples, v_lo, v_hi, variant_mask, "3VK")
        ctx = self._context()
        n_rows, rows = self._plane_rows(idx)
        table = torch.zeros((n_rows, K), dtype=torch.float64, device=ctx.device)
        for group, lo, hi, n_var, mask in queries if len(idx) else ():
            w = self._to_device(weights[group])
            if mask is not None:
                mask = self._device_bool(mask)
                w = self._zero_outside(w, mask)
            for a, b, words, planes in self._plane_walk(group, idx, lo, hi, n_var, "score_plane_blocks", slab_bytes,
                                                        plane_bytes, self._device_mask(mask, lo, n_var)):
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
        freq = np.unique(idx) if freq_samples is None else self._query("score", queries[0][0], freq_samples, single=True)[0]
        ctx = self._context()
        weights, masks, used_n = {}, {}, {}
        offset = torch.zeros(K, dtype=torch.float64, device=ctx.device)
        for group, lo, hi, n_var, mask in queries:
            beta = self._to_device(betas[group])
            if mask is not None:
                masks[group] = mask = self._device_bool(mask)
                beta = self._zero_outside(beta, mask)
            weights[group], off, used = score_class_weights(beta, self.allele_counts(group, freq, lo, hi, slab_bytes), impute)
            offset += off
            used_n[group] = int((used if mask is None else used & mask).sum())
        lo, hi = queries[0][1:3] if len(queries) == 1 else (0, None)
        mask = None if not masks else masks if len(queries) > 1 else masks[queries[0][0]]
        sums = self.score_sums(weights, [q[0] for q in queries], idx, lo, hi, mask, slab_bytes, plane_bytes)
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
        w = weights if torch.is_tensor(weights) else np.asarray(weights)
        shape = tuple(int(x) for x in w.shape)
        if len(shape) == 2:
            w, shape = w[:, :, None], shape + (1,)
        if (str(w.dtype).split(".")[-1] != "float64" or len(shape) != 3 or shape[:2] != (3, n_var)
                or not 1 <= shape[2] <= REGION_MAX_COLS):
            raise ValueError(f"region_sums: the weights of {group} must be float64 [3, {n_var}] + [K], 1 <= K <= {REGION_MAX_COLS}, "
                             f"not {w.dtype} {list(shape)}")
        R, K = len(regions), shape[2]
        n_rows, rows = self._plane_rows(idx)
        _table_budget("region_sums", f"a table of {n_rows} rows x {R} regions x {K} columns ({{}} bytes) exceeds",
                      n_rows * R * K * 8, max_table_bytes)
        ctx = self._context()
        table = torch.zeros((n_rows, R, K), dtype=torch.float64, device=ctx.device)
        if len(idx) and hi > lo:
            w = self._to_device(w[:, lo:hi])
            full = regions[regions[:, 0] < regions[:, 1]]
            covered = np.zeros(hi - lo + 1, np.int64)           # the variants of the hull that lie in at least one region
            np.add.at(covered, full[:, 0] - lo, 1)
            np.add.at(covered, full[:, 1] - lo, -1)
            covered = self._to_device(np.cumsum(covered)[:-1] > 0)
            if mask is not None:
                mask = self._device_bool(mask)[lo:hi]
                w = self._zero_outside(w, mask)
                covered = covered & mask
            bs = self._blocksize()
            for a, b, words, planes in self._plane_walk(group, idx, lo, hi, n_var, "region_plane_blocks", slab_bytes,
                                                        plane_bytes, self._device_mask(mask, lo, n_var)):
                pieces, runs, n_slots = plan_regions(regions, a, b, bs)
                ctx.region_sums(planes, self._window_values(w, lo, a, b, words), pieces, runs, n_slots, R, sums=table, wait=False)
                self.stats["region_pieces"] += len(pieces)
            self.stats["region_variants"] += int(covered.sum())
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
        named = isinstance(weights, str)
        if named and weights != "beta":
            raise ValueError(f"burden: weights {weights!r} (None, \"beta\" or an array)")
        if weights is not None and not named:
            w = weights if torch.is_tensor(weights) else np.asarray(weights)
            shape = tuple(int(x) for x in w.shape)
            if (str(w.dtype).split(".")[-1] != "float64" or len(shape) not in (1, 2) or shape[0] != n_var
                    or not 1 <= (shape + (1,))[1] <= REGION_MAX_COLS):
                raise ValueError(f"burden: the weights of {group} must be float64 [{n_var}] or [{n_var}, K], 1 <= K <= "
                                 f"{REGION_MAX_COLS}, not {w.dtype} {list(shape)}")
        K = 1 if weights is None or named or len(shape) == 1 else shape[1]
        n_rows = self._plane_rows(idx)[0]
        _table_budget("burden", f"a table of {n_rows} rows x {len(regions)} regions x {K} columns ({{}} bytes) exceeds",
                      n_rows * len(regions) * K * 8, max_table_bytes)
        freq = np.unique(idx) if freq_samples is None else self._query("burden", group, freq_samples, single=True)[0]
        ctx = self._context()
        # the allele counts of the regions' hull, zeros (AN == 0: not used) in the rest of the group
        counts = torch.zeros((n_var, 4), dtype=torch.int32, device=ctx.device)
        if hi > lo:
            counts[lo:hi] = self.allele_counts(group, freq, lo, hi, slab_bytes)
        marked = counts[:, AN] > 0
        if mask is not None:
            mask = self._device_bool(mask)
            marked = marked & mask
        used = region_totals(marked.to(torch.float64)[:, None], regions)[:, 0].to(torch.int64)
        if coding == "carrier":
            Wd = torch.stack([torch.zeros(n_var, dtype=torch.float64, device=ctx.device)] + [marked.to(torch.float64)] * 2)
            sums = self.region_sums(group, regions, Wd, idx, mask, slab_bytes, plane_bytes, max_table_bytes)
            return (sums > 0).to(torch.float64), used
        if weights is None:
            w = torch.ones((n_var, 1), dtype=torch.float64, device=ctx.device)
        elif named:
            w = beta_density_weights(counts)[:, None]
        else:
            w = self._to_device(w)
        Wd, o, _ = burden_class_weights(w, counts, impute)
        if mask is not None:
            o = self._zero_outside(o, mask)
        sums = self.region_sums(group, regions, Wd.contiguous(), idx, mask, slab_bytes, plane_bytes, max_table_bytes)
        return sums + region_totals(o, regions)[None], used

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
        ctx = self._context()
        fitted = []
        for group, lo, hi, n_var, mask in queries:
            fitted.append(self._dosages(group, idx, lo, hi, mask, slab_bytes))
        n_variants = sum(int(used.sum()) for _, used in fitted)
        if n_variants == 0:
            raise ValueError("projection_weights: no variant is used")
        out = {}
        for (group, lo, hi, n_var, _), (z, used) in zip(queries, fitted):
            T = self.assoc_sums(group, vectors, idx, lo, hi, used, slab_bytes, plane_bytes)
            counted = torch.nonzero(used).reshape(-1)
            zc = z[:, counted]
            Wd = torch.zeros((3, n_var, vectors.shape[1]), dtype=torch.float64, device=ctx.device)
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
        written anywhere.  Chunks are handled as in allele_counts (cached ones used, the read cache neither filled nor
        evicted).  out: a tensor of the right dtype and shape with dense rows (a row stride of at least M: a slice of a
        wider batch buffer will do), filled in place and returned.  ValueError before X is allocated if it would exceed
        max_bytes (default MAX_FEATURE_BYTES, 4 GiB)."""
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
            freq = np.unique(idx) if freq_samples is None else self._query("feature_matrix", queries[0][0], freq_samples, single=True)[0]
        columns, tables, plans, col0 = [], [], [], 0
        for group, lo, hi, n_var, mask in queries:
            keep = None if mask is None else self._device_bool(mask)
            if not raw:
                counts = (self.allele_counts(group, freq, lo, hi, slab_bytes) if need_counts else
                          torch.zeros((hi - lo, 4), dtype=torch.int32, device=ctx.device))
                values, used = call_class_values(counts, coding, impute)
                if need_counts:
                    keep = used if keep is None else used & keep
            if keep is None:
                counted = torch.arange(lo, hi, dtype=torch.int64, device=ctx.device)
            else:
                counted = torch.nonzero(keep).reshape(-1) + lo
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
        d_map = torch.from_numpy(row_map.view(np.int32)).to(ctx.device)
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
