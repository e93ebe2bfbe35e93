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

# the reference's per-donor record (vcf_to_h5.py:119-127): packed, 35 bytes
SNP_DTYPE = np.dtype([("chrom", "S5"), ("start", np.uint32), ("stop", np.uint32), ("ref", "S10"),
                      ("alt", "S10"), ("phase1", np.int8), ("phase2", np.int8)])
assert SNP_DTYPE.itemsize == 35

# default budget of GenotypeStore's device cache of compressed chunks: a 2504-sample cohort's chunk of 64 x 8192 calls
# compresses to ~0.1-0.2 MiB, so this holds about one chr1-sized group of such a cohort (the cache only grows with use)
DEFAULT_CACHE_BYTES = 256 << 20

# one selection of the window planner: request q, chunk (vcol, scol), Blosc block, decoded bytes [lo, hi) of the block,
# and where they go in the output
PLAN_DTYPE = np.dtype([("req", np.int64), ("vcol", np.int64), ("scol", np.int64), ("block", np.uint32),
                       ("lo", np.uint32), ("hi", np.uint32), ("dst_off", np.uint64)])


def plan_windows(requests, sc, vc, blocksize):
    """(sample, v_lo, v_hi) requests -> (selections PLAN_DTYPE, out_off int64 [n + 1]).  Chunks are (sc, vc, 2) int8,
    sample-major: byte 2v of sample row r = s % sc of chunk column v // vc is chunk byte r*vc*2 + 2*(v % vc) of chunk
    (v // vc, s // sc).  Each range is split at chunk and block boundaries; request q's rows land at
    [out_off[q], out_off[q + 1]) of the output, the requests end to end.  Empty requests give no selection."""
    sc, vc, bs = int(sc), int(vc), int(blocksize)
    out_off = np.zeros(len(requests) + 1, np.int64)
    rows = []
    for q, (s, v_lo, v_hi) in enumerate(requests):
        s, v_lo, v_hi = int(s), int(v_lo), int(v_hi)
        out_off[q + 1] = out_off[q] + 2 * max(v_hi - v_lo, 0)
        if v_hi <= v_lo:
            continue
        scol, r = divmod(s, sc)
        for vcol in range(v_lo // vc, (v_hi - 1) // vc + 1):
            a, b = max(v_lo, vcol * vc), min(v_hi, (vcol + 1) * vc)
            c0 = r * vc * 2 + 2 * (a - vcol * vc)
            c1 = c0 + 2 * (b - a)
            dst = int(out_off[q]) + 2 * (a - v_lo)
            for blk in range(c0 // bs, (c1 - 1) // bs + 1):
                x0, x1 = max(c0, blk * bs), min(c1, (blk + 1) * bs)
                rows.append((q, vcol, scol, blk, x0 - blk * bs, x1 - blk * bs, dst + x0 - c0))
    return np.array(rows, dtype=PLAN_DTYPE), out_off


# columns of GenotypeStore.allele_counts (and of hhgt_count_alleles' counters)
AN, AC, HET, HOM_ALT = 0, 1, 2, 3

# one selection of the count planner: chunk (vcol, scol), Blosc block `part` of its rows, the rows counted (bit r = row r),
# variants [lo, hi) of that block, and the output row of variant lo
COUNT_PLAN_DTYPE = np.dtype([("vcol", np.int64), ("scol", np.int64), ("part", np.uint32), ("row_mask", np.uint64),
                             ("lo", np.uint32), ("hi", np.uint32), ("out_row", np.int64)])


def plan_counts(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize=None):
    """the selections of an allele count (hhgt_count_alleles) over the samples `sample_idx` (indices; each counted once,
    however often it is named) and the variants [v_lo, v_hi) of a group of n_samples x n_variants stored in chunks of
    sc x vc: per chunk row, the selected rows as a 64-bit mask; the variant range cut at chunk columns and at Blosc
    blocks (a row of vc variants is vc * 2 / blocksize blocks of blocksize / 2 variants: its two halves with 8 KiB blocks
    and vc = 8192).  Padded rows (samples >= n_samples) and padded variants (>= n_variants) are never selected.  Chunk
    columns come in order, within one the chunk rows, within a chunk its blocks, so the selections of a chunk are adjacent.
    An empty sample list or range gives no selection."""
    sc, vc, n_samples, n_variants = int(sc), int(vc), int(n_samples), int(n_variants)
    v_lo, v_hi = int(v_lo), int(v_hi)
    bs = min(vc * 2, 8192) if blocksize is None else int(blocksize)
    if not 1 <= sc <= 64 or bs % 2 or (vc * 2) % bs:
        raise ValueError(f"plan_counts: chunks of {sc} x {vc} in blocks of {bs} bytes (1..64 rows, whole blocks per row)")
    if not 0 <= v_lo <= v_hi <= n_variants:
        raise IndexError(f"variants [{v_lo}, {v_hi}) outside 0..{n_variants}")
    s = np.unique(np.asarray(sample_idx, dtype=np.int64).reshape(-1))
    if s.size and (s[0] < 0 or s[-1] >= n_samples):
        raise IndexError(f"sample index outside 0..{n_samples - 1}")
    if s.size == 0 or v_hi == v_lo:
        return np.zeros(0, COUNT_PLAN_DTYPE)
    masks = np.zeros(-(-n_samples // sc), np.uint64)
    np.bitwise_or.at(masks, s // sc, np.left_shift(np.uint64(1), (s % sc).astype(np.uint64)))
    scols = np.nonzero(masks)[0]
    vb = bs // 2
    seg = np.arange(v_lo // vb, (v_hi - 1) // vb + 1, dtype=np.int64)        # blocks of vb variants touched, in order
    a, b = np.maximum(v_lo, seg * vb), np.minimum(v_hi, (seg + 1) * vb)
    out = np.zeros(seg.size * scols.size, COUNT_PLAN_DTYPE)
    rep = lambda x: np.repeat(x, scols.size)
    out["vcol"] = rep(seg * vb // vc)
    out["part"] = rep((seg * vb % vc) // vb)
    out["lo"] = rep(a - seg * vb)
    out["hi"] = rep(b - seg * vb)
    out["out_row"] = rep(a - v_lo)
    out["scol"] = np.tile(scols, seg.size)
    out["row_mask"] = np.tile(masks[scols], seg.size)
    return out[np.lexsort((out["part"], out["scol"], out["vcol"]))]


# one selection of the per-sample count planner: plan_counts' cut, with the output row of chunk row 0 and the first word of
# the block's bits in the packed variant mask
SAMPLE_PLAN_DTYPE = np.dtype([("vcol", np.int64), ("scol", np.int64), ("part", np.uint32), ("row_mask", np.uint64),
                              ("lo", np.uint32), ("hi", np.uint32), ("out_row", np.int64), ("mask_word", np.int64)])


def mask_words_per_block(blocksize):
    """uint32 words a Blosc block of blocksize / 2 variants owns in a packed variant mask: its bits start at a word"""
    return -(-(int(blocksize) // 2) // 32)


def plan_sample_counts(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize=None):
    """the selections of a per-sample count (hhgt_count_samples): plan_counts' cuts of (samples, [v_lo, v_hi)) — the same
    chunks, blocks, row masks and ranges, in the same order —, where chunk row r of chunk row `scol` is counted into
    output row scol * sc + r (the sample's index), and the block's mask bits begin at word (vcol * blocks per row + part) *
    mask_words_per_block(blocksize) of the group's packed variant mask (pack_variant_mask)."""
    sc, vc = int(sc), int(vc)
    bs = min(vc * 2, 8192) if blocksize is None else int(blocksize)
    cut = plan_counts(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize=bs)
    out = np.zeros(len(cut), SAMPLE_PLAN_DTYPE)
    for f in ("vcol", "scol", "part", "row_mask", "lo", "hi"):
        out[f] = cut[f]
    out["out_row"] = cut["scol"] * sc
    out["mask_word"] = (cut["vcol"] * (vc * 2 // bs) + cut["part"].astype(np.int64)) * mask_words_per_block(bs)
    return out


def pack_variant_mask(mask, v_lo, n_variants, vc, blocksize):
    """bool mask [n] over the variants [v_lo, v_lo + n) of a group of n_variants (numpy array or torch tensor, on any
    device) -> the group's variant mask as hhgt_count_samples reads it: uint32 words (numpy: uint32; torch: int32 on the
    mask's device, the same bits), mask_words_per_block words per Blosc block of every chunk column, variant v of a block
    at bit v % 32 of the block's word v // 32.  Variants outside [v_lo, v_lo + n) and the padding are 0."""
    vc, bs, v_lo, n_variants = int(vc), int(blocksize), int(v_lo), int(n_variants)
    vb, wpb = bs // 2, mask_words_per_block(bs)
    n = int(mask.shape[0])
    if mask.ndim != 1 or not 0 <= v_lo <= v_lo + n <= n_variants:
        raise IndexError(f"variant mask of shape {tuple(mask.shape)} at {v_lo} outside 0..{n_variants}")
    n_bits = -(-n_variants // vc) * (vc // vb) * wpb * 32
    if isinstance(mask, np.ndarray):
        v = np.arange(v_lo, v_lo + n, dtype=np.int64)
        bits = np.zeros(n_bits, bool)
        bits[v // vb * (wpb * 32) + v % vb] = mask.astype(bool)
        return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)
    import torch
    v = torch.arange(v_lo, v_lo + n, dtype=torch.int64, device=mask.device)
    bits = torch.zeros(n_bits, dtype=torch.uint8, device=mask.device)
    bits[v // vb * (wpb * 32) + v % vb] = mask.to(torch.uint8)
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=mask.device)
    return (bits.view(-1, 8) * weights).sum(1).to(torch.uint8).view(torch.int32)      # (little-endian words)


# columns of GenotypeStore.pair_counts (and of hhgt_pair_counts' table), for the ordered pair (i, j) over the counted variants.
# A call is complete iff both alleles are 0 or 1; a missing allele or an allele >= 2 takes the call out of every column.
NSNP, HETHET, IBS0, HET1 = 0, 1, 2, 3    # both complete; both HET; opposite homozygotes; i HET and j complete

# default budgets of GenotypeStore.pair_counts: the plane buffer of one window of variants, and the largest table it makes
DEFAULT_PLANE_BYTES = 1 << 30
MAX_PAIR_TABLE_BYTES = 2 << 30

# one selection of the plane planner: plan_sample_counts' record (out_row: the plane row of chunk row 0) plus the first word
# of the block's bits in a plane row
PLANE_PLAN_DTYPE = np.dtype([("vcol", np.int64), ("scol", np.int64), ("part", np.uint32), ("row_mask", np.uint64),
                             ("lo", np.uint32), ("hi", np.uint32), ("out_row", np.int64), ("mask_word", np.int64),
                             ("out_word", np.int64)])


def plane_rows(sample_idx, sc):
    """the plane rows of a sample list: chunk rows without a listed sample get none, the others sc rows each in order ->
    (scols: the chunk rows kept, ascending; rows int64 [len(sample_idx)]: the plane row of each listed sample)"""
    s = np.asarray(sample_idx, dtype=np.int64).reshape(-1)
    scols = np.unique(s // int(sc))
    return scols, np.searchsorted(scols, s // int(sc)) * int(sc) + s % int(sc)


def plan_planes(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize=None, block0=None):
    """the selections of hhgt_genotype_planes: plan_counts' cuts of (samples, [v_lo, v_hi)) — the same chunks, blocks, row
    masks and ranges, in the same order, mask_word as plan_sample_counts gives it —, with the plane rows compacted by chunk
    row (plane_rows: the k-th chunk row that has a selected sample owns plane rows [k * sc, (k + 1) * sc)) and the bits of
    block B of the group (B = v // (blocksize / 2)) at word (B - block0) * mask_words_per_block(blocksize) of a plane row;
    block0: the first block of the plane buffer (default: the block of v_lo)."""
    sc, vc = int(sc), int(vc)
    bs = min(vc * 2, 8192) if blocksize is None else int(blocksize)
    cut = plan_sample_counts(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize=bs)
    vb, wpb = bs // 2, mask_words_per_block(bs)
    block0 = int(v_lo) // vb if block0 is None else int(block0)
    out = np.zeros(len(cut), PLANE_PLAN_DTYPE)
    for f in ("vcol", "scol", "part", "row_mask", "lo", "hi", "mask_word"):
        out[f] = cut[f]
    scols = np.unique(cut["scol"])
    out["out_row"] = np.searchsorted(scols, cut["scol"]) * sc
    out["out_word"] = (cut["vcol"] * (vc // vb) + cut["part"].astype(np.int64) - block0) * wpb
    if len(out) and int(out["out_word"].min()) < 0:
        raise IndexError(f"plan_planes: block0 {block0} lies behind variant {int(v_lo)}")
    return out


def plane_windows(v_lo, v_hi, blocksize, n_rows, plane_bytes):
    """[v_lo, v_hi) cut at Blosc block boundaries into windows whose plane buffer (3 planes x n_rows rows x the words of the
    window's blocks) is at most plane_bytes, one block at least -> list of (a, b), in order, covering the range once"""
    v_lo, v_hi, vb = int(v_lo), int(v_hi), int(blocksize) // 2
    per_block = 3 * max(int(n_rows), 1) * mask_words_per_block(blocksize) * 4
    step = max(int(plane_bytes) // per_block, 1) * vb
    out, a = [], v_lo
    while a < v_hi:
        b = min((a // vb) * vb + step, v_hi)
        out.append((a, b))
        a = b
    return out


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def ibs_counts(table):
    """pair table [n, n, 4] (numpy or torch, any integer type) -> (IBS0, IBS1, IBS2), int64 [n, n] each: the variants at
    which a pair's complete calls share no, one, both alleles.  IBS2 = 2 HETHET + NSNP - HET1[i][j] - HET1[j][i] - IBS0
    (identical genotypes), IBS1 = NSNP - IBS0 - IBS2."""
    if _is_torch(table):
        import torch
        t = table.to(torch.int64)
        h2 = t[..., HET1].transpose(0, 1)
    else:
        t = np.asarray(table).astype(np.int64)
        h2 = t[..., HET1].T
    ibs2 = 2 * t[..., HETHET] + t[..., NSNP] - t[..., HET1] - h2 - t[..., IBS0]
    return t[..., IBS0], t[..., NSNP] - t[..., IBS0] - ibs2, ibs2


def kinship_from_counts(table):
    """pair table [n, n, 4] (numpy or torch) -> float64 [n, n]: the KING-robust between-family kinship estimator
    (Manichaikul et al. 2010) as this project defines it,
        phi = 1/2 - (4 IBS0 + HET1[i][j] + HET1[j][i] - 2 HETHET) / (4 min(HET1[i][j], HET1[j][i])),
    in float64 from the integer table, NaN where the minimum is 0.  A sample against itself or against a duplicate gives
    exactly 0.5.  The formula is the contract: equality with plink2's KINSHIP column is neither claimed nor tested."""
    if _is_torch(table):
        import torch
        t = table.to(torch.int64)
        h1, h2 = t[..., HET1], t[..., HET1].transpose(0, 1)
        num = (4 * t[..., IBS0] + h1 + h2 - 2 * t[..., HETHET]).to(torch.float64)
        den = (4 * torch.minimum(h1, h2)).to(torch.float64)
        return torch.where(den > 0, 0.5 - num / den, torch.full_like(den, float("nan")))
    t = np.asarray(table).astype(np.int64)
    h1, h2 = t[..., HET1], t[..., HET1].T
    num = (4 * t[..., IBS0] + h1 + h2 - 2 * t[..., HETHET]).astype(np.float64)
    den = (4 * np.minimum(h1, h2)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, 0.5 - num / den, np.nan)


# columns of GenotypeStore.ld_counts (and of hhgt_ld_counts' table), for the ordered pair (u, v) of counted variants, v after
# u, over the counted samples: M = the call is complete, H = HET, A = HOM_ALT.  The dosage of a complete call is 0, 1, 2.
LD_N, LD_HM, LD_AM, LD_MH, LD_MA = 0, 1, 2, 3, 4     # Mu Mv; Hu Mv; Au Mv; Mu Hv; Mu Av
LD_HH, LD_HA, LD_AA = 5, 6, 7                        # Hu Hv; Hu Av or Au Hv; Au Av

# the smallest tile of GenotypeStore.ld_prune, in counted variants
LD_MIN_TILE = 64


def plane_positions(v_lo, v_hi, blocksize, block0=None):
    """the bit positions of the variants [v_lo, v_hi) of a group in a plane row whose first block is block0 (default: the
    block of v_lo), as plan_planes lays them out -> int64 [v_hi - v_lo]: variant v of block B = v // (blocksize / 2) sits
    at bit (B - block0) * 32 * mask_words_per_block(blocksize) + v % (blocksize / 2).  The padding of a block whose
    blocksize / 2 variants do not fill whole words is nobody's position."""
    v_lo, v_hi, vb = int(v_lo), int(v_hi), int(blocksize) // 2
    block0 = v_lo // vb if block0 is None else int(block0)
    if v_hi < v_lo or block0 * vb > v_lo:
        raise IndexError(f"plane_positions: variants [{v_lo}, {v_hi}) in a row that begins at block {block0}")
    v = np.arange(v_lo, v_hi, dtype=np.int64)
    return (v // vb - block0) * (32 * mask_words_per_block(blocksize)) + v % vb


def ld_sums(table):
    """LD table [..., 8] (numpy or torch, any integer type) -> (n, sx, sy, sxx, syy, sxy), int64 each: over the samples at
    which both calls of a pair are complete, their number and the sums of the dosages x (first variant) and y (second),
    of their squares and of their products: sx = HM + 2 AM, sxx = HM + 4 AM, sy = MH + 2 MA, syy = MH + 4 MA,
    sxy = HH + 2 HA + 4 AA."""
    if _is_torch(table):
        import torch
        t = table.to(torch.int64)
    else:
        t = np.asarray(table).astype(np.int64)
    return (t[..., LD_N], t[..., LD_HM] + 2 * t[..., LD_AM], t[..., LD_MH] + 2 * t[..., LD_MA],
            t[..., LD_HM] + 4 * t[..., LD_AM], t[..., LD_MH] + 4 * t[..., LD_MA],
            t[..., LD_HH] + 2 * t[..., LD_HA] + 4 * t[..., LD_AA])


def _ld_products(table):
    """-> (num * num, dx * dy) of an LD table, float64: num = N sxy - sx sy, dx = N sxx - sx^2, dy = N syy - sy^2 in int64,
    converted, and the two products, each rounded once"""
    n, sx, sy, sxx, syy, sxy = ld_sums(table)
    num, dx, dy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    if _is_torch(table):
        import torch
        num, dx, dy = num.to(torch.float64), dx.to(torch.float64), dy.to(torch.float64)
    else:
        num, dx, dy = num.astype(np.float64), dx.astype(np.float64), dy.astype(np.float64)
    return num * num, dx * dy


def r2_from_counts(table):
    """LD table [n, W, 8] (numpy or torch) -> float64 [n, W]: r^2 = (num * num) / (dx * dy) with num = N sxy - sx sy,
    dx = N sxx - sx^2, dy = N syy - sy^2 of ld_sums — the squared Pearson correlation of the two variants' dosages over
    the samples at which both calls are complete (unphased).  NaN where dx * dy = 0: one of the two is monomorphic among
    those samples, or there are none.  A variant against a duplicate of itself gives exactly 1.0.  The formula is the
    contract: equality with plink2's --r2-unphased column is neither claimed nor tested."""
    nn, den = _ld_products(table)
    if _is_torch(table):
        import torch
        return torch.where(den != 0, nn / den, torch.full_like(den, float("nan")))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0, nn / den, np.nan)


def ld_exceeds(table, r2):
    """LD table [n, W, 8] (numpy or torch) -> bool [n, W]: num * num > r2 * (dx * dy), the three products in float64 and
    each rounded once — the decision hhgt_ld_prune makes from the same integers, bit for bit.  A pair whose r^2 is NaN
    (zero denominator) never exceeds."""
    nn, den = _ld_products(table)
    return nn > float(r2) * den


class StoreWriter:
    def __init__(self, path, samples, sc, vc, typesize=2, cohort_name="", donor_ids=None, chunk_format="blosc2"):
        self.path = path
        os.makedirs(path, exist_ok=True)
        assert chunk_format in ("blosc1", "blosc2")
        self.meta = dict(format="hhgt-store", version=1, cohort_name=cohort_name, samples=list(samples),
                         donor_ids=list(donor_ids) if donor_ids is not None else list(samples),
                         sc=int(sc), vc=int(vc), typesize=int(typesize), blocksize=min(int(vc) * 2, 8192),
                         chunk_format=chunk_format,
                         codec=f"{chunk_format}: byte-shuffle + LZ4 block format", groups={})
        self._cur = None

    def begin_group(self, group):
        d = os.path.join(self.path, group)
        os.makedirs(d, exist_ok=True)
        self._cur = dict(name=group, dir=d, f=open(os.path.join(d, "chunks.bin"), "wb", buffering=0), offsets=[0],
                         start=[], ref=[], alt=[], runs=[], n_variants=0, raw_bytes=0)

    def add_chunks(self, data, offsets, raw_bytes):
        """data: bytes-like of concatenated framed chunks; offsets: uint64 relative offsets [k+1]"""
        from .h5file import H5Writer
        c = self._cur
        base = c["offsets"][-1]
        mv = memoryview(data).cast("B")
        n, fd = len(mv), c["f"].fileno()
        if n >= H5Writer.PAR_MIN and H5Writer.PAR_THREADS > 1:     # large batches: several pwrite threads (see H5Writer.append)
            if getattr(self, "_pool", None) is None:
                from concurrent.futures import ThreadPoolExecutor
                self._pool = ThreadPoolExecutor(H5Writer.PAR_THREADS)
            step = -(-(-(-n // H5Writer.PAR_THREADS)) // 4096) * 4096
            for fut in [self._pool.submit(H5Writer._pwrite_all, fd, mv[o:o + step], base + o) for o in range(0, n, step)]:
                fut.result()
        else:
            H5Writer._pwrite_all(fd, mv, base)
        c["offsets"].extend(int(base + o) for o in offsets[1:])
        c["raw_bytes"] += int(raw_bytes)

    def add_variants(self, start, ref, alt):
        c = self._cur
        c["start"].append(np.asarray(start, np.uint32).copy())
        c["ref"].append(np.asarray(ref, np.uint8).copy())
        c["alt"].append(np.asarray(alt, np.uint8).copy())
        c["n_variants"] += len(start)

    def add_chrom_runs(self, runs):
        self._cur["runs"].extend([(int(a), str(b)) for a, b in runs])

    def end_group(self):
        c = self._cur
        c["f"].close()
        np.save(os.path.join(c["dir"], "offsets.npy"), np.asarray(c["offsets"], np.uint64))
        for k in ("start", "ref", "alt"):
            arr = np.concatenate(c[k]) if c[k] else np.zeros(0, np.uint32 if k == "start" else np.uint8)
            np.save(os.path.join(c["dir"], k + ".npy"), arr)
        json.dump(c["runs"], open(os.path.join(c["dir"], "chrom_runs.json"), "w"))
        S, sc, vc = len(self.meta["samples"]), self.meta["sc"], self.meta["vc"]
        # a file with no kept SNP gives a group with no chunk column
        self.meta["groups"][c["name"]] = dict(n_variants=c["n_variants"], n_vcol=-(-c["n_variants"] // vc),
                                              n_scol=-(-max(S, 1) // sc), n_chunks=len(c["offsets"]) - 1,
                                              compressed_bytes=c["offsets"][-1], raw_bytes=c["raw_bytes"])
        self._cur = None

    def close(self):
        if getattr(self, "_pool", None) is not None:
            self._pool.shutdown()
            self._pool = None
        json.dump(self.meta, open(os.path.join(self.path, "meta.json"), "w"), indent=1)


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
        # host counters of read_windows: chunks and compressed bytes read from the file, Blosc blocks decoded and their
        # decoded size (the kernel decodes a block whole and writes the selected range of it)
        self.stats = dict(chunks_read=0, compressed_bytes_read=0, blocks_decoded=0, bytes_decoded=0)
        # and of allele_counts: Blosc blocks it decoded, compressed bytes it read from the file (cache hits not included)
        self.stats.update(count_blocks=0, count_compressed_bytes_read=0)
        # and of sample_counts (which shares count_compressed_bytes_read with it): Blosc blocks it decoded
        self.stats.update(sample_count_blocks=0)
        # and of pair_counts: Blosc blocks its first stage decoded, plane words per row its second stage read
        self.stats.update(pair_plane_blocks=0, pair_words=0)
        # and of ld_counts / ld_prune: Blosc blocks their plane stage decoded, pairs of counted variants they counted
        self.stats.update(ld_plane_blocks=0, ld_pairs=0)
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
            meta.setdefault("blocksize", min(vc * 2, 8192))
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
            n_var = self.meta["groups"][group]["n_variants"]
            v_lo, v_hi = int(v_lo), int(v_hi)
            if not 0 <= v_lo <= v_hi <= n_var:
                raise IndexError(f"variants [{v_lo}, {v_hi}) outside {group} (0..{n_var})")
            norm.append((group, self._sample_index(sample), v_lo, v_hi))
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
            # one host-to-device copy of all misses; then every cached chunk gets its own allocation (a device copy), so
            # evicting a chunk frees its bytes and the cache holds no more than its budget
            host = np.concatenate(list(missing.values()))
            dev = torch.from_numpy(host).to(ctx.device)
            pos = 0
            for k, a in missing.items():
                chunks[k] = dev if len(missing) == 1 else dev[pos:pos + a.size].clone()
                pos += a.size
                self._cache[k] = chunks[k]
                self._cache_used += a.size
            del dev
            self.stats["chunks_read"] += len(missing)
            self.stats["compressed_bytes_read"] += int(host.size)
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
        sc, vc = self.meta["sc"], self.meta["vc"]
        g = self.meta["groups"][group]
        n_var = g["n_variants"]
        v_hi = n_var if v_hi is None else int(v_hi)
        v_lo = int(v_lo)
        if not 0 <= v_lo <= v_hi <= n_var:
            raise IndexError(f"variants [{v_lo}, {v_hi}) outside {group} (0..{n_var})")
        idx = (np.arange(len(self.samples)) if samples is None else
               np.array([self._sample_index(x) for x in samples], dtype=np.int64))
        bs = self._blocksize()
        plan = plan_counts(idx, len(self.samples), sc, vc, n_var, v_lo, v_hi, blocksize=bs)
        counts = torch.zeros((v_hi - v_lo, 4), dtype=torch.int32, device=ctx.device)
        if not len(plan):
            return counts
        self._run_plan(group, plan, slab_bytes, COUNT_SEL_DTYPE, "count_blocks", lambda dsel: ctx.count_alleles(
            dsel, sc, vc, typesize=self.meta["typesize"], blocksize=bs, counts=counts))
        return counts

    def _run_plan(self, group, plan, slab_bytes, sel_dtype, stat_key, call):
        """runs the selections `plan` of a group through a row kernel, slab by slab (_scan_slabs): a slab's selections
        become sel_dtype records — the chunk's address and size from the slab, every other field the plan has from the
        plan —, call(records) -> (_, n_bad) launches them and synchronises; RuntimeError if a selection was bad;
        stats[stat_key] counts the blocks decoded (one per selected row and selection)."""
        fields = [f for f in sel_dtype.names if f in plan.dtype.names]
        blocks = np.array([bin(int(m)).count("1") for m in plan["row_mask"]], np.int64)

        def launch(chunks, keys, rows):
            dsel = np.zeros(len(rows), sel_dtype)
            dsel["src_ptr"] = [chunks[keys[i]].data_ptr() for i in rows]
            dsel["src_bytes"] = [chunks[keys[i]].numel() for i in rows]
            for f in fields:
                dsel[f] = plan[f][rows]
            _, bad = call(dsel)
            if bad:
                raise RuntimeError(f"{bad} corrupt chunk(s) in {group}")
            self.stats[stat_key] += int(blocks[rows].sum())

        self._scan_slabs(group, plan, slab_bytes, launch)

    def _scan_slabs(self, group, plan, slab_bytes, launch):
        """the chunk handling of a count over the selections `plan` (vcol / scol per selection, plan order: chunk columns
        in order) of a group: chunks in the read cache are used as they are, the rest read from the file and uploaded in
        slabs of at most slab_bytes (default: the cache budget; a larger chunk goes alone), one copy per slab; then
        launch(chunks, keys, rows) runs the slab's selections — chunks: key -> device tensor, keys[i]: the chunk of
        selection i, rows: the slab's selections — and must synchronise, for the slab is freed behind it.  The cache is
        neither filled nor evicted."""
        budget = self.cache_bytes if slab_bytes is None else int(slab_bytes)
        keys = [(group, self._chunk_id(group, int(v), int(c))) for v, c in zip(plan["vcol"], plan["scol"])]
        run = lambda chunks, rows: launch(chunks, keys, rows)
        slab, rows, host, size = {}, [], [], 0
        for i, k in enumerate(keys):
            if k not in slab:
                if k in self._cache:
                    slab[k] = self._cache[k]
                else:
                    a = self._read_chunk(group, int(plan["vcol"][i]), int(plan["scol"][i]))
                    if host and size + a.size > budget:
                        self._count_slab(slab, host, rows, run)
                        slab, rows, host, size = {}, [], [], 0
                    slab[k] = None
                    host.append((k, a))
                    size += a.size
            rows.append(i)
        self._count_slab(slab, host, rows, run)

    def _count_slab(self, slab, host, rows, launch):
        """uploads the chunks read for one slab of a count in one copy, then runs its selections"""
        import torch
        if host:
            cat = np.concatenate([a for _, a in host])
            dev = torch.from_numpy(cat).to(self._context().device)
            pos = 0
            for k, a in host:
                slab[k] = dev[pos:pos + a.size]
                pos += a.size
            self.stats["count_compressed_bytes_read"] += int(cat.size)
        if rows:
            launch(slab, rows)          # (synchronises: the slab's memory is free to go when this returns)

    def _group_list(self, groups):
        names = self.groups() if groups is None else [groups] if isinstance(groups, str) else list(groups)
        for g in names:
            if g not in self.meta["groups"]:
                raise KeyError(g)
        return names

    def _group_queries(self, who, groups, samples, v_lo, v_hi, variant_mask):
        """what sample_counts and pair_counts (`who`, for the messages) do with their arguments first -> (idx, queries):
        idx, the sample indices (int64 array), and a generator of (group, lo, hi, n_var, vmask) per group — its variant
        range, checked, and its variant mask packed (pack_variant_mask) and on the device, or None."""
        import torch
        bs = self._blocksize()
        names = self._group_list(groups)
        if len(names) != 1 and (int(v_lo) != 0 or v_hi is not None):
            raise ValueError(f"{who}: v_lo / v_hi need a single group")
        if isinstance(variant_mask, dict):
            for g in variant_mask:
                if g not in names:
                    raise KeyError(g)
            masks = variant_mask
        elif variant_mask is not None:
            if len(names) != 1:
                raise ValueError(f"{who}: one variant_mask needs a single group (several: a dict group -> mask)")
            masks = {names[0]: variant_mask}
        else:
            masks = {}
        idx = (np.arange(len(self.samples)) if samples is None else
               np.array([self._sample_index(x) for x in samples], dtype=np.int64).reshape(-1))

        def queries():
            for group in names:
                n_var = self.meta["groups"][group]["n_variants"]
                lo, hi = (int(v_lo), n_var if v_hi is None else int(v_hi)) if len(names) == 1 else (0, n_var)
                if not 0 <= lo <= hi <= n_var:
                    raise IndexError(f"variants [{lo}, {hi}) outside {group} (0..{n_var})")
                vmask = None
                if group in masks:
                    m = masks[group]
                    if m.ndim != 1 or int(m.shape[0]) != hi - lo:
                        raise ValueError(f"variant_mask of {group}: shape {tuple(m.shape)}, expected ({hi - lo},)")
                    vmask = pack_variant_mask(m, lo, n_var, self.meta["vc"], bs)
                    if not torch.is_tensor(vmask):          # a host mask goes up once, not with every slab
                        vmask = torch.from_numpy(vmask.view(np.int32)).to(self._context().device)
                yield group, lo, hi, n_var, vmask

        return idx, queries()

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
        idx, queries = self._group_queries("sample_counts", groups, samples, v_lo, v_hi, variant_mask)
        table = torch.zeros((-(-max(len(self.samples), 1) // sc) * sc, 4), dtype=torch.int32, device=ctx.device)
        for group, lo, hi, n_var, vmask in queries:
            plan = plan_sample_counts(idx, len(self.samples), sc, vc, n_var, lo, hi, blocksize=bs)
            self._run_plan(group, plan, slab_bytes, SAMPLE_SEL_DTYPE, "sample_count_blocks",
                           lambda dsel, vmask=vmask: ctx.count_samples(dsel, sc, vc, typesize=self.meta["typesize"],
                                                                       blocksize=bs, vmask=vmask, counts=table))
        return table[torch.from_numpy(idx).to(ctx.device)]

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
        from .device import PLANE_SEL_DTYPE
        sc, vc, bs = self.meta["sc"], self.meta["vc"], self._blocksize()
        idx, queries = self._group_queries("pair_counts", groups, samples, v_lo, v_hi, variant_mask)
        scols, rows = plane_rows(idx, sc)
        n_rows = len(scols) * sc
        limit = MAX_PAIR_TABLE_BYTES if max_table_bytes is None else int(max_table_bytes)
        if n_rows * n_rows * 16 > limit:
            raise ValueError(f"pair_counts: a table of {n_rows} x {n_rows} pairs ({n_rows * n_rows * 16} bytes) exceeds "
                             f"max_table_bytes = {limit}")
        ctx = self._context()
        table = torch.zeros((n_rows, n_rows, 4), dtype=torch.int32, device=ctx.device)
        budget = DEFAULT_PLANE_BYTES if plane_bytes is None else int(plane_bytes)
        vb, wpb = bs // 2, mask_words_per_block(bs)
        for group, lo, hi, n_var, vmask in queries:
            if n_rows == 0:
                continue
            planes = None
            for a, b in plane_windows(lo, hi, bs, n_rows, budget):
                words = ((b - 1) // vb - a // vb + 1) * wpb
                if planes is None or planes.shape[2] != words:
                    planes = None                       # (the last window of a range may be shorter)
                    planes = torch.zeros((3, n_rows, words), dtype=torch.int32, device=ctx.device)
                else:
                    planes.zero_()
                plan = plan_planes(idx, len(self.samples), sc, vc, n_var, a, b, blocksize=bs)
                self._run_plan(group, plan, slab_bytes, PLANE_SEL_DTYPE, "pair_plane_blocks",
                               lambda dsel, vmask=vmask, planes=planes: ctx.genotype_planes(
                                   dsel, sc, vc, typesize=self.meta["typesize"], blocksize=bs, vmask=vmask, planes=planes))
                ctx.pair_counts(planes, 0, words, table=table)
                self.stats["pair_words"] += words
        pick = torch.from_numpy(rows).to(ctx.device)
        return table[pick][:, pick].contiguous()

    def kinship(self, groups=None, samples=None, v_lo=0, v_hi=None, variant_mask=None, slab_bytes=None, plane_bytes=None,
                max_table_bytes=None):
        """KING-robust kinship of every pair of `samples` from pair_counts (same arguments): a float64 device tensor [n, n],
        kinship_from_counts' formula — NaN where a pair has no heterozygous call to divide by, exactly 0.5 for a sample
        against itself or a duplicate.  The formula there is the contract; plink2's KINSHIP column is not."""
        return kinship_from_counts(self.pair_counts(groups, samples, v_lo, v_hi, variant_mask, slab_bytes, plane_bytes,
                                                    max_table_bytes))

    def _ld_rows(self, who, group, samples, v_lo, v_hi, variant_mask, window, slab_bytes, plane_bytes):
        """what ld_counts and ld_prune (`who`, for the messages) do alike -> (lo, hi, counted, n_counted, rows): the range,
        checked; the offsets into it of the variants the mask marks, an int64 device tensor, or None; the number of counted variants (with a mask
        it comes from the device, together with the number of counted variants per plane window: one small copy per call,
        whatever the number of windows); and a generator of int32 device tensors [3, m, sw], the variant-major
        planes (HET, COMPLETE, HOM_ALT over the plane rows of `samples`) of the counted variants, in order, plane window by
        plane window: the planes come as in pair_counts (cached chunks used, the read cache neither filled nor evicted;
        no variant mask there), each window is transposed (hhgt_variant_planes) and the rows at plane_positions of the
        counted variants gathered, which leaves out block padding and masked variants in one step."""
        import torch
        from .device import PLANE_SEL_DTYPE
        if not isinstance(group, str) or group not in self.meta["groups"]:
            raise KeyError(group)
        window = int(window)
        if not 1 <= window <= 1024:
            raise ValueError(f"{who}: window {window} (1 to 1024)")
        ctx = self._context()
        sc, vc, bs = self.meta["sc"], self.meta["vc"], self._blocksize()
        n_var = self.meta["groups"][group]["n_variants"]
        lo, hi = int(v_lo), n_var if v_hi is None else int(v_hi)
        if not 0 <= lo <= hi <= n_var:
            raise IndexError(f"variants [{lo}, {hi}) outside {group} (0..{n_var})")
        idx = (np.arange(len(self.samples)) if samples is None else
               np.array([self._sample_index(x) for x in samples], dtype=np.int64).reshape(-1))
        mask = None
        if variant_mask is not None:
            if variant_mask.ndim != 1 or int(variant_mask.shape[0]) != hi - lo:
                raise ValueError(f"variant_mask of {group}: shape {tuple(variant_mask.shape)}, expected ({hi - lo},)")
            mask = (variant_mask if torch.is_tensor(variant_mask) else
                    torch.from_numpy(np.ascontiguousarray(variant_mask, dtype=bool))).to(ctx.device).to(torch.bool)
        n_rows = len(plane_rows(idx, sc)[0]) * sc
        budget = DEFAULT_PLANE_BYTES if plane_bytes is None else int(plane_bytes)
        vb, wpb = bs // 2, mask_words_per_block(bs)
        windows = plane_windows(lo, hi, bs, n_rows, budget) if n_rows else []
        if mask is None:
            n_counted, counted, cuts = hi - lo, None, None
        else:
            # the counted variants (offsets into the range) stay on the device; what comes back, in one copy for the whole
            # call, is how many of them lie before each plane window's end
            counted = torch.nonzero(mask).reshape(-1)
            ends = torch.tensor([0] + [b - lo for _, b in windows] + [hi - lo], dtype=torch.int64, device=ctx.device)
            cuts = torch.searchsorted(counted, ends).cpu().tolist()
            n_counted = cuts[-1]

        def rows():
            planes = None
            for w, (a, b) in enumerate(windows):
                words = ((b - 1) // vb - a // vb + 1) * wpb
                if planes is None or planes.shape[2] != words:
                    planes = None                       # (the last window of a range may be shorter)
                    planes = torch.zeros((3, n_rows, words), dtype=torch.int32, device=ctx.device)
                else:
                    planes.zero_()
                plan = plan_planes(idx, len(self.samples), sc, vc, n_var, a, b, blocksize=bs)
                self._run_plan(group, plan, slab_bytes, PLANE_SEL_DTYPE, "ld_plane_blocks",
                               lambda dsel, planes=planes: ctx.genotype_planes(
                                   dsel, sc, vc, typesize=self.meta["typesize"], blocksize=bs, planes=planes))
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
        limit = MAX_PAIR_TABLE_BYTES if max_table_bytes is None else int(max_table_bytes)
        if n * window * 32 > limit:
            raise ValueError(f"ld_counts: a table of {n} x {window} pairs ({n * window * 32} bytes) exceeds "
                             f"max_table_bytes = {limit}")
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
        budget = DEFAULT_PLANE_BYTES if plane_bytes is None else int(plane_bytes)
        tile = max(budget // (window * 32) - window, LD_MIN_TILE)
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

    def variant_mask(self, group, samples=None, v_lo=0, v_hi=None, min_maf=None, max_ac=None, min_ac=None):
        """a class of the variants [v_lo, v_hi) of a group, from allele_counts over `samples` (same arguments), as a bool
        device tensor [v_hi - v_lo] that sample_counts takes as variant_mask; nothing is copied to the host.  A variant
        is kept iff it passes every bound given: min_maf — AN > 0 and min(AC, AN - AC) >= min_maf * AN, compared as
        float64 —; min_ac <= AC; AC <= max_ac (integers; singletons: min_ac = max_ac = 1).  No bound: every variant."""
        import torch
        c = self.allele_counts(group, samples, v_lo, v_hi)
        an, ac = c[:, AN].to(torch.int64), c[:, AC].to(torch.int64)
        keep = torch.ones(c.shape[0], dtype=torch.bool, device=c.device)
        if min_maf is not None:
            keep &= (an > 0) & (torch.minimum(ac, an - ac).double() >= float(min_maf) * an.double())
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
        start, ref, alt, runs = tables if tables is not None else self.variants(group)
        n = len(start)
        v_hi = n if v_hi is None else v_hi
        if v_lo == 0 and v_hi == n:
            ph = self.sample_row(group, sample)
        else:
            ph = self.read_windows([(group, sample, v_lo, v_hi)])[0].cpu().numpy()
        rec = np.zeros(v_hi - v_lo, dtype=SNP_DTYPE)
        bounds = [r[0] for r in runs] + [n]
        for (a, name), b in zip(runs, bounds[1:]):
            a, b = max(a, v_lo), min(b, v_hi)
            if a < b:
                rec["chrom"][a - v_lo:b - v_lo] = name.encode()[:5]
        rec["start"] = start[v_lo:v_hi]
        rec["stop"] = start[v_lo:v_hi] + 1
        rec["ref"] = ref[v_lo:v_hi].view("S1")
        rec["alt"] = alt[v_lo:v_hi].view("S1")
        rec["phase1"] = ph[:, 0]
        rec["phase2"] = ph[:, 1]
        return rec


DONOR_CHUNK_ROWS = 7488          # 8 Blosc blocks of 936 records (32 760 B = the largest multiple of 35 under 32 KiB)


def _h5_strings(xs):
    n = max([len(x.encode()) for x in xs] + [1])
    return np.array([x.encode() for x in xs], dtype=f"S{n}")


def _h5_group_datasets(w, group, meta, g, base, off, start, ref, alt, runs):
    """the datasets of group chr_{N} (see export_h5): the chunk index of /genotype over chunk bytes already in the file at
    base + off[k], and the variant tables"""
    from .h5file import FILTER_BLOSC, blosc_cd_values
    sc, vc, S = meta["sc"], meta["vc"], len(meta["samples"])
    off = np.asarray(off, np.uint64)
    ids = np.arange(len(off) - 1)
    vcol, scol = ids // max(g["n_scol"], 1), ids % max(g["n_scol"], 1)
    chunks = [((int(sci) * sc, int(vci) * vc, 0), base + int(o0), int(o1 - o0))
              for sci, vci, o0, o1 in zip(scol, vcol, off[:-1], off[1:])]
    w.add_chunked(group, "genotype", (S, g["n_variants"], 2), np.int8, (sc, vc, 2), chunks, filter_id=FILTER_BLOSC,
                  cd_values=blosc_cd_values(meta["typesize"], sc * vc * 2), filter_name=b"blosc")
    start = np.asarray(start)
    w.add_array(group, "start", start.astype(np.uint32))
    w.add_array(group, "stop", (start + 1).astype(np.uint32))
    w.add_array(group, "ref", np.asarray(ref).astype(np.uint8).view("S1"))
    w.add_array(group, "alt", np.asarray(alt).astype(np.uint8).view("S1"))
    w.add_array(group, "chrom_run_first", np.array([r[0] for r in runs], np.uint32))
    w.add_array(group, "chrom_run_name", _h5_strings([r[1] for r in runs]) if runs else np.zeros(0, "S1"))


class H5CohortWriter:
    """StoreWriter's interface (begin_group / add_chunks / add_variants / add_chrom_runs / end_group / close, .meta) writing
    straight into OUT/{cohort}.h5: the chunk bytes of a group are appended to the file as the engine hands them over, its
    chunk index and tables follow at end_group — the file export_h5 makes from a store, without the store and without the
    second copy of every chunk (round 4: the converter's 3 M x 2504 run was 1.1 s of engine + store and 1.1 s of export).
    Used by the converter when one GPU does the work and neither the store nor the per-donor datasets are asked for."""

    def __init__(self, h5_path, samples, sc, vc, typesize=2, cohort_name="", donor_ids=None):
        from .h5file import H5Writer
        self.path = h5_path
        self.meta = dict(format="hhgt-store", version=1, cohort_name=cohort_name, samples=list(samples),
                         donor_ids=list(donor_ids) if donor_ids is not None else list(samples),
                         sc=int(sc), vc=int(vc), typesize=int(typesize), blocksize=min(int(vc) * 2, 8192),
                         chunk_format="blosc1", codec="blosc1: byte-shuffle + LZ4 block format", groups={})
        self.w = H5Writer(h5_path)
        self._cur = None
        self._named = False
        self._q = self._thread = self._err = None     # the writer thread of add_chunks(..., release=...)

    def _names(self):
        # /samples and /donor_ids first, as export_h5 writes them (the sample names arrive with the first header, before the
        # first group begins): the file comes out byte-identical to the one exported from a store
        if not self._named:
            self.w.add_array("/", "samples", _h5_strings(self.meta["samples"]))
            self.w.add_array("/", "donor_ids", _h5_strings(self.meta["donor_ids"]))
            self._named = True

    def begin_group(self, group):
        self._names()
        self._cur = dict(name=group, base=None, offsets=[0], start=[], ref=[], alt=[], runs=[], n_variants=0, raw_bytes=0)

    def add_chunks(self, data, offsets, raw_bytes, release=None):
        """release (optional): `data` stays valid until release() is called — the bytes are then written by the writer thread
        while the caller goes on (pipeline.stream_files(hold_columns=True)); without it they are written before this returns"""
        c = self._cur
        if release is None:
            addr = self.w.append(data, align=8 if c["base"] is None else 1)
        else:
            self._raise_pending()
            addr = self.w.reserve(len(data), align=8 if c["base"] is None else 1)
            if self._q is None:
                import queue
                import threading
                self._q = queue.Queue()
                self._thread = threading.Thread(target=self._write_loop, name="h5-cohort-writer", daemon=True)
                self._thread.start()
            self._q.put((addr, data, release))
        if c["base"] is None:
            c["base"] = addr
        elif addr != c["base"] + c["offsets"][-1]:
            raise RuntimeError("H5CohortWriter: the chunks of a group must follow each other in the file")
        base = c["offsets"][-1]
        c["offsets"].extend(int(base + o) for o in offsets[1:])
        c["raw_bytes"] += int(raw_bytes)

    def _write_loop(self):
        while True:
            item = self._q.get()
            try:
                if item is None:
                    return
                addr, data, release = item
                try:
                    if self._err is None:
                        self.w.write_at(addr, data)
                except BaseException as e:      # (kept for the caller's thread: _raise_pending)
                    self._err = e
                finally:
                    release()
            finally:
                self._q.task_done()

    def _drain(self):
        if self._q is not None:
            self._q.join()
        self._raise_pending()

    def _raise_pending(self):
        if self._err is not None:
            e, self._err = self._err, None
            raise e

    add_variants = StoreWriter.add_variants
    add_chrom_runs = StoreWriter.add_chrom_runs

    def end_group(self):
        c = self._cur
        S, sc, vc = len(self.meta["samples"]), self.meta["sc"], self.meta["vc"]
        # (the group's index and tables go behind its chunks in the file: reserve() has fixed the chunks' places, the writer
        # thread may still be filling them — nothing below reads them)
        g = dict(n_variants=c["n_variants"], n_vcol=-(-c["n_variants"] // vc), n_scol=-(-max(S, 1) // sc),
                 n_chunks=len(c["offsets"]) - 1, compressed_bytes=c["offsets"][-1], raw_bytes=c["raw_bytes"])
        self.meta["groups"][c["name"]] = g
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
        _h5_group_datasets(self.w, c["name"], self.meta, g, c["base"] if c["base"] is not None else self.w.pos, c["offsets"],
                           cat(c["start"], np.uint32), cat(c["ref"], np.uint8), cat(c["alt"], np.uint8), c["runs"])
        self._cur = None

    def close(self):
        if self.w is not None:
            try:
                self._drain()
            finally:
                if self._q is not None:
                    self._q.put(None)
                    self._thread.join()
                    self._q = self._thread = None
            self._names()
            self.w.close()
            self.w = None


def export_h5(store_path, h5_path, donor_records=False, ctx=None):
    """store directory -> one HDF5 file at the reference's output path (`OUT/{cohort}.h5`,
    /root/reference/src/haplohyped/vcf_to_h5.py:161), written natively (h5file.py; no h5py in this image):

        /samples, /donor_ids                         fixed-length strings
        /chr_{N}/genotype   int8 [S, V', 2]          chunks (sc, vc, 2), filter 32001 (Blosc): the stored chunk bytes
                                                     ARE the store's chunks, copied once in bulk
        /chr_{N}/start, stop   uint32 [V']           0-based start, stop = start + 1 (vcfpp.h:1118-1127, SNPs)
        /chr_{N}/ref, alt      S1 [V']
        /chr_{N}/chrom_run_first, chrom_run_name     CHROM value runs (first variant index, name)

    The reference's layout (S x 22 groups `donor_{id}/chr_{N}` of 35-byte compound records) is what
    GenotypeStore.snp_records / VCFH5Reader synthesise on demand; here every genotype is stored once.
    Needs Blosc-1 framed chunks (filter 32001 is hdf5-blosc / hdf5plugin.Blosc): stores written with
    chunk_format="blosc1", which is what the converter does.

    donor_records=True adds the reference's literal layout for every donor of the sample list:
        /donor_{id}/chr_{N}/snp_data   (also linked as .../genotype, the name h5_reader.py:38-40 opens) compound (35 B packed: chrom S5, start u4, stop u4, ref S10, alt S10, phase1 i1,
                                       phase2 i1 — vcf_to_h5.py:119-135), chunks of 7488 records, filter 32001 with
                                       typesize 35 (shuffle + LZ4 on the device, like every other chunk)
    That is S x 22 datasets repeating the variant table per donor (263 GB raw for 2504 donors x 3 M variants), so the
    converter only asks for it for small cohorts."""
    from .h5file import FILTER_BLOSC, H5Writer, blosc_cd_values
    meta = json.load(open(os.path.join(store_path, "meta.json")))
    if meta.get("chunk_format", "blosc2") != "blosc1":
        raise ValueError("export_h5: filter 32001 stores Blosc-1 chunks; this store holds " + meta.get("chunk_format", "blosc2"))
    sc, vc, S = meta["sc"], meta["vc"], len(meta["samples"])

    strings = _h5_strings
    with H5Writer(h5_path) as w:
        w.add_array("/", "samples", strings(meta["samples"]))
        w.add_array("/", "donor_ids", strings(meta["donor_ids"]))
        for group, g in meta["groups"].items():
            d = os.path.join(store_path, group)
            off = np.load(os.path.join(d, "offsets.npy")).astype(np.uint64)
            start = np.load(os.path.join(d, "start.npy"))
            base = w.append_file(os.path.join(d, "chunks.bin"))       # one bulk copy of all chunk bytes
            _h5_group_datasets(w, group, meta, g, base, off, start, np.load(os.path.join(d, "ref.npy")), np.load(os.path.join(d, "alt.npy")),
                               json.load(open(os.path.join(d, "chrom_runs.json"))))
        if donor_records:
            import torch
            from .device import BLOSC1
            st = GenotypeStore(store_path, ctx=ctx)
            c = st._context()
            chunk_nbytes = DONOR_CHUNK_ROWS * SNP_DTYPE.itemsize
            for donor in meta["donor_ids"]:
                if donor not in st.samples:
                    continue
                for group in meta["groups"]:
                    rec = st.snp_records(group, donor)
                    n_chunks = -(-max(len(rec), 1) // DONOR_CHUNK_ROWS)
                    padded = np.zeros(n_chunks * DONOR_CHUNK_ROWS, dtype=SNP_DTYPE)
                    padded[:len(rec)] = rec
                    src = torch.from_numpy(padded.view(np.uint8).reshape(-1)).to(c.device)
                    dst, off, total = c.compress(src, chunk_nbytes, typesize=SNP_DTYPE.itemsize, blocksize=32760, fmt=BLOSC1)
                    off = off.cpu().numpy()
                    base = w.append(dst[:total].cpu().numpy().tobytes(), align=1)
                    chunks = [((i * DONOR_CHUNK_ROWS,), base + int(off[i]), int(off[i + 1] - off[i])) for i in range(n_chunks)]
                    w.add_chunked(f"donor_{donor}/{group}", "snp_data", (len(rec),), SNP_DTYPE, (DONOR_CHUNK_ROWS,), chunks,
                                  filter_id=FILTER_BLOSC, cd_values=blosc_cd_values(SNP_DTYPE.itemsize, chunk_nbytes),
                                  filter_name=b"blosc", aliases=("genotype",))   # the name the reference's reader opens (h5_reader.py:38-40)
    return h5_path
