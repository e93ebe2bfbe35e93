"""The host-side planning of GenotypeStore's queries, numpy only (no device, no torch unless a torch mask is packed): what
a query's arguments mean (query_args), and which chunks, Blosc blocks, rows and variant ranges a query touches and where
their results go (plan_windows for reads, plan_rows and its three public faces for the row kernels, plan_gather on top of
it for the feature matrix, the plane layout)."""
import numpy as np

# one selection of the window planner: request q, chunk (vcol, scol), Blosc block, decoded bytes [lo, hi) of the block,
# and where they go in the output
PLAN_DTYPE = np.dtype([("req", np.int64), ("vcol", np.int64), ("scol", np.int64), ("block", np.uint32),
                       ("lo", np.uint32), ("hi", np.uint32), ("dst_off", np.uint64)])

# default budgets of GenotypeStore.pair_counts: the plane buffer of one window of variants, and the largest table it makes
DEFAULT_PLANE_BYTES = 1 << 30
MAX_PAIR_TABLE_BYTES = 2 << 30
# the largest matrix GenotypeStore.feature_matrix makes by default
MAX_FEATURE_BYTES = 4 << 30

# the smallest tile of GenotypeStore.ld_prune, in counted variants
LD_MIN_TILE = 64


def sample_index(index, n_samples, sample):
    """a sample's name (looked up in index: name -> position) or position -> its position, checked"""
    s = index[sample] if isinstance(sample, str) else int(sample)
    if not 0 <= s < n_samples:
        raise IndexError(f"sample {sample} out of range (0..{n_samples - 1})")
    return s


def query_args(meta, index, who, groups, samples=None, v_lo=0, v_hi=None, variant_mask=None, single=False):
    """what every query of GenotypeStore does with its arguments first, `who` naming it in the messages -> (idx, queries):
    idx, the sample indices (int64 array; samples: names or positions, None = every sample of meta, in order), and per
    group of `groups` (one name, a list, None = every group of meta; single: `groups` is the one group and variant_mask
    its mask, whatever their types) a tuple (group, lo, hi, n_var, mask): its variant range — [v_lo, v_hi) with one group,
    v_hi = None for its end; the whole group with several —, its number of variants and its variant mask as given
    (variant_mask: an array or tensor [hi - lo] with one group, or a dict group -> mask) or None.  KeyError for an unknown group, in `groups` or in the dict; ValueError for v_lo / v_hi or
    one mask with several groups and for a mask of another shape than its range; IndexError for a range outside the
    group and for a sample position outside the store (an unknown name: KeyError)."""
    if single:
        names = [groups]
    else:
        names = list(meta["groups"]) if groups is None else [groups] if isinstance(groups, str) else list(groups)
    for g in names:
        if g not in meta["groups"]:
            raise KeyError(g)
    if len(names) != 1 and (int(v_lo) != 0 or v_hi is not None):
        raise ValueError(f"{who}: v_lo / v_hi need a single group")
    if isinstance(variant_mask, dict) and not single:
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
    queries = []
    for group in names:
        n_var = meta["groups"][group]["n_variants"]
        lo, hi = (int(v_lo), n_var if v_hi is None else int(v_hi)) if len(names) == 1 else (0, n_var)
        if not 0 <= lo <= hi <= n_var:
            raise IndexError(f"variants [{lo}, {hi}) outside {group} (0..{n_var})")
        queries.append((group, lo, hi, n_var, masks.get(group)))
    n = len(meta["samples"])
    idx = (np.arange(n) if samples is None else
           np.array([sample_index(index, n, x) for x in samples], dtype=np.int64).reshape(-1))
    for group, lo, hi, _, m in queries:
        if m is not None and (m.ndim != 1 or int(m.shape[0]) != hi - lo):
            raise ValueError(f"variant_mask of {group}: shape {tuple(m.shape)}, expected ({hi - lo},)")
    return idx, queries


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


# one selection of the row planner: chunk (vcol, scol), Blosc block `part` of its rows, the rows selected (bit r = row r),
# variants [lo, hi) of that block, and where the block's results go: out_row (plan_counts: the output row of variant lo;
# plan_sample_counts, plan_planes: the output row of chunk row 0), mask_word (the first word of the block's bits in the
# group's packed variant mask), out_word (the first word of the block's bits in a plane row)
ROW_PLAN_DTYPE = np.dtype([("vcol", np.int64), ("scol", np.int64), ("part", np.uint32), ("row_mask", np.uint64),
                           ("lo", np.uint32), ("hi", np.uint32), ("out_row", np.int64), ("mask_word", np.int64),
                           ("out_word", np.int64)])
COUNT_PLAN_DTYPE = SAMPLE_PLAN_DTYPE = PLANE_PLAN_DTYPE = ROW_PLAN_DTYPE


def default_blocksize(vc):
    """the Blosc block size the writers give chunks of vc variants per row: a row, 8 KiB at the most"""
    return min(int(vc) * 2, 8192)


def mask_words_per_block(blocksize):
    """uint32 words a Blosc block of blocksize / 2 variants owns in a packed variant mask: its bits start at a word"""
    return -(-(int(blocksize) // 2) // 32)


def plan_rows(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize=None, out_row="variant", block0=None):
    """the selections of a row kernel over the samples `sample_idx` (indices; each selected once, however often it is
    named) and the variants [v_lo, v_hi) of a group of n_samples x n_variants stored in chunks of sc x vc: per chunk row,
    the selected rows as a 64-bit mask; the variant range cut at chunk columns and at Blosc blocks (a row of vc variants
    is vc * 2 / blocksize blocks of blocksize / 2 variants: its two halves with 8 KiB blocks and vc = 8192; blocksize
    None: default_blocksize(vc)).  Padded rows (samples >= n_samples) and padded variants (>= n_variants) are never selected.
    Chunk columns come in order, within one the chunk rows, within a chunk its blocks, so the selections of a chunk are
    adjacent.  An empty sample list or range gives no selection.  With block B = v // (blocksize / 2) of the group:
    mask_word = B * mask_words_per_block(blocksize), out_word = (B - block0) * mask_words_per_block(blocksize) (block0:
    the first block of a plane buffer; default: the block of v_lo), and out_row by what the rows of the output are —
    "variant": the variants of the range, out_row = that of the selection's first; "sample": the samples, chunk row r of
    chunk row `scol` at scol * sc + r; "plane": the plane rows of plane_rows, compacted by chunk row."""
    sc, vc, n_samples, n_variants = int(sc), int(vc), int(n_samples), int(n_variants)
    v_lo, v_hi = int(v_lo), int(v_hi)
    bs = default_blocksize(vc) if blocksize is None else int(blocksize)
    if not 1 <= sc <= 64 or bs % 2 or (vc * 2) % bs:
        raise ValueError(f"plan_counts: chunks of {sc} x {vc} in blocks of {bs} bytes (1..64 rows, whole blocks per row)")
    if not 0 <= v_lo <= v_hi <= n_variants:
        raise IndexError("variants [{}, {}) outside 0..{}".format(v_lo, v_hi, n_variants))     # (of a plan; a query's: query_args)
    s = np.unique(np.asarray(sample_idx, dtype=np.int64).reshape(-1))
    if s.size and (s[0] < 0 or s[-1] >= n_samples):
        raise IndexError(f"sample index outside 0..{n_samples - 1}")
    if s.size == 0 or v_hi == v_lo:
        return np.zeros(0, ROW_PLAN_DTYPE)
    masks = np.zeros(-(-n_samples // sc), np.uint64)
    np.bitwise_or.at(masks, s // sc, np.left_shift(np.uint64(1), (s % sc).astype(np.uint64)))
    scols = np.nonzero(masks)[0]
    vb, wpb = bs // 2, mask_words_per_block(bs)
    block0 = v_lo // vb if block0 is None else int(block0)
    if block0 > v_lo // vb:
        raise IndexError(f"plan_planes: block0 {block0} lies behind variant {v_lo}")
    seg = np.arange(v_lo // vb, (v_hi - 1) // vb + 1, dtype=np.int64)        # blocks of vb variants touched, in order
    a, b = np.maximum(v_lo, seg * vb), np.minimum(v_hi, (seg + 1) * vb)
    out = np.zeros(seg.size * scols.size, ROW_PLAN_DTYPE)
    rep = lambda x: np.repeat(x, scols.size)
    out["vcol"] = rep(seg * vb // vc)
    out["part"] = rep((seg * vb % vc) // vb)
    out["lo"] = rep(a - seg * vb)
    out["hi"] = rep(b - seg * vb)
    out["scol"] = np.tile(scols, seg.size)
    out["row_mask"] = np.tile(masks[scols], seg.size)
    out["mask_word"] = rep(seg * wpb)
    out["out_word"] = rep((seg - block0) * wpb)
    out["out_row"] = {"variant": lambda: rep(a - v_lo), "sample": lambda: out["scol"] * sc,
                      "plane": lambda: np.tile(np.arange(scols.size) * sc, seg.size)}[out_row]()
    return out[np.lexsort((out["part"], out["scol"], out["vcol"]))]


def plan_counts(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize=None):
    """the selections of an allele count (hhgt_count_alleles): plan_rows' cut of (samples, [v_lo, v_hi)), out_row the
    output row of the selection's first variant, v_lo at row 0"""
    return plan_rows(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize, "variant")


def plan_sample_counts(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize=None):
    """the selections of a per-sample count (hhgt_count_samples): plan_counts' cuts of (samples, [v_lo, v_hi)) — the same
    chunks, blocks, row masks and ranges, in the same order —, where chunk row r of chunk row `scol` is counted into
    output row scol * sc + r (the sample's index), and the block's mask bits begin at word (vcol * blocks per row + part) *
    mask_words_per_block(blocksize) of the group's packed variant mask (pack_variant_mask)."""
    return plan_rows(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize, "sample")


def plan_planes(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize=None, block0=None):
    """the selections of hhgt_genotype_planes: plan_counts' cuts of (samples, [v_lo, v_hi)) — the same chunks, blocks, row
    masks and ranges, in the same order, mask_word as plan_sample_counts gives it —, with the plane rows compacted by chunk
    row (plane_rows: the k-th chunk row that has a selected sample owns plane rows [k * sc, (k + 1) * sc)) and the bits of
    block B of the group (B = v // (blocksize / 2)) at word (B - block0) * mask_words_per_block(blocksize) of a plane row;
    block0: the first block of the plane buffer (default: the block of v_lo)."""
    return plan_rows(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize, "plane", block0)


# one selection of plan_gather: the row planner's fields, and the output column of the block's first gathered variant
GATHER_PLAN_DTYPE = np.dtype(ROW_PLAN_DTYPE.descr + [("out_col", np.int64)])


def plan_gather(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, block_counts, blocksize=None, col0=0):
    """the selections of hhgt_gather_calls: plan_sample_counts' cuts of (samples, [v_lo, v_hi)) — the same chunks, blocks,
    row masks, ranges and mask_word, in the same order; out_row = scol * sc, the entry of chunk row 0 in a row map of
    ceil(n_samples / sc) * sc entries — with the output columns of every block: block_counts[k] is the number of
    gathered variants in the k-th Blosc block (of blocksize / 2 variants) the range touches, and the block's first gathered
    variant owns column out_col = col0 + the sum of the counts of the blocks before it.  A block that gathers nothing gives
    no selection.  ValueError if block_counts is not one count per touched block, or a count exceeds its block's part of
    the range."""
    plan = plan_rows(sample_idx, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize, "sample")
    v_lo, v_hi = int(v_lo), int(v_hi)
    vb = (default_blocksize(vc) if blocksize is None else int(blocksize)) // 2
    counts = np.asarray(block_counts, dtype=np.int64).reshape(-1)
    seg = np.arange(v_lo // vb, (v_hi - 1) // vb + 1, dtype=np.int64) if v_hi > v_lo else np.zeros(0, np.int64)
    room = np.minimum(v_hi, (seg + 1) * vb) - np.maximum(v_lo, seg * vb)
    if counts.size != seg.size or (counts < 0).any() or (counts > room).any():
        raise ValueError(f"plan_gather: {counts.size} block counts for the {seg.size} blocks of [{v_lo}, {v_hi}), each at most its block's variants")
    first = int(col0) + np.cumsum(counts) - counts
    out = np.zeros(len(plan), GATHER_PLAN_DTYPE)
    for f in ROW_PLAN_DTYPE.names:
        out[f] = plan[f]
    k = plan["vcol"] * (int(vc) // vb) + plan["part"].astype(np.int64) - (v_lo // vb)        # the selection's touched block
    out["out_col"] = first[k] if len(plan) else 0
    return out[counts[k] > 0] if len(plan) else out


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


def plane_rows(sample_idx, sc):
    """the plane rows of a sample list: chunk rows without a listed sample get none, the others sc rows each in order ->
    (scols: the chunk rows kept, ascending; rows int64 [len(sample_idx)]: the plane row of each listed sample)"""
    s = np.asarray(sample_idx, dtype=np.int64).reshape(-1)
    scols = np.unique(s // int(sc))
    return scols, np.searchsorted(scols, s // int(sc)) * int(sc) + s % int(sc)


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


# hhgt_region_sums' geometry and tables (HHGT_REGION_SPAN, HHGT_REGION_MAX_COLS, HHGT_PIECE_*, HHGT_RUN_* of include/hhgt.h):
# the plane words a piece has at most, the columns of weights a call takes at most, the fields of a piece and of a run
REGION_SPAN = 64
REGION_MAX_COLS = 16
PIECE_LO, PIECE_HI, PIECE_OUT, PIECE_SLOT, PIECE_FIELDS = 0, 1, 2, 3, 4
PIECE_DIRECT = -1
RUN_OUT, RUN_SLOT, RUN_PIECES, RUN_FIELDS = 0, 1, 2, 3


def plan_regions(regions, a, b, blocksize, block0=None):
    """the tables of hhgt_region_sums for `regions`, int64 [R, 2] variant intervals [lo, hi) of one group, over the plane
    window of the variants [a, b), whose rows begin at Blosc block block0 (default: the block of a) -> (pieces int64
    [n, PIECE_FIELDS], runs int64 [m, RUN_FIELDS], n_slots).  The regions may come in any order, overlap, repeat each other
    or be empty; region r adds to output r.  Each is clipped to the window and mapped through plane_positions: its pieces
    cover the bit positions from its first variant's to its last one's — the padding of the blocks in between included,
    which has no bit and no weight — and it is cut every REGION_SPAN words counted from the word of its OWN first position,
    so a region's pieces, and with them its sums to the bit, do not depend on which other regions the call carries (they do
    depend on the window, where the window clips).  A region without a variant in the window gives no piece.  Pieces come
    in the order of the regions, a region's in ascending order of position; a region of one piece is PIECE_DIRECT, one of
    several holds consecutive slots from the running total and gets a run."""
    a, b, vb = int(a), int(b), int(blocksize) // 2
    block0 = a // vb if block0 is None else int(block0)
    regions = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    if b < a or block0 * vb > a:
        raise IndexError(f"plan_regions: a window [{a}, {b}) in rows that begin at block {block0}")
    lo, hi = np.maximum(regions[:, 0], a), np.minimum(regions[:, 1], b)
    out = np.nonzero(lo < hi)[0]
    lo, last = lo[out], hi[out] - 1
    bits = 32 * mask_words_per_block(blocksize)
    p_lo = (lo // vb - block0) * bits + lo % vb
    p_hi = (last // vb - block0) * bits + last % vb + 1
    w0 = p_lo // 32
    n = -(-(-(-p_hi // 32) - w0) // REGION_SPAN)            # pieces of every region: at least 1
    first = np.cumsum(n) - n
    k = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(first, n)       # a piece's number in its region
    rep = lambda x: np.repeat(x, n)
    pieces = np.zeros((k.size, PIECE_FIELDS), np.int64)
    pieces[:, PIECE_LO] = np.maximum(rep(p_lo), 32 * (rep(w0) + k * REGION_SPAN))
    pieces[:, PIECE_HI] = np.minimum(rep(p_hi), 32 * (rep(w0) + (k + 1) * REGION_SPAN))
    pieces[:, PIECE_OUT] = rep(out)
    long = n > 1
    slots = np.where(long, n, 0)
    slot0 = np.cumsum(slots) - slots
    pieces[:, PIECE_SLOT] = np.where(rep(long), rep(slot0) + k, PIECE_DIRECT)
    runs = np.stack([out[long], slot0[long], n[long]], axis=1).astype(np.int64).reshape(-1, RUN_FIELDS)
    return pieces, runs, int(slots.sum())
