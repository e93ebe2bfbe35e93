"""-m gpu: selected variants as dense columns.  hhgt_gather_calls (one workgroup per (chunk, Blosc block column): the masked
variants of every selected row compacted in LDS and stored as elements of a class table, or as the calls themselves) bit
for bit against numpy on the raw bytes — every geometry and header format, mask densities and hand-made masks at the
kernel's internal boundaries, every chunk kind, every element size and raw mode, odd columns, wide rows, an output off its
16-byte boundary, a row map, untouched elements, bad selections, refused arguments; GenotypeStore.feature_matrix,
VCFH5Reader.feature_matrix and the features CLI on converter output against the contract restated from read_windows."""
import ctypes as C

import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd import device as dev, synth
from haplohyped_varawareml_amd._lib import HhgtError, check
from haplohyped_varawareml_amd.device import GATHER_SEL_DTYPE
from haplohyped_varawareml_amd.store import (GenotypeStore, call_class_values, cast_class_values, mask_words_per_block,
                                             pack_variant_mask)
from tests.test_gpu_allele_counts import CHROM3, GEOMS, S3, V3, cohort, kernel_chunks  # noqa: F401 (cohort: fixture)
from tests.test_gpu_sample_counts import block_mask, two_groups  # noqa: F401 (two_groups: fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
TORCH_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def np_classes(g):
    """int8 [..., 2] -> the class of every call: 0 HOM_REF, 1 HET, 2 HOM_ALT, 3 not complete (the contract, restated)"""
    a, b = g[..., 0].astype(np.int64), g[..., 1].astype(np.int64)
    complete = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
    return np.where(complete, a + b, 3)


def random_table(rng, n_cols, eb):
    """[4, n_cols] of random bit patterns (for 2, 4, 8 bytes: float NaNs with payloads among them), as unsigned integers"""
    t = rng.integers(0, 256, (4, n_cols, eb), dtype=np.uint8).view(UINT[eb]).reshape(4, n_cols)
    if eb > 1:
        nan = {2: 0x7E01, 4: 0x7FC00123, 8: 0x7FF8000000000ABC}[eb]
        t[rng.random(t.shape) < 0.1] = nan
    return t


def output_buffer(ctx, n_rows, row_stride, eb, raw):
    """a sentinel-filled output one element past a 16-byte boundary -> (the tensor gather_calls takes, its uint8 backing)"""
    flat = torch.full((n_rows * row_stride * eb + 64,), SENTINEL, dtype=torch.uint8, device=ctx.device)
    assert flat.data_ptr() % 16 == 0
    body = flat[eb:eb + n_rows * row_stride * eb]
    out = body.view(torch.int8).view(n_rows, row_stride, 2) if raw else body.view(TORCH_INT[eb]).view(n_rows, row_stride)
    assert out.data_ptr() % 16 == eb
    return out, flat


def as_uint(out, flat, eb):
    """the output's elements and the bytes around them, as numpy: (uint [n_rows, row_stride], uint8 before, uint8 after)"""
    n = out.shape[0] * out.shape[1] * eb
    f = flat.cpu().numpy()
    return f[eb:eb + n].view(UINT[eb]).reshape(out.shape[0], out.shape[1]), f[:eb], f[eb + n:]


def gather_sel(rng, d, off, sc, vc, bs, n, n_map, words, vmask, col0=1, hand=None):
    """n selections over random chunks, blocks, row masks and ranges, each owning the columns behind the previous one's
    (so no two own an element, whatever their rows) -> (sel, the column behind the last)"""
    parts, vb, wpb = vc * 2 // bs, bs // 2, mask_words_per_block(bs)
    sel, col = np.zeros(n, GATHER_SEL_DTYPE), col0
    for j in range(n):
        i, p = int(rng.integers(len(off) - 1)), int(rng.integers(parts))
        mask = int(rng.integers(0, 1 << 63)) | (int(rng.integers(0, 2)) << 63)
        if j % 5 == 0:
            mask = (1 << sc) - 1
        if j % 7 == 3:
            mask = 1 << int(rng.integers(sc))
        mask &= (1 << sc) - 1
        lo, hi = (0, vb) if j % 3 == 0 else sorted(int(x) for x in rng.choice(vb + 1, 2, replace=False))
        word = int(rng.integers(0, words - wpb + 1)) if hand is None else hand[j] * wpb
        sel[j] = (d.data_ptr() + int(off[i]), int(off[i + 1] - off[i]), mask, int(rng.integers(0, n_map - sc + 1)), word, col,
                  p, lo, hi, 0)
        keep = np.zeros(vb, bool)
        keep[lo:hi] = True
        if vmask is not None:
            keep &= block_mask(vmask, word, vb)
        col += int(keep.sum())
    return sel, col


def expected(raw, ptrs, sel, sc, bs, want, vmask, row_map, table):
    """writes what the selections own into `want` (uint [n_rows, row_stride]; table None: raw mode, the allele pair as
    one little-endian uint16) -> the owned elements as a bool array"""
    vb = bs // 2
    owned = np.zeros(want.shape, bool)
    for s in sel:
        i = int(np.searchsorted(ptrs, int(s["src_ptr"])))
        keep = np.zeros(vb, bool)
        keep[int(s["lo"]):int(s["hi"])] = True
        if vmask is not None:
            keep &= block_mask(vmask, int(s["mask_word"]), vb)
        v0, c0, n = int(s["part"]) * vb, int(s["out_col"]), int(keep.sum())
        for r in range(sc):
            if not int(s["row_mask"]) >> r & 1 or n == 0:
                continue
            R = int(s["out_row"]) + r if row_map is None else int(row_map[int(s["out_row"]) + r])
            g = raw[i][r, v0:v0 + vb][keep]
            if table is None:
                want[R, c0:c0 + n] = np.ascontiguousarray(g).view("<u2").reshape(-1)
            else:
                want[R, c0:c0 + n] = table[np_classes(g), c0 + np.arange(n)]
            assert not owned[R, c0:c0 + n].any()
            owned[R, c0:c0 + n] = True
    return owned


def run_and_compare(ctx, raw, d, off, sel, n_cols, sc, vc, bs, eb, vmask, row_map, n_rows, table, halves=False):
    is_raw = table is None
    out, flat = output_buffer(ctx, n_rows, n_cols + 3, eb, is_raw)
    want = np.full((n_rows, n_cols + 3), int.from_bytes(bytes([SENTINEL]) * eb, "little"), UINT[eb])
    owned = expected(raw, d.data_ptr() + off[:-1], sel, sc, bs, want, vmask, row_map, table)
    values = None if is_raw else torch.from_numpy(table.view({1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[eb])).to(ctx.device)
    kw = dict(values=values, out=out, n_cols=n_cols, row_map=row_map, vmask=vmask, blocksize=bs)
    if halves:           # two calls on one stream fill disjoint columns of one matrix
        _, bad0 = ctx.gather_calls(sel[:len(sel) // 2], sc, vc, **kw)
        got, bad = ctx.gather_calls(sel[len(sel) // 2:], sc, vc, **kw)
        bad += bad0
    else:
        got, bad = ctx.gather_calls(sel, sc, vc, **kw)
    assert bad == 0 and got is out
    have, before, after = as_uint(out, flat, eb)
    assert (before == SENTINEL).all() and (after == SENTINEL).all()
    assert np.array_equal(have, want)                       # owned elements exact, every other element still the sentinel
    return owned


@pytest.mark.parametrize("fmt", [dev.BLOSC1, dev.BLOSC2])
@pytest.mark.parametrize("sc,vc,bs", GEOMS)
def test_kernel_matches_numpy(ctx, fmt, sc, vc, bs):
    rng = np.random.default_rng(sc * 7 + vc + bs + fmt)
    raw, d, off = kernel_chunks(ctx, rng, sc, vc, bs, fmt)
    g = raw[[0, 1, 2, 4]]
    assert all((g == x).any() for x in (0, 1, -9, 2, 3)) and ((g[..., 0] == -9) != (g[..., 1] == -9)).any()
    n_rows, words = 2 * sc + 5, 12 * mask_words_per_block(bs)
    k = 0
    for density in (None, 0.0, 0.03, 0.3, 1.0):
        vmask = None if density is None else np.packbits(rng.random(words * 32) < density, bitorder="little").view("<u4")
        for eb, is_raw in ((1, False), (2, False), (4, False), (8, False), (2, True)):
            row_map = rng.permutation(n_rows).astype(np.uint32) if k % 2 == 0 else None
            sel, end = gather_sel(rng, d, off, sc, vc, bs, 10, n_rows, words, vmask)
            table = None if is_raw else random_table(rng, end + 2, eb)
            owned = run_and_compare(ctx, raw, d, off, sel, end + 2, sc, vc, bs, eb, vmask, row_map, n_rows, table, halves=k % 3 == 0)
            assert owned.any() == (density != 0.0)
            k += 1
    # every chunk kind, whole rows: the memcpyed chunk (3) and the unshuffled one (4) included; the mask as a device tensor
    parts, vb, wpb = vc * 2 // bs, bs // 2, mask_words_per_block(bs)
    keep = rng.random(vc) < 0.3
    packed = pack_variant_mask(torch.from_numpy(keep).to(ctx.device), 0, vc, vc, bs)
    block_n = [int(keep[p * vb:(p + 1) * vb].sum()) for p in range(parts)]
    table = random_table(rng, int(keep.sum()), 4)
    values = torch.from_numpy(table.view(np.int32)).to(ctx.device)
    for i in range(5):
        s = np.zeros(parts, GATHER_SEL_DTYPE)
        for p in range(parts):
            s[p] = (d.data_ptr() + int(off[i]), int(off[i + 1] - off[i]), (1 << sc) - 1, 0, p * wpb, sum(block_n[:p]), p, 0, vb, 0)
        out, bad = ctx.gather_calls(s, sc, vc, values=values, blocksize=bs, vmask=packed)        # (the default output)
        assert bad == 0 and tuple(out.shape) == (sc, int(keep.sum())) and out.dtype == torch.int32
        want = table[np_classes(raw[i][:, keep]), np.arange(int(keep.sum()))[None, :]]
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want), i
        pairs, bad = ctx.gather_calls(s, sc, vc, n_cols=int(keep.sum()), blocksize=bs, vmask=packed)
        assert bad == 0 and pairs.dtype == torch.int8 and np.array_equal(pairs.cpu().numpy(), raw[i][:, keep]), i


@pytest.mark.parametrize("sc,vc,bs", GEOMS)
def test_hand_made_masks_at_the_kernels_boundaries(ctx, sc, vc, bs):
    """only variant 0, only the last one, and only the pair on either side of each boundary inside the kernel: the thread's 16
    variants, the 32-bit mask word, the wave (1024 variants), the two passes (2048 variants at two waves)"""
    rng = np.random.default_rng(bs + 1)
    raw, d, off = kernel_chunks(ctx, rng, sc, vc, bs, dev.BLOSC2)
    vb, wpb = bs // 2, mask_words_per_block(bs)
    takes = [[0], [vb - 1]] + [[b - 1, b] for b in (16, 32, 1024, 2048) if b < vb]
    assert len(takes) == (6 if vb == 4096 else 3)
    bits = np.zeros((len(takes), wpb * 32), bool)
    for k, t in enumerate(takes):
        bits[k, t] = True
    vmask = np.packbits(bits.reshape(-1), bitorder="little").view("<u4")
    n_rows = sc + 3
    for eb, is_raw in ((1, False), (8, False), (2, True)):
        sel, end = gather_sel(rng, d, off, sc, vc, bs, len(takes), n_rows, 0, vmask, hand=list(range(len(takes))))
        sel["lo"], sel["hi"] = 0, vb
        sel["out_col"] = 1 + np.cumsum([0] + [len(t) for t in takes[:-1]])
        end = 1 + sum(len(t) for t in takes)
        table = None if is_raw else random_table(rng, end, eb)
        owned = run_and_compare(ctx, raw, d, off, sel, end, sc, vc, bs, eb, vmask, None, n_rows, table)
        assert owned.any()


def test_bad_selections_counted(ctx):
    sc, vc, bs = 40, 4096, 8192
    rng = np.random.default_rng(11)
    raw, d, off = kernel_chunks(ctx, rng, sc, vc, bs, dev.BLOSC1)
    n_rows, wpb, eb = 2 * sc, mask_words_per_block(bs), 2
    words = 3 * wpb
    vmask = np.packbits(rng.random(words * 32) < 0.5, bitorder="little").view("<u4")
    row_map = rng.permutation(n_rows).astype(np.uint32)
    row_map = np.append(row_map, [n_rows, 7]).astype(np.uint32)              # entry n_rows names a row past the output
    n_map = len(row_map)
    sel, end = gather_sel(rng, d, off, sc, vc, bs, 12, n_rows, words, vmask)
    n_cols = end + 40
    # chunk 0 again with the size word of its first stream zeroed: a corrupt stream
    size0 = int(off[1] - off[0])
    broken = d[:size0].cpu().numpy().copy()
    first = int(broken[16:20].view("<u4")[0])                                 # Blosc-1: block 0's streams start here
    broken[first:first + 4] = 0
    dbroken = torch.from_numpy(broken).to(ctx.device)
    p0 = d.data_ptr()
    in_mask = int(block_mask(vmask, 0, bs // 2)[:10].sum())
    assert 0 < in_mask < 10
    extra = np.zeros(12, GATHER_SEL_DTYPE)
    extra[0] = (p0, size0 - 100, 1, 0, 0, end, 0, 0, 10, 0)                   # truncated chunk: invalid header
    extra[1] = (p0, size0, 1, 0, 0, end, 1, 0, 10, 0)                         # part past the row's blocks
    extra[2] = (p0, size0, 1, 0, 0, end, 0, 5, 5, 0)                          # lo == hi
    extra[3] = (p0, size0, 1, 0, 0, end, 0, 0, bs // 2 + 1, 0)                # hi past the block
    extra[4] = (p0, size0, 1 << sc, 0, 0, end, 0, 0, 10, 0)                   # a row bit >= sc
    extra[5] = (p0, size0, 1 << 7, n_map - 7, 0, end, 0, 0, 10, 0)            # the highest selected row past the row map
    extra[6] = (p0, size0, 1, 0, words - wpb + 1, end, 0, 0, 10, 0)           # mask words past the mask
    extra[7] = (dbroken.data_ptr(), size0, 3, 0, 0, end, 0, 0, 10, 0)         # corrupt stream (row 0)
    extra[8] = (p0, size0, 1, 0, 0, end, 0, 7, 3, 0)                          # lo > hi
    extra[9] = (p0, size0, 5, n_rows - 2, 0, end, 0, 0, 10, 0)                # a selected row (entry n_rows) whose R >= n_rows
    extra[10] = (p0, size0, 1, 0, 0, n_cols - in_mask + 1, 0, 0, 10, 0)       # out_col + gathered > n_cols
    extra[11] = (p0, size0, 1, 0, 0, n_cols + 1, 0, 0, 10, 0)                 # out_col itself past n_cols
    both = np.concatenate([sel[:7], extra, sel[7:]])
    table = random_table(rng, n_cols, eb)
    values = torch.from_numpy(table.view(np.int16)).to(ctx.device)
    out, flat = output_buffer(ctx, n_rows, n_cols + 3, eb, False)
    want = np.full((n_rows, n_cols + 3), 0xA5A5, np.uint16)
    expected(raw, p0 + off[:-1], sel, sc, bs, want, vmask, row_map, table)
    _, bad = ctx.gather_calls(both, sc, vc, values=values, out=out, n_cols=n_cols, row_map=row_map, vmask=vmask, blocksize=bs)
    assert bad == len(extra)
    have = as_uint(out, flat, eb)[0]
    theirs = np.zeros(have.shape, bool)        # the corrupt selection's own elements may hold anything
    theirs[[int(row_map[0]), int(row_map[1])], end:end + in_mask] = True
    assert np.array_equal(have[~theirs], want[~theirs])          # the good ones exact, a bad selection writes nothing
    # each of those turned good again: the limits themselves are allowed
    extra[5]["out_row"], extra[9]["row_mask"], extra[10]["out_col"] = n_map - 8, 1, n_cols - in_mask
    extra[6]["mask_word"], extra[5]["out_col"] = words - wpb, end + 20              # (5 in columns of its own)
    out.fill_(0)
    _, bad = ctx.gather_calls(extra[[5, 6, 9, 10]], sc, vc, values=values, out=out, n_cols=n_cols, row_map=row_map,
                              vmask=vmask, blocksize=bs)
    assert bad == 0
    # without a map out_row + r is the row; without a mask the mask words are not looked at
    one = extra[6:7].copy()
    one["out_row"], one["mask_word"], one["row_mask"] = n_rows - 8, 1 << 40, 1 << 7
    got, bad = ctx.gather_calls(one, sc, vc, values=values, n_rows=n_rows, blocksize=bs)
    assert bad == 0 and np.array_equal(got[n_rows - 1, end:end + 10].cpu().numpy().view(np.uint16),
                                       table[np_classes(raw[0][7, :10]), end + np.arange(10)])
    one["out_row"] = n_rows - 7
    assert ctx.gather_calls(one, sc, vc, values=values, n_rows=n_rows, blocksize=bs)[1] == 1
    # a selection without rows, or whose mask takes nothing, is good and writes nothing
    none = extra[6:8].copy()
    none["src_ptr"], none["mask_word"], none["out_row"] = p0, 0, 0
    none[0]["row_mask"] = 0
    none[1]["lo"], none[1]["hi"] = 0, 10
    empty = np.zeros(words, np.uint32)
    out.fill_(3)
    assert ctx.gather_calls(none, sc, vc, values=values, out=out, n_cols=n_cols, vmask=empty, blocksize=bs)[1] == 0
    assert bool((out == 3).all())
    # a mask without words: every selection is past it
    assert ctx.gather_calls(sel, sc, vc, values=values, out=out, n_cols=n_cols, vmask=np.zeros(0, np.uint32), blocksize=bs)[1] == len(sel)


def test_refused_arguments(ctx):
    sel = np.zeros(1, GATHER_SEL_DTYPE)
    values = torch.zeros((4, 16), dtype=torch.int16, device=ctx.device)
    for kw in (dict(sc=64, vc=8192, typesize=3, blocksize=8190), dict(sc=64, vc=8192, typesize=2, blocksize=6000),
               dict(sc=65, vc=8192, typesize=2, blocksize=8192), dict(sc=64, vc=16384, typesize=2, blocksize=16384)):
        with pytest.raises(HhgtError) as e:
            ctx.gather_calls(sel, kw["sc"], kw["vc"], values=values, n_rows=64, typesize=kw["typesize"], blocksize=kw["blocksize"])
        assert e.value.code == -1 and "gather_calls" in str(e.value)
    # what the binding never passes goes through the C entry point itself (the arguments are checked whatever the number
    # of selections: none here, so nothing is launched)
    out = torch.zeros(64 * 20, dtype=torch.int16, device=ctx.device)

    def call(d_values, elem_bytes, d_out, n_cols=16, row_stride=20):
        bad = C.c_uint64(5)
        with torch.cuda.device(ctx.device):
            check(ctx.lib.hhgt_gather_calls(ctx.h, None, 0, 64, 8192, 2, 8192, None, 0, None, 0,
                                            C.c_void_p(d_values) if d_values else None, elem_bytes, C.c_void_p(d_out), 64,
                                            n_cols, row_stride, C.byref(bad), None))
        return int(bad.value)

    v, o = values.data_ptr(), out.data_ptr()
    for args, word in (((v, 3, o), "elem_bytes"), ((v, 16, o), "elem_bytes"), ((0, 4, o), "elem_bytes"), ((0, 1, o), "elem_bytes"),
                       ((v, 2, o, 16, 15), "row_stride"), ((v, 2, o + 1), "d_out"), ((v + 1, 2, o), "d_values"),
                       ((v, 8, o + 4), "d_out"), ((0, 2, o + 1), "d_out")):
        with pytest.raises(HhgtError) as e:
            call(*args)
        assert e.value.code == -1 and "gather_calls" in str(e.value) and word in str(e.value), args
    assert call(v, 2, o) == 0 and call(0, 2, o) == 0 and call(v, 2, o, 16, 16) == 0            # accepted
    # the binding's own checks
    for kw in (dict(values=values.to(torch.float32)[:, ::2]), dict(values=values, n_cols=8), dict(values=values.cpu()),
               dict(values=values, out=torch.zeros((64, 16), dtype=torch.int32, device=ctx.device)),
               dict(values=values, out=torch.zeros((64, 8), dtype=torch.int16, device=ctx.device)),
               dict(values=values, out=torch.zeros((64, 32), dtype=torch.int16, device=ctx.device)[:, ::2]),
               dict(out=torch.zeros((64, 16), dtype=torch.int8, device=ctx.device)),
               dict(values=values, row_map=torch.zeros(64, dtype=torch.int64, device=ctx.device))):
        with pytest.raises(ValueError):
            ctx.gather_calls(sel, 64, 8192, **kw)


# ---- the store ---------------------------------------------------------------------------------------------------------
def t_classes(g):
    """int8 device tensor [..., 2] -> int64 classes, np_classes in torch"""
    a, b = g[..., 0].to(torch.int64), g[..., 1].to(torch.int64)
    complete = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
    return torch.where(complete, a + b, torch.full_like(a, 3))


def bits_equal(x, y):
    """two tensors of one dtype and shape hold the same bytes"""
    view = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(view), y.contiguous().view(view))


def contract(st, group, idx, lo, hi, mask, coding, dtype, impute, freq):
    """feature_matrix restated: read_windows of each sample, the class, call_class_values, torch's cast -> (X, variants)"""
    dev_ = st._context().device
    G = torch.stack(st.read_windows([(group, int(s), lo, hi) for s in idx]))           # [n, hi - lo, 2]
    keep = torch.ones(hi - lo, dtype=torch.bool, device=dev_) if mask is None else st._device_bool(mask)
    if coding == "haplotypes":
        return G[:, keep], torch.nonzero(keep).reshape(-1) + lo
    values, used = call_class_values(st.allele_counts(group, freq, lo, hi), coding, impute)
    keep = keep & used
    table = cast_class_values(values[:, keep], dtype)
    cls = t_classes(G[:, keep])
    return table[cls, torch.arange(cls.shape[1], device=dev_)[None, :]], torch.nonzero(keep).reshape(-1) + lo


CODINGS = [("dosage", torch.int8, "missing"), ("dosage", torch.float16, "mean"), ("dosage", torch.bfloat16, "mean"),
           ("dosage", torch.float32, "mean"), ("dosage", torch.float64, "mean"), ("dosage", torch.float32, "missing"),
           ("standardized", torch.float16, "mean"), ("standardized", torch.bfloat16, "mean"),
           ("standardized", torch.float32, "mean"), ("standardized", torch.float64, "mean"),
           ("standardized", torch.float32, "missing"), ("haplotypes", torch.int8, "mean")]


def test_store_feature_matrix(ctx, cohort):
    g = f"chr_{CHROM3}"
    rng = np.random.default_rng(5)
    shuffled = [int(x) for x in rng.permutation(S3)[:21]]
    shuffled.insert(9, shuffled[2])                                       # a sample named twice
    one_row = [70, 65, 127, 100]                                          # all in chunk row 1
    names = synth.sample_names(S3)
    for path in cohort["paths"]:
        st = GenotypeStore(path, ctx=ctx)
        maf = st.variant_mask(g, shuffled, min_maf=0.05)
        pruned = st.ld_prune(g, shuffled, variant_mask=maf, window=20, r2=0.2)
        assert 0 < int(pruned.sum()) < int(maf.sum()) < V3
        # (every coding and dtype on the first file, a dosage, a standardized and the haplotypes on the others)
        for coding, dtype, impute in CODINGS if path == cohort["paths"][0] else CODINGS[::6] + CODINGS[-1:]:
            for samples, lo, hi, mask in ((shuffled, 0, V3, pruned), (one_row, 4000, 12500, maf[4000:12500]),
                                          ([names[i] for i in one_row], 4095, 4097, None)):
                idx = [st._sample_index(s) for s in samples]
                X, cols = st.feature_matrix(g, samples, lo, hi, variant_mask=mask, coding=coding, dtype=dtype, impute=impute)
                want, variants = contract(st, g, idx, lo, hi, mask, coding, dtype, impute, sorted(set(idx)))
                assert X.is_cuda and bits_equal(X, want), (path, coding, dtype, impute, lo, hi)
                assert len(cols) == 1 and cols[0][0] == g and cols[0][1].dtype == torch.int64 and torch.equal(cols[0][1], variants)
        # defaults: int8 dosage cannot carry a mean, standardized is float32
        with pytest.raises(ValueError):
            st.feature_matrix(g, one_row)
        X, _ = st.feature_matrix(g, one_row, coding="standardized", variant_mask=maf)
        assert X.dtype == torch.float32
        assert st.feature_matrix(g, one_row, impute="missing")[0].dtype == torch.int8
        # out= reuse: a slice of a wider batch buffer, filled in place, nothing else touched
        want, _ = contract(st, g, shuffled, 0, V3, pruned, "dosage", torch.float16, "mean", sorted(set(shuffled)))
        M = want.shape[1]
        buf = torch.full((len(shuffled), M + 5), 7.0, dtype=torch.float16, device=ctx.device)
        X, _ = st.feature_matrix(g, shuffled, variant_mask=pruned, dtype=torch.float16, out=buf[:, 2:2 + M])
        assert X.data_ptr() == buf[:, 2:].data_ptr() and bits_equal(buf[:, 2:2 + M], want)
        assert bool((buf[:, :2] == 7).all()) and bool((buf[:, 2 + M:] == 7).all())
        with pytest.raises(ValueError):
            st.feature_matrix(g, shuffled, variant_mask=pruned, dtype=torch.float16, out=buf[:, :M + 1])
        with pytest.raises(ValueError):
            st.feature_matrix(g, shuffled, variant_mask=pruned, dtype=torch.float32, out=buf[:, :M])
        # small slabs; a warm read cache, used and left alone
        st.stats.update(gather_blocks=0)
        X, _ = st.feature_matrix(g, shuffled, variant_mask=pruned, dtype=torch.float16, slab_bytes=300_000)
        assert bits_equal(X, want)
        touched = len(set(s // 64 for s in shuffled))
        assert 0 < st.stats["gather_blocks"] <= (len(set(shuffled))) * 5 and touched > 1
        st.read_windows([(g, s, 1000, 4000) for s in shuffled[:4]])
        keys, used, n = list(st._cache), st._cache_used, st.stats["count_compressed_bytes_read"]
        X, _ = st.feature_matrix(g, shuffled[:4], 1000, 4000, dtype=torch.float16, impute="missing")
        assert list(st._cache) == keys and st._cache_used == used and st.stats["count_compressed_bytes_read"] == n
        assert bits_equal(X, contract(st, g, shuffled[:4], 1000, 4000, None, "dosage", torch.float16, "missing", None)[0])
        # the frequencies of a strict subset: the training samples'
        train = shuffled[:8]
        m = st.variant_mask(g, train, min_maf=0.05)
        X, cols = st.feature_matrix(g, shuffled, variant_mask=m, coding="standardized", freq_samples=train)
        want, variants = contract(st, g, shuffled, 0, V3, m, "standardized", torch.float32, "mean", train)
        assert bits_equal(X, want) and torch.equal(cols[0][1], variants)
        own, own_cols = st.feature_matrix(g, shuffled, variant_mask=m, coding="standardized")
        both = torch.isin(own_cols[0][1], variants), torch.isin(variants, own_cols[0][1])
        assert not torch.equal(own[:, both[0]], X[:, both[1]])             # other frequencies, other values
        # the size guard, before anything is allocated
        with pytest.raises(ValueError, match="max_bytes"):
            st.feature_matrix(g, shuffled, dtype=torch.float64, max_bytes=len(shuffled) * V3 * 8 - 1)
        st.feature_matrix(g, shuffled[:2], 0, 100, impute="missing", max_bytes=200)
        for kw in (dict(coding="additive"), dict(dtype=torch.int32, impute="missing"), dict(impute="zero"),
                   dict(coding="haplotypes", dtype=torch.float32)):
            with pytest.raises(ValueError):
                st.feature_matrix(g, one_row, **kw)
        assert tuple(st.feature_matrix(g, [], impute="missing")[0].shape) == (0, V3)
        assert tuple(st.feature_matrix(g, one_row, variant_mask=torch.zeros(V3, dtype=torch.bool), coding="haplotypes")[0].shape) == (4, 0, 2)
        st.close()


def test_dosage_matrix_agrees_with_score(ctx, cohort):
    """feature_matrix(dosage, float64, mean) @ beta against GenotypeStore.score(beta, impute="mean") over the same mask: the
    bound the project documents for that comparison, V * 2^-50 * sum |beta|"""
    g = f"chr_{CHROM3}"
    st = GenotypeStore(cohort["paths"][0], ctx=ctx)
    rng = np.random.default_rng(3)
    samples = [int(x) for x in rng.permutation(S3)[:50]]
    mask = st.variant_mask(g, samples, min_maf=0.05)
    beta = torch.from_numpy(rng.normal(size=(V3, 3))).to(ctx.device)
    X, cols = st.feature_matrix(g, samples, variant_mask=mask, dtype=torch.float64)
    scores, used = st.score(beta, g, samples, variant_mask=mask, impute="mean")
    assert used[g] == X.shape[1] == int(mask.sum())
    got = X @ beta[cols[0][1]] + 0
    bound = X.shape[1] * 2.0 ** -50 * beta[cols[0][1]].abs().sum(0)            # per score, V the variants that take part
    err = (got - scores).abs().max(0).values
    print(f"feature_matrix @ beta against score: max error {err.tolist()}, bound {bound.tolist()}")
    assert bool((err <= bound).all())
    st.close()


def test_several_groups_concatenate(ctx, two_groups):
    st = GenotypeStore(two_groups["path"], ctx=ctx)
    pick = [100, 3, 129, 3, 64]
    masks = {g: st.variant_mask(g, pick, min_maf=0.2) for g in st.groups()}
    for groups in (None, ["chr_11", "chr_3"]):
        for coding, dtype, impute in (("standardized", torch.float32, "mean"), ("dosage", torch.int8, "missing"),
                                      ("haplotypes", torch.int8, "mean")):
            X, cols = st.feature_matrix(groups, pick, variant_mask=masks, coding=coding, dtype=dtype, impute=impute)
            names = st.groups() if groups is None else groups
            assert [c[0] for c in cols] == names
            parts = [contract(st, g, pick, 0, st.meta["groups"][g]["n_variants"], masks[g], coding, dtype, impute, sorted(set(pick)))
                     for g in names]
            assert bits_equal(X, torch.cat([p[0] for p in parts], dim=1))
            assert all(torch.equal(c[1], p[1]) for c, p in zip(cols, parts))
    with pytest.raises(ValueError):
        st.feature_matrix(None, pick, v_lo=5, impute="missing")
    st.close()


def test_reader_and_cli_round_trip(ctx, cohort):
    from click.testing import CliRunner
    from haplohyped_varawareml_amd.features import HEADER, main
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    tab, tmp = cohort["tab"], cohort["tmp"]
    names = synth.sample_names(S3)
    rng = np.random.default_rng(8)
    rows = [names[i] for i in rng.permutation(S3)[:30]]
    train = rows[:20]
    (tmp / "fm_rows.txt").write_text("\n".join(rows) + "\n")
    (tmp / "fm_train.txt").write_text("\n".join(train) + "\n")
    g = f"chr_{CHROM3}"
    with VCFH5Reader(cohort["paths"][0], ctx=ctx) as r:
        st = r.store
        for tr in (None, train):
            donors, X, rec = r.feature_matrix([CHROM3], rows, min_maf=0.05, ld_window=20, coding="standardized",
                                              dtype=torch.float32, train_donor_ids=tr)
            who = rows if tr is None else tr
            mask = st.ld_prune(g, who, variant_mask=st.variant_mask(g, who, min_maf=0.05), window=20, r2=0.2)
            want, variants = contract(st, g, [names.index(x) for x in rows], 0, V3, mask, "standardized", torch.float32, "mean",
                                      sorted(set(names.index(x) for x in who)))
            assert donors == rows and bits_equal(X, want)
            v = variants.cpu().numpy()
            assert np.array_equal(rec["start"], tab["pos"][v].astype(np.int64) - 1) and len(rec) == X.shape[1]
            assert (np.char.decode(rec["chrom"]) == f"chr{CHROM3}").all()
            assert set(rec.dtype.names) == {"chrom", "start", "ref", "alt"}
        for args, coding, dtype, impute in ((["--coding", "standardized"], "standardized", torch.float32, "mean"),
                                            ([], "dosage", torch.int8, "missing"),
                                            (["--dtype", "float16"], "dosage", torch.float16, "mean"),
                                            (["--coding", "haplotypes"], "haplotypes", torch.int8, "mean")):
            prefix = str(tmp / "fm")
            res = CliRunner().invoke(main, ["--h5", cohort["paths"][0], "--out", prefix, "--min_maf", "0.05", "--ld_window", "20",
                                            "--sample_list", str(tmp / "fm_rows.txt"), "--train_sample_list", str(tmp / "fm_train.txt")] + args)
            assert res.exit_code == 0, res.output
            donors, X, rec = r.feature_matrix([CHROM3], rows, min_maf=0.05, ld_window=20, coding=coding, dtype=dtype, impute=impute,
                                              train_donor_ids=train)
            saved = np.load(prefix + ".npy")
            assert saved.dtype == X.cpu().numpy().dtype and saved.tobytes() == X.cpu().numpy().tobytes() and saved.shape == tuple(X.shape)
            assert open(prefix + ".samples.txt").read().split() == rows
            lines = open(prefix + ".variants.tsv").read().splitlines()
            assert lines[0] + "\n" == HEADER and len(lines) == 1 + len(rec)
            assert [x.split("\t")[1] for x in lines[1:]] == [str(int(s) + 1) for s in rec["start"]]
            assert lines[1].split("\t")[0] == f"chr{CHROM3}" and lines[1].split("\t")[2] == rec["ref"][0].decode()
    res = CliRunner().invoke(main, ["--h5", cohort["paths"][0], "--out", str(tmp / "fm"), "--coding", "standardized", "--dtype", "int8"])
    assert res.exit_code != 0
