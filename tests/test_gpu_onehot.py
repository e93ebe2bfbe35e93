"""The one-hot kernels of csrc/onehot.hip through the C ABI: hhgt_onehot_windows (k_overlay + k_onehot) and
hhgt_onehot_bases_u8, against a plain numpy restatement of their contract in include/hhgt.h:
  * window position i reads ref[win_start + i] when 0 <= win_start + i < ref_len, and 'N' otherwise;
  * the records j in [var_lo, var_hi) with win_start <= start[j] < win_start + seq_len are overlaid in index order, so the
    last record at a position wins: allele == 1 gives alt[j], any other allele gives ref[j]; the donor's allele pair of
    record j is geno[j - geno_first];
  * the row of a byte has a 1 in column lut[byte] when lut[byte] < C, and is all zero otherwise.
The restatement is written from those rules alone (not from dataset.channel_lut or the kernels); the CPU tests pin it to
hand-written windows.  The -m gpu tests run the shapes where the kernels loop (more than 2048 records in a window, more
than one grid pass of k_onehot and of k_onehot_bases_u8), the window geometry the dataset never produces, and surround
every output with sentinel bytes that must come back unchanged."""
import ctypes

import numpy as np
import pytest
import torch

# bytes the random references, REF / ALT columns and LUTs draw from; 'Q' is kept for the bytes past ref_len
LETTERS = np.frombuffer(b"ACGTNacgtnRYX-*", dtype=np.uint8)
POISON = ord("Q")
SLACK = 64            # sentinel elements on each side of an output: 64 floats / 64 bytes keep the interior 16-byte aligned
SENTINEL_F = -3.5
SENTINEL_U8 = 0xA5
ONEHOT_PASS = 4096 * 256 * 4        # floats one k_onehot grid pass writes per item (grid capped at 4096 blocks)
BASES_PASS = 65536 * 256 * 4        # bytes one k_onehot_bases_u8 grid pass writes (grid capped at 65536 blocks)


# ---- the restatement ------------------------------------------------------------------------------------------------
def window_letters(L, ref, ref_len, win_start, start, vref, valt, geno, geno_first, var_lo, var_hi):
    """-> uint8 [2, L]: the bases of both haplotypes of one window, by the rules of the module docstring"""
    pos = win_start + np.arange(L, dtype=np.int64)
    seq = np.full(L, ord("N"), np.uint8)
    inside = (pos >= 0) & (pos < ref_len)
    if inside.any():
        seq[inside] = ref[pos[inside]]
    h = np.stack([seq, seq.copy()])
    for j in range(var_lo, var_hi):
        off = int(start[j]) - win_start
        if 0 <= off < L:
            for k in (0, 1):
                h[k, off] = valt[j] if geno[j - geno_first, k] == 1 else vref[j]
    return h


def onehot_rows(letters, lut, C, dtype=np.float32):
    """letters [...] -> [..., C]: a 1 in column lut[byte] when lut[byte] < C"""
    ch = lut[letters].astype(np.int64)
    out = np.zeros(letters.shape + (C,), dtype)
    hit = ch < C
    out[np.nonzero(hit) + (ch[hit],)] = 1
    return out


# ---- known answers for the restatement (CPU) ------------------------------------------------------------------------
def _item(ref=b"", ref_len=None, win_start=0, recs=(), geno=(), geno_first=0, var_lo=0, var_hi=None):
    """recs: (start, REF, ALT) per record; geno: (h0, h1) per record from geno_first on"""
    return dict(ref=np.frombuffer(ref, np.uint8) if ref else None, ref_len=len(ref) if ref_len is None else ref_len,
                win_start=win_start, start=np.array([r[0] for r in recs], np.uint32),
                vref=np.frombuffer(b"".join(r[1] for r in recs), np.uint8),
                valt=np.frombuffer(b"".join(r[2] for r in recs), np.uint8), geno=np.array(geno, np.int8).reshape(-1, 2),
                geno_first=geno_first, var_lo=var_lo, var_hi=len(recs) if var_hi is None else var_hi)


def _letters(L, it):
    h = window_letters(L, **it)
    return h[0].tobytes(), h[1].tobytes()


def test_restatement_reference_edges():
    ref = b"ACGTACGTAC"
    assert _letters(6, _item(ref, win_start=2)) == (b"GTACGT", b"GTACGT")
    assert _letters(6, _item(ref, win_start=-2)) == (b"NNACGT", b"NNACGT")            # before the contig
    assert _letters(5, _item(ref, win_start=8)) == (b"ACNNN", b"ACNNN")                # past ref_len
    assert _letters(4, _item(ref + b"QQQQ", ref_len=10, win_start=9)) == (b"CNNN", b"CNNN")   # bytes past ref_len unread
    assert _letters(3, _item(ref, win_start=-7)) == (b"NNN", b"NNN")                   # wholly before
    assert _letters(3, _item(ref, win_start=20)) == (b"NNN", b"NNN")                   # wholly past
    assert _letters(3, _item(b"", win_start=0)) == (b"NNN", b"NNN")                    # no reference at all


def test_restatement_overlay_rules():
    ref = b"AAAAAAAAAA"
    # allele 1 -> ALT; 0, -9, 2, 3 -> REF (here a REF column that differs from the reference base)
    recs = [(1, b"C", b"G"), (2, b"C", b"G"), (3, b"C", b"G"), (4, b"C", b"G"), (5, b"C", b"G")]
    it = _item(ref, recs=recs, geno=[(1, 0), (0, 1), (-9, 1), (2, 1), (3, 3)])
    assert _letters(7, it) == (b"AGCCCCA", b"ACGGGCA")
    # three records at one position: the last one in [var_lo, var_hi) wins, even where it is REF for the donor
    recs = [(2, b"A", b"C"), (2, b"A", b"G"), (2, b"A", b"T"), (4, b"A", b"C"), (4, b"A", b"T")]
    it = _item(ref, recs=recs, geno=[(1, 1), (1, 0), (0, 1), (1, 1), (0, 1)])
    assert _letters(6, it) == (b"AAAAAA", b"AATATA")      # hap1's last records are REF (A)
    it["var_hi"] = 2                                      # the range ends inside the run: record 1 is the last one seen
    assert _letters(6, it) == (b"AAGAAA", b"AAAAAA")
    it["var_lo"], it["var_hi"] = 3, 5                     # the range starts after the first run
    assert _letters(6, it) == (b"AAAAAA", b"AAAATA")


def test_restatement_window_filter_and_geno_first():
    ref = b"ACGTACGTAC"
    # records before and after the window are in [var_lo, var_hi) but change nothing; geno_first < var_lo
    recs = [(0, b"A", b"T"), (3, b"T", b"A"), (5, b"C", b"G"), (8, b"A", b"C"), (9, b"C", b"G")]
    it = _item(ref, win_start=3, recs=recs, geno=[(9, 9), (1, 1), (1, 0), (0, 1), (1, 1)], geno_first=0, var_lo=1)
    assert _letters(5, it) == (b"AAGGT", b"AACGT")
    # the donor's rows start at record 2: element 0 of geno belongs to record 2
    it = _item(ref, win_start=3, recs=recs, geno=[(1, 0), (0, 1), (1, 1)], geno_first=2, var_lo=2)
    assert _letters(5, it) == (b"TAGGT", b"TACGT")
    # a window before the contig still takes the records it covers
    it = _item(ref, win_start=-3, recs=recs[:1], geno=[(1, 0)])
    assert _letters(4, it) == (b"NNNT", b"NNNA")


def test_restatement_onehot_rows():
    lut = np.full(256, 255, np.uint8)
    lut[ord("A")], lut[ord("C")], lut[ord("G")], lut[ord("T")] = 1, 0, 2, 7    # T: channel >= C -> zero row
    got = onehot_rows(np.frombuffer(b"ACGTN", np.uint8), lut, 3)
    assert got.tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0]]
    lut1 = np.zeros(256, np.uint8)
    lut1[ord("N")] = 1
    assert onehot_rows(np.frombuffer(b"AN", np.uint8), lut1, 1, np.uint8).tolist() == [[1], [0]]


# ---- random windows ---------------------------------------------------------------------------------------------------
def random_lut(rng, C):
    """channels < C for most bytes, some entries >= C (all-zero rows), 'Q' and 'N' told apart by their rows"""
    lut = rng.integers(0, C, 256).astype(np.uint8)
    bad = rng.random(256) < 0.25
    lut[bad] = rng.integers(C, 256, int(bad.sum()))
    lut[ord("X")], lut[ord("*")] = min(C, 255), 255
    lut[POISON] = 0
    lut[ord("N")] = 1 if C > 1 else 255
    return lut


def random_reference(rng, ref_len, pad):
    """ref_len random bases followed by `pad` bytes of POISON the kernel must never read"""
    ref = LETTERS[rng.integers(0, LETTERS.size, ref_len + pad)]
    ref[ref_len:] = POISON
    return ref


def random_table(rng, span, n_pos, max_run=3):
    """records at n_pos sorted positions in [0, span), runs of 1..max_run records at one position; -> start, ref, alt"""
    pos = np.unique(rng.integers(0, span, n_pos))
    pos[0] = 0
    runs = rng.integers(1, max_run + 1, pos.size)
    start = np.repeat(pos, runs).astype(np.uint32)
    vref = LETTERS[rng.integers(0, LETTERS.size, start.size)]
    valt = LETTERS[rng.integers(0, LETTERS.size, start.size)]
    return start, vref, valt


def random_geno(rng, n):
    return rng.choice(np.array([-9, 0, 1, 2, 3], np.int8), size=(n, 2), p=[0.05, 0.4, 0.4, 0.1, 0.05])


def geometry_items(rng, L, ref, ref_len, table):
    """one window of each geometry the header allows and the dataset never produces"""
    start, vref, valt = table
    V = start.size

    def item(win_start, lo=None, hi=None, geno_first=None, with_ref=True):
        if lo is None:
            lo = int(np.searchsorted(start, max(win_start, 0), side="left"))
            hi = int(np.searchsorted(start, max(win_start + L, 0), side="left"))
        gf = lo if geno_first is None else geno_first
        return dict(ref=ref if with_ref else None, ref_len=ref_len if with_ref else 0, win_start=win_start, start=start,
                    vref=vref, valt=valt, geno=random_geno(rng, max(hi - gf, 1)), geno_first=gf, var_lo=lo, var_hi=hi)

    mid = ref_len // 3
    lo_r = int(rng.integers(0, V // 2))
    hi_r = int(rng.integers(lo_r, V + 1))
    return [
        item(mid),                                        # inside the reference, records of the window only
        item(-(L // 2) - 1),                              # starts before the contig
        item(-L - 7),                                     # wholly before the contig
        item(ref_len - L // 2 - 1),                       # runs past ref_len (POISON behind it)
        item(ref_len + 3),                                # wholly past ref_len
        item(mid, with_ref=False),                        # ref_ptr = 0, ref_len = 0
        item(mid, lo=0, hi=V),                            # [var_lo, var_hi) holds records on both sides of the window
        item(max(mid - L, 0), lo=lo_r, hi=hi_r),          # a range that may cut a run of records at one position
        item(mid, lo=max(lo_r, 3), hi=V, geno_first=max(lo_r, 3) - 3),   # geno_first < var_lo
    ]


# ---- the ABI, called the way dataset.py calls it ---------------------------------------------------------------------
def _sync():
    torch.cuda.current_stream().synchronize()


def run_windows(ctx, items, L, lut, C):
    """hhgt_onehot_windows on `items` -> (hap1, hap2) float32 [n, L, C] views into outputs with SLACK sentinel floats on
    both sides, which are checked to be unchanged"""
    from haplohyped_varawareml_amd import _lib
    d = ctx.device
    keep, ptr = [], {}

    def up(a):
        if a is None:
            return 0
        if id(a) not in ptr:
            c = np.ascontiguousarray(a)
            t = torch.from_numpy(c.view(np.int32) if c.dtype == np.uint32 else c).to(d)
            keep.append(t)
            ptr[id(a)] = t.data_ptr()
        return ptr[id(a)]

    ws = (_lib.Window * len(items))()
    for w, it in zip(ws, items):
        w.ref_ptr, w.ref_len, w.win_start = up(it["ref"]), it["ref_len"], it["win_start"]
        w.var_start_ptr, w.var_ref_ptr, w.var_alt_ptr = up(it["start"]), up(it["vref"]), up(it["valt"])
        w.geno_ptr, w.geno_first, w.var_lo, w.var_hi = up(it["geno"]), it["geno_first"], it["var_lo"], it["var_hi"]
    n = len(items) * L * C
    with torch.cuda.device(d):
        d_items = torch.frombuffer(bytearray(bytes(ws)), dtype=torch.uint8).to(d)
        bufs = [torch.full((n + 2 * SLACK,), SENTINEL_F, dtype=torch.float32, device=d) for _ in range(2)]
        outs = [b.data_ptr() + 4 * SLACK for b in bufs]
        assert all(p % 16 == 0 for p in outs)
        _lib.check(ctx.lib.hhgt_onehot_windows(ctx.h, _vp(d_items.data_ptr()), len(items), L, lut.ctypes.data, C,
                                               _vp(outs[0]), _vp(outs[1]), _vp(torch.cuda.current_stream().cuda_stream)))
        _sync()
    for k, b in enumerate(bufs):
        assert bool((b[:SLACK] == SENTINEL_F).all()), f"hap{k + 1}: write below the output"
        assert bool((b[SLACK + n:] == SENTINEL_F).all()), f"hap{k + 1}: write past the output"
    return tuple(b[SLACK:SLACK + n].view(len(items), L, C) for b in bufs)


def _vp(p):
    return ctypes.c_void_p(p)


def _first_diff(got, want):
    bad = np.argwhere(got != want)[0]
    return f"first difference at {tuple(int(x) for x in bad)}: got {got[tuple(bad)]} want {want[tuple(bad)]}"


def assert_windows(ctx, items, L, lut, C):
    """kernel output == restatement for every item; small outputs compared in numpy, large ones on the device"""
    h = run_windows(ctx, items, L, lut, C)
    letters = np.stack([window_letters(L, **it) for it in items], axis=1)          # [2, n, L]
    assert not (letters == POISON).any()                                          # the restatement itself reads no pad
    for k in (0, 1):
        if len(items) * L * C <= 1 << 22:
            got, want = h[k].cpu().numpy(), onehot_rows(letters[k], lut, C)
            assert np.array_equal(got, want), f"hap{k + 1}: " + _first_diff(got, want)
        else:
            lut_t = torch.from_numpy(lut.astype(np.int64)).to(ctx.device)
            want = (lut_t[torch.from_numpy(letters[k]).to(ctx.device).long()].unsqueeze(-1) ==
                    torch.arange(C, device=ctx.device)).float()
            if not torch.equal(h[k], want):
                bad = torch.nonzero(h[k] != want)[0].tolist()
                raise AssertionError(f"hap{k + 1}: first difference at {bad}: got {h[k][tuple(bad)].item()} "
                                     f"want {want[tuple(bad)].item()}")


# ---- hhgt_onehot_windows (-m gpu) -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 3, 5, 1001])
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 7, 254])
def test_windows_geometry(ctx, C, L):
    rng = np.random.default_rng(1000 * C + L)
    ref_len = 4 * L + 50
    ref = random_reference(rng, ref_len, pad=L + 64)
    table = random_table(rng, ref_len + 2 * L + 10, max(ref_len // 2, 8))
    assert_windows(ctx, geometry_items(rng, L, ref, ref_len, table), L, random_lut(rng, C), C)


@pytest.mark.gpu
def test_windows_batch_of_hundreds(ctx):
    """320 items of every geometry in one call (the dataset's batches are 32 at most)"""
    rng = np.random.default_rng(320)
    L, C, ref_len = 1001, 5, 60_000
    ref = random_reference(rng, ref_len, pad=2048)
    table = random_table(rng, ref_len + 3000, 20_000)
    items = []
    while len(items) < 320:
        items += geometry_items(rng, L, ref, ref_len, table)
    assert_windows(ctx, items[:320], L, random_lut(rng, C), C)


def dense_window(rng, L, win_start, ref, ref_len):
    """a window with far more than 2048 records (k_overlay's 8 x 256 threads per item loop), most of them in runs of
    2-3 at one position like a normalised multi-allelic site: REF = the reference base, distinct ALTs, and the donor
    carries the first ALT of every run while the last record of the run is REF for hap1"""
    pos = np.unique(rng.integers(max(win_start, 0), win_start + L, L // 40))
    runs = rng.choice([1, 2, 3], pos.size, p=[0.3, 0.4, 0.3])
    start = np.repeat(pos, runs).astype(np.uint32)
    first = np.concatenate([[0], np.cumsum(runs)[:-1]])
    last = first + runs - 1
    base = np.where(start < ref_len, ref[np.minimum(start, ref_len - 1)], ord("N")).astype(np.uint8)
    vref = np.frombuffer(bytes(base).upper(), np.uint8).copy()
    acgt = np.frombuffer(b"ACGT", np.uint8)
    valt = acgt[rng.integers(0, 4, start.size)]
    valt = np.where(valt == vref, acgt[(np.searchsorted(acgt, valt) + 1) % 4], valt).astype(np.uint8)
    geno = random_geno(rng, start.size)
    multi = runs > 1
    geno[first[multi], 0] = 1
    geno[last[multi], 0] = 0
    return start, vref, valt, geno, int(multi.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("L,C", [(131072, 5), (1_048_576, 4), (1_048_576, 5), (1_000_001, 5), (1_000_001, 7)])
def test_windows_long_and_dense(ctx, L, C):
    """seq_len * C past one k_onehot grid pass (and odd, for the scalar tail), and a window of > 2048 records"""
    rng = np.random.default_rng(L + C)
    ref_len = 3 * L
    ref = random_reference(rng, ref_len, pad=L)
    w0 = L // 2 + 11
    start, vref, valt, geno, n_runs = dense_window(rng, L, w0, ref, ref_len)
    assert start.size > 2 * 2048 * (L // 131072) and n_runs > 1000
    dense = dict(ref=ref, ref_len=ref_len, win_start=w0, start=start, vref=vref, valt=valt, geno=geno, geno_first=0,
                 var_lo=0, var_hi=start.size)
    edge = dict(dense, win_start=ref_len - L // 3, geno=random_geno(rng, start.size))     # past ref_len, no records
    before = dict(dense, win_start=-(L // 2), var_lo=5, geno=geno[3:], geno_first=3)
    items = [dense, edge, before]
    if L * C > ONEHOT_PASS:
        items = items[:2]                       # two items keep the outputs of the widest case at 2 x 56 MB
    assert_windows(ctx, items, L, random_lut(rng, C), C)


# ---- hhgt_onehot_bases_u8 (-m gpu) -----------------------------------------------------------------------------------
def run_bases(ctx, d_bases, lut, C):
    """hhgt_onehot_bases_u8 -> uint8 [n, C] view into an output with SLACK sentinel bytes on both sides (checked)"""
    from haplohyped_varawareml_amd import _lib
    n = d_bases.numel()
    buf = torch.full((n * C + 2 * SLACK,), SENTINEL_U8, dtype=torch.uint8, device=ctx.device)
    out = buf.data_ptr() + SLACK
    assert out % 16 == 0
    with torch.cuda.device(ctx.device):
        _lib.check(ctx.lib.hhgt_onehot_bases_u8(ctx.h, _vp(d_bases.data_ptr()), n, lut.ctypes.data, C, _vp(out),
                                                _vp(torch.cuda.current_stream().cuda_stream)))
        _sync()
    assert bool((buf[:SLACK] == SENTINEL_U8).all()), "write below the output"
    assert bool((buf[SLACK + n * C:] == SENTINEL_U8).all()), "write past the output"
    return buf[SLACK:SLACK + n * C].view(n, C)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1001, 65_537])
@pytest.mark.parametrize("C", [1, 3, 5, 7, 254])
def test_bases_small(ctx, C, n):
    rng = np.random.default_rng(10 * n + C)
    bases = rng.integers(0, 256, n).astype(np.uint8)
    lut = random_lut(rng, C)
    got = run_bases(ctx, torch.from_numpy(bases).to(ctx.device), lut, C).cpu().numpy()
    want = onehot_rows(bases, lut, C, np.uint8)
    assert np.array_equal(got, want), _first_diff(got, want)


@pytest.mark.gpu
def test_bases_rejects_unaligned_output(ctx):
    """d_out must be 4-byte aligned: refused on the host, before any launch"""
    from haplohyped_varawareml_amd import _lib
    d_bases = torch.zeros(16, dtype=torch.uint8, device=ctx.device)
    buf = torch.full((128,), SENTINEL_U8, dtype=torch.uint8, device=ctx.device)
    lut = np.zeros(256, np.uint8)
    with torch.cuda.device(ctx.device), pytest.raises(_lib.HhgtError, match="4-byte aligned"):
        _lib.check(ctx.lib.hhgt_onehot_bases_u8(ctx.h, _vp(d_bases.data_ptr()), 16, lut.ctypes.data, 5, _vp(buf.data_ptr() + 2),
                                                _vp(torch.cuda.current_stream().cuda_stream)))
    _sync()
    assert bool((buf == SENTINEL_U8).all())


def assert_bases_on_device(ctx, d_bases, lut, C, chunk_rows=1 << 25):
    """the whole output against lut[bases] == arange(C), on the device; the rows around every grid-pass boundary once
    more on the host.  -> the number of boundaries that split a row"""
    got = run_bases(ctx, d_bases, lut, C)
    n = d_bases.numel()
    lut_t = torch.from_numpy(lut.astype(np.int64)).to(ctx.device)
    ar = torch.arange(C, device=ctx.device)
    for a in range(0, n, chunk_rows):
        b = min(a + chunk_rows, n)
        want = (lut_t[d_bases[a:b].long()].unsqueeze(1) == ar).to(torch.uint8)
        if not torch.equal(got[a:b], want):
            r = a + int(torch.nonzero((got[a:b] != want).any(1))[0])
            raise AssertionError(f"row {r} (byte {r * C}): got {got[r].tolist()} want {want[r - a].tolist()}")
    n_pass = -(-n * C // BASES_PASS)
    assert n_pass >= 2
    split = 0
    for t in range(1, n_pass):
        r = t * BASES_PASS // C
        split += (t * BASES_PASS) % C != 0
        rows = slice(r - 2, min(r + 3, n))
        want = onehot_rows(d_bases[rows].cpu().numpy(), lut, C, np.uint8)
        assert np.array_equal(got[rows].cpu().numpy(), want), f"rows around pass boundary {t} (row {r})"
    return split


@pytest.mark.gpu
@pytest.mark.parametrize("n,C", [(2 * BASES_PASS // 7 + 12_345, 7), (300_001, 254)])
def test_bases_several_passes(ctx, n, C):
    g = torch.Generator(device=ctx.device).manual_seed(n)
    d_bases = torch.randint(0, 256, (n,), dtype=torch.uint8, device=ctx.device, generator=g)
    assert_bases_on_device(ctx, d_bases, random_lut(np.random.default_rng(n), C), C)


@pytest.mark.gpu
def test_bases_chromosome_1(ctx):
    """one call at the length of GRCh38 chr1 with the fasta_encoder's five columns: 19 grid passes, 15 of whose 18
    boundaries split a row (2^26 is not a multiple of 5)"""
    n, C = 248_956_422, 5
    g = torch.Generator(device=ctx.device).manual_seed(1)
    letters = torch.from_numpy(LETTERS.copy()).to(ctx.device)
    d_bases = letters[torch.randint(0, LETTERS.size, (n,), device=ctx.device, generator=g)]
    lut = random_lut(np.random.default_rng(1), C)
    assert assert_bases_on_device(ctx, d_bases, lut, C) == 15
