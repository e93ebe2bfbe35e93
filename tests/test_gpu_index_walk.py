"""-m gpu: the walking line index (csrc/index.hip, k_index_hop<U, true>; include/hhgt.h hhgt_set_index_mode) — the head of
each record says where its sample columns start, and with FORMAT == "GT" where its newline must be — against the plain scan
of every byte, the hop by the bound, and the oracle: wide random text (every FORMAT / GT shape of tests/test_gpu_fuzz.py at
cohort widths), heads that do not fit the 1 KiB window, records near the end of the text, and the one input shape on which
the walk trusts a newline that is not the record's own."""
import os

import numpy as np
import pytest

from oracle import oracle
from haplohyped_varawareml_amd import synth
from haplohyped_varawareml_amd._lib import HhgtError
from tests.gatk_text import gatk_text
from tests.gpu_util import assert_one_pass, assert_same_as_oracle, gpu_encode
from tests.test_gpu_fuzz import make_text

pytestmark = pytest.mark.gpu


def encode_modes(ctx, text, S, region, modes=(0, 1, 2)):
    out = {}
    try:
        for m in modes:
            ctx.set_index_mode(m)
            out[m] = gpu_encode(ctx, text, S, region=region)
    finally:
        ctx.set_index_mode(-1)
    return out


def same(a, b):
    assert a["n_kept"] == b["n_kept"] and a["stats"] == b["stats"]
    for k in ("G", "start", "stop", "ref", "alt"):
        assert np.array_equal(a[k], b[k]), k
    assert a["res"].chrom_runs == b["res"].chrom_runs


@pytest.mark.parametrize("seed", range(8))
def test_wide_random_text_every_mode(ctx, seed):
    rng = np.random.default_rng(4000 + seed)
    S = int(rng.choice([760, 761, 800, 1023, 1100, 2049]))
    text = make_text(rng, S, int(rng.integers(40, 120)), fixed_share=float(rng.choice([0.0, 0.5, 0.9, 1.0])))
    for region in ("", "chrA"):
        o = oracle.vcf_encode(text, S, region=region)
        g = encode_modes(ctx, text, S, region)
        for m in g:
            assert_same_as_oracle(g[m], o)
        same(g[0], g[2])
        same(g[1], g[2])
        # one pass (what the engine and the converter run): blank / late '##' lines behind short GT records are shapes it
        # may flag, so: the oracle's result or "Error parsing VCF file", never another matrix
        assert_one_pass(ctx, text, S, o, region=region, flaggable=True)


def wide_lines(S, V, seed=7, contig="chr7"):
    text, _ = synth.render_fixed_numpy(contig, synth.variant_table(seed, V, S), S, seed=seed)
    lines = bytes(text).split(b"\n")
    hdr = [x for x in lines if x.startswith(b"#")]
    return hdr, [x for x in lines if x and not x.startswith(b"#")]


@pytest.mark.parametrize("S", [800, 2504])
def test_fixed_width_shard_every_mode(ctx, S):
    """the shape the walk is for: every record costs one 1 KiB head"""
    hdr, rec = wide_lines(S, 900 if S == 800 else 400)
    t = b"\n".join(hdr + rec) + b"\n"
    g = encode_modes(ctx, t, S, "chr7")
    assert g[2]["n_kept"] == len(rec) and g[2]["stats"]["n_general_lines"] == 0
    o = oracle.vcf_encode(t, S, region="chr7")
    assert_same_as_oracle(g[2], o)
    same(g[0], g[2])
    same(g[1], g[2])
    assert_one_pass(ctx, t, S, o, region="chr7")


@pytest.mark.parametrize("S", [800, 2100])
def test_heads_of_every_length(ctx, S):
    """INFO columns from 1 byte to several KiB: nine tabs inside the 1 KiB head, just inside, just outside, far outside"""
    hdr, rec = wide_lines(S, 64)
    out = []
    for k, ln in enumerate(rec):
        f = ln.split(b"\t")
        pad = [1, 200, 900, 960, 975, 985, 990, 1000, 1010, 1500, 5000, 70000][k % 12]
        f[7] = b"X=" + b"q" * pad
        if k % 7 == 3:
            f[8] = b"GT:DP"
            f[9:] = [x + b":%d" % (k % 50) for x in f[9:]]
        out.append(b"\t".join(f))
    t = b"\n".join(hdr + out) + b"\n"
    g = encode_modes(ctx, t, S, "chr7")
    o = oracle.vcf_encode(t, S, region="chr7")
    assert_same_as_oracle(g[2], o)
    same(g[0], g[2])
    assert_one_pass(ctx, t, S, o, region="chr7")     # GT:DP records of two widths in turn: the width of the last one is no guide


@pytest.mark.parametrize("S", [800, 2100])
@pytest.mark.parametrize("tail", ["newline", "none", "crlf", "blank"])
def test_records_near_the_end_of_the_text(ctx, S, tail):
    """the last records of a text: their heads and candidates reach past the last KiB"""
    hdr, rec = wide_lines(S, 5)
    for n in (1, 2, 5):
        t = b"\n".join(hdr + rec[:n])
        t = {"newline": t + b"\n", "none": t, "crlf": t.replace(b"\n", b"\r\n") + b"\r\n", "blank": t + b"\n\n"}[tail]
        g = encode_modes(ctx, t, S, "chr7", modes=(0, 2))
        o = oracle.vcf_encode(t, S, region="chr7")
        assert_same_as_oracle(g[2], o)
        same(g[0], g[2])
        assert_one_pass(ctx, t, S, o, region="chr7")


@pytest.mark.parametrize("S", [800, 2100])
def test_format_that_only_starts_with_gt(ctx, S):
    """FORMAT columns "GTX", "G", "GT:GT", "TG" and a FORMAT of "GT" whose calls are not three bytes wide"""
    hdr, rec = wide_lines(S, 12)
    out = []
    for k, ln in enumerate(rec):
        f = ln.split(b"\t")
        if k % 4 == 1:
            f[8] = b"GT:GQ"
            f[9:] = [x + b":9" for x in f[9:]]
        elif k % 4 == 2:
            f[9:] = [b"0" if (i + k) % 3 == 0 else (b"10|1" if (i + k) % 3 == 1 else x) for i, x in enumerate(f[9:])]
        elif k % 4 == 3:
            f[8] = b"DP:GT"
            f[9:] = [b"7:" + x for x in f[9:]]
        out.append(b"\t".join(f))
    t = b"\n".join(hdr + out) + b"\n"
    g = encode_modes(ctx, t, S, "chr7")
    o = oracle.vcf_encode(t, S, region="chr7")
    assert_same_as_oracle(g[2], o)
    same(g[0], g[2])
    assert_one_pass(ctx, t, S, o, region="chr7")
    for bad in (b"GTX", b"TG", b"G"):          # no GT key: vcfpp.h:550-552 "genotypes not present"
        f = rec[3].split(b"\t")
        f[8] = bad
        t2 = b"\n".join(hdr + rec[:3] + [b"\t".join(f)] + rec[4:]) + b"\n"
        for m in (0, 2):
            ctx.set_index_mode(m)
            try:
                with pytest.raises(HhgtError, match="Error parsing VCF file"):
                    gpu_encode(ctx, t2, S, region="chr7")
            finally:
                ctx.set_index_mode(-1)


@pytest.mark.parametrize("S", [800, 2100])
def test_newline_of_another_line_where_the_head_points(ctx, S):
    """The one shape on which the walk takes a newline that is not the record's own: a FORMAT == "GT" record whose sample
    columns are ONE byte shorter than S diploid calls (one haploid call and one two-digit allele), followed by an empty
    line — the byte at soff + 4 S - 1 is then the empty line's newline.  The merged record is kept, its fields do not
    match "a|b\\t", the variable-width encoder finds the newline inside it: the pass FAILS with HHGT_ERR_MALFORMED (flagged,
    never a different matrix; the same rule as for records shorter than the hop's bound) — which is what the
    asynchronous form reports; the synchronous call then scans every byte (as hhgt_set_index_mode 0 does from the start) and
    decodes what the oracle decodes."""
    hdr, rec = wide_lines(S, 10)
    f = rec[4].split(b"\t")
    f[9 + 17] = b"1"
    f[9 + 40] = b"10|1"
    odd = b"\t".join(f)
    assert len(odd) == len(rec[4]) - 1
    t = b"\n".join(hdr + rec[:4] + [odd, b""] + rec[5:]) + b"\n"
    try:
        want = oracle.vcf_encode(t, S, region="chr7")
    except Exception:
        want = None
    import torch
    from haplohyped_varawareml_amd import device as dev
    from tests.gpu_util import to_dev
    try:
        ctx.set_index_mode(2)
        lay = dev.make_layout(S, 128, sc=64, vc=128)
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=ctx.device)
        res = dev.EncodeResult(z(dev.layout_bytes(lay), torch.uint8), lay, z(lay.v_capacity, torch.int32), z(lay.v_capacity, torch.int32),
                               z(lay.v_capacity, torch.uint8), z(lay.v_capacity, torch.uint8), 0, {})
        with pytest.raises(HhgtError, match="Error parsing VCF file"):       # one pass (the asynchronous form): flagged
            ctx.encode_text_async(to_dev(t), S, res, z(1, torch.int64), max_lines=200, region="chr7").wait()
        if want is not None:                                                 # the synchronous call scans every byte then
            assert_same_as_oracle(gpu_encode(ctx, t, S, region="chr7"), want)
        ctx.set_index_mode(0)
        if want is not None:
            assert_same_as_oracle(gpu_encode(ctx, t, S, region="chr7"), want)
    finally:
        ctx.set_index_mode(-1)
    assert assert_one_pass(ctx, t, S, want, region="chr7", flaggable=True) >= 1     # mode 2 flags it, in both forms
    # without the empty line nothing is special: the candidate is not a newline, the search finds the record's own
    t3 = b"\n".join(hdr + rec[:4] + [odd] + rec[5:]) + b"\n"
    g = encode_modes(ctx, t3, S, "chr7", modes=(0, 2))
    o3 = oracle.vcf_encode(t3, S, region="chr7")
    assert_same_as_oracle(g[2], o3)
    same(g[0], g[2])
    assert_one_pass(ctx, t3, S, o3, region="chr7")


# ---- the hand-overs between the walk's phases (csrc/index.hip: walk_batch -> check_candidate -> search_newline / read_head) --
# Fixed-width GT records — the batch path, four lines per step — with ONE line that breaks the chain, at every slot of the
# four-line step: each kind of break leaves the batch by another door.

def _info(new):
    def f(ln, S):
        c = ln.split(b"\t")
        c[7] = new(c[7])
        return [b"\t".join(c)]
    return f


def _gt_dp(ln, S):
    c = ln.split(b"\t")
    c[8] = b"GT:DP"
    c[9:] = [x + b":7" for x in c[9:]]
    return [b"\t".join(c)]


HAND_OVERS = {
    "info_300_longer": _info(lambda c: c + b"q" * 300),     # the head ends past the batch's 256-byte window, inside the 1 KiB one
    "info_1000": _info(lambda c: b"X=" + b"q" * 998),       # fewer than nine tabs in the 1 KiB head
    "gt_dp": _gt_dp,                         # a FORMAT without a computable width
    "crlf": lambda ln, S: [ln + b"\r"],
    "header_and_blank": lambda ln, S: [ln, b"##note=between the records", b""],
    "one_column_short": lambda ln, S: [b"\t".join(ln.split(b"\t")[:9 + S - 1])],      # the batch head cannot see it (`rehead`)
}
_hand_over_cache = {}


def hand_over_text(kind, k, twice, S=800, V=100):
    """-> (text, the oracle's result or None where it rejects the text).  The break replaces line 40 + k (and, `twice`,
    line 41 + k: two steps in a row that get nowhere switch the batches off for the wave's range); uniform lines follow."""
    if "lines" not in _hand_over_cache:
        _hand_over_cache["lines"] = wide_lines(S, V)
    hdr, rec = _hand_over_cache["lines"]
    out = []
    for j, ln in enumerate(rec):
        out += HAND_OVERS[kind](ln, S) if j == 40 + k or (twice and j == 41 + k) else [ln]
    t = b"\n".join(hdr + out) + b"\n"
    assert len(t) > 3 * WAVE_RANGE
    try:
        return t, oracle.vcf_encode(t, S, region="chr7")
    except RuntimeError as e:
        assert "oracle_vcf_encode failed rc=-2" in str(e), e      # the oracle's parse error (too few sample columns), nothing else
        return t, None


@pytest.mark.parametrize("twice", [False, True], ids=["once", "twice"])
@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("kind", sorted(HAND_OVERS))
def test_hand_overs_between_the_phases(ctx, kind, k, twice):
    S = 800
    t, o = hand_over_text(kind, k, twice, S)
    if kind == "one_column_short":
        assert o is None
        for m in (0, 1, 2):                  # every mode reports HHGT_ERR_MALFORMED
            ctx.set_index_mode(m)
            try:
                with pytest.raises(HhgtError, match="Error parsing VCF file"):
                    gpu_encode(ctx, t, S, region="chr7")
            finally:
                ctx.set_index_mode(-1)
        assert_one_pass(ctx, t, S, None, region="chr7", flaggable=True, forms=[(m, p) for m in (0, 1, 2) for p in (False, True)])
        return
    assert o is not None and o["n_kept"] == 100
    g = encode_modes(ctx, t, S, "chr7")
    for m in g:
        assert_same_as_oracle(g[m], o)
    same(g[0], g[2])
    same(g[1], g[2])
    # (the synchronous call scans every byte once more where a pass fails: one pass of each mode must equal the oracle too)
    assert_one_pass(ctx, t, S, o, region="chr7", forms=[(m, p) for m in (0, 1, 2) for p in (False, True)])


# ---- the width of the last non-GT record as the guess for the next one (the walk's `len_other`) -------------------------
# A non-GT record A, a shorter non-GT record B, then lines whose lengths add up so that one of them ends exactly at
# soff_B + len(A's sample columns): where the last record of B's kind says B's newline is.  Valid text, none of the shapes
# DESIGN.md lets one pass flag: one pass must decode what the oracle decodes.

LEN_OTHER_FORMATS = {
    # FORMAT -> sample column of GT `g` whose numeric sub-field carries `k` extra digits (A is B widened that way)
    "GT:DP": lambda g, k: b"%s:1%s" % (g, b"0" * k),
    "GT:AD:DP:GQ:PL": lambda g, k: b"%s:3,4:7%s:99:120,0,80" % (g, b"0" * k),
    "DP:GT": lambda g, k: b"1%s:%s" % (b"0" * k, g),
}
GTS = [b"0|0", b"0|1", b"1|0", b"1|1", b"0/1", b"./.", b".|1"]
WAVE_RANGE = 6 * 16384      # bytes of text one wave of the walk indexes (csrc/index.hip: 6 regions of INDEX_REGION, texts < 768 MB)


def len_other_text(S, fmt, seed, reps=6):
    """-> (text, triples): GT-only records (the batch path, four lines per step) with (A, B, lines in between) triples at
    shifting offsets — every kind of line in between (a full record, a blank line, a '##' line) for B kept, B an indel and
    B on another contig, `reps` times.  triples: per triple (offset of B's sample columns, offset of the guessed newline)"""
    rng = np.random.default_rng(seed)
    hdr, fill = wide_lines(S, 300, seed=seed)
    cell = LEN_OTHER_FORMATS[fmt.decode()]
    out, triples, fi = list(hdr), [], 0
    size = sum(len(x) + 1 for x in out)

    def add(line):
        nonlocal size
        out.append(line)
        size += len(line) + 1

    def record(contig, ref, extra):
        gts = rng.choice(len(GTS), S)
        ks = [extra // S + (1 if i < extra % S else 0) for i in range(S)]
        cols = b"\t".join(cell(GTS[g], k) for g, k in zip(gts, ks))
        head = b"%s\t%d\t.\t%s\tG\t.\tPASS\tNS=%d\t%s" % (contig, 50_000_000 + int(rng.integers(0, 10 ** 6)), ref, S, fmt)
        return head + b"\t" + cols, len(head) + 1

    variants = [(between, b_kind) for between in ("record", "blank", "header") for b_kind in ("kept", "indel", "contig")]
    for rep in range(reps):
        for j, (between, b_kind) in enumerate(variants):
            for k in range((j + 3 * rep) % 8):             # 0 .. 7 GT records in front: every slot of the four-line step
                f = fill[fi % len(fill)]
                fi += 1
                if k == 0:                                  # and a shift of the byte offsets against the regions
                    c = f.split(b"\t")
                    c[7] = b"X=" + b"a" * int(rng.integers(0, 3000))
                    f = b"\t".join(c)
                add(f)
            if between == "record":
                mid = fill[fi % len(fill)]
                fi += 1
            elif between == "blank":
                mid = b""
            else:
                mid = b"##note=" + b"n" * int(rng.integers(0, 300))
            extra = len(mid) + 1
            a, sa = record(b"chr7", b"A", extra)
            add(a)
            if rep % 2:                                     # GT records between A and B keep the guess
                add(fill[fi % len(fill)])
                fi += 1
            b, sb = record(b"chr8" if b_kind == "contig" else b"chr7", b"AT" if b_kind == "indel" else b"C", 0)
            soff_b = size + sb
            add(b)
            add(mid)
            assert len(a) - sa == len(b) - sb + extra      # the guess soff_B + len(A's columns) is the newline of `mid`
            triples.append((soff_b, soff_b + len(a) - sa))
    for f in fill[fi % len(fill):][:5]:
        add(f)
    return b"\n".join(out) + b"\n", triples


@pytest.mark.parametrize("fmt", [b"GT:DP", b"GT:AD:DP:GQ:PL", b"DP:GT"])
@pytest.mark.parametrize("S", [760, 800, 2100, 2504])
def test_width_of_the_last_other_format_record_is_not_trusted(ctx, S, fmt):
    text, triples = len_other_text(S, fmt, seed=S + len(fmt))
    assert all(text[e:e + 1] == b"\n" for _, e in triples)
    # placements whose guessed newline lies in the same wave's range as B's own (the guess state is per wave)
    inside = sum(b // WAVE_RANGE == e // WAVE_RANGE for b, e in triples)
    assert inside >= 3, inside
    o = oracle.vcf_encode(text, S, region="chr7")
    assert o["n_kept"] == sum(1 for ln in text.split(b"\n") if ln.startswith(b"chr7\t") and b"\tAT\t" not in ln)
    assert_one_pass(ctx, text, S, o, region="chr7")
    assert_same_as_oracle(gpu_encode(ctx, text, S, region="chr7"), o)


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("HHGT_FUZZ_SEEDS", "3")))))
def test_gatk_shaped_text_one_pass(ctx, seed):
    """GATK-shaped cohort text (tests/gatk_text.py: GT:AD:DP:GQ:PL rows 0 .. 100 % missing, widths that vary by
    kilobytes, GT-only rows between, dropped multi-allelic / indel rows): one pass of every index mode, int8 and planes
    form, equals the oracle"""
    rng = np.random.default_rng(9000 + seed)
    S = [760, 2504, 1100, 3000, 801][seed % 5]
    text, n = gatk_text(rng, S, int(rng.choice([8, 16, 30])) << 20, contig="chr3")
    forms = [(m, p) for m in (0, 1, 2) for p in (False, True)]
    for region in ("chr3", "chr3:10000-%d" % (10_000 + 100 * n)):
        o = oracle.vcf_encode(text, S, region=region)
        assert o["n_kept"] > 0 and o["stats"]["n_drop_filter"] > 0
        assert_one_pass(ctx, text, S, o, region=region, forms=forms)
