"""-m gpu: the encode path the way a few-sample, whole-chromosome file drives it: one text block of millions of short lines.

- The per-line scan (csrc/scan.hip launch_scan_exclusive_u32_pair) gives every line its kept index and CHROM-run index.  Above
  SCAN_SHORT_MAX tiles it takes a three-launch form (k_scan_reduce / k_scan_partials / k_scan_down) that only texts of more
  than 2048 x 2048 lines reach; k_scan_partials carries across its 256-partial loop beyond 256 tiles.  Contig changes, dropped
  records, a '##' and an empty line sit at the line indices where those forms split the work, and every form is checked against
  the oracle: synchronous encode (exact line count), asynchronous encode into G and into bit planes with the caller's bound on
  either side of the threshold, and the ingest engine (one 512 MiB device-inflate block and several 64 MiB host blocks).
- A text block may hold any number of CHROM runs up to MAX_CHROM_RUNS (4096): every CHROM change and every empty or header line
  starts one.  The engine, the synchronous encode, the Python block loop and the oracle agree on such texts.
- The line index holds up to INDEX_CAP (1024) newlines per 16 KiB region: text at the cap encodes exactly, one newline more is
  an error, never a shorter line list.

Every expected value comes from the oracle on the same bytes."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from haplohyped_varawareml_amd import synth
from haplohyped_varawareml_amd._lib import HhgtError
from haplohyped_varawareml_amd.pipeline import stream_file
from haplohyped_varawareml_amd.reader import write_bgzf, write_bgzf_native
from tests.gpu_util import assert_same_as_oracle, gpu_encode, gpu_encode_one_pass
from tests.test_gpu_ingest import check_against_oracle, run_engine

pytestmark = pytest.mark.gpu

TILE = 2048                 # entries per scan tile (SCAN_TILE)
SHORT_MAX = 2048            # tiles up to which the scan takes its two-launch form (SCAN_SHORT_MAX)
LONG = TILE * SHORT_MAX     # 4,194,304 scanned lines: one more and the three-launch form runs
CARRY = 256 * TILE          # k_scan_partials carries across its loop beyond this many lines
MAX_RUNS = 4096             # MAX_CHROM_RUNS
ERR_CAPACITY, ERR_LINE_DENSITY = -3, -5
N_LINES = LONG + 3 * TILE + 77
MODEST = 600_000

SNP, MULTI, INDEL, META, EMPTY = 0, 1, 2, 3, 4     # line kinds of render()


def long_form(max_lines):
    return -(-max_lines // TILE) > SHORT_MAX


def header(S, names=None):
    if S:
        return synth.header_text("chr1", names or synth.sample_names(S))
    return b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def render(S, names, cidx, kind, pos, seed, head):
    """-> (uint8 text, line_end uint64[header lines + len(kind)]): head, then one line per entry of `kind` — SNP a biallelic
    SNP record, MULTI a record with ALT 'X,Y' and INDEL one with a two-base REF (both dropped by the SNP filter), META a '##'
    line, EMPTY an empty line.  names: contig names of one width; cidx, pos (< 10^9): per line.  Vectorised: a row per line,
    the columns a kind does not have masked out."""
    n = len(kind)
    rng = np.random.default_rng(seed)
    nm = np.frombuffer("".join(names).encode(), np.uint8).reshape(len(names), -1)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    r = rng.integers(0, 4, n)
    a = (r + rng.integers(1, 4, n)) % 4
    col = lambda b: np.broadcast_to(np.frombuffer(b, np.uint8), (n, len(b)))
    one = lambda x: np.asarray(x, np.uint8)[:, None]
    pos = np.asarray(pos, np.int64)
    parts = [(nm[cidx], None), (col(b"\t"), None),
             (((pos[:, None] // 10 ** np.arange(8, -1, -1)) % 10 + 48).astype(np.uint8), None),
             (col(b"\t.\t"), None), (one(acgt[r]), None), (one(acgt[(r + 1) % 4]), kind == INDEL),
             (col(b"\t"), None), (one(acgt[a]), None), (col(b","), kind == MULTI), (one(acgt[(a + 1) % 4]), kind == MULTI),
             (col(b"\t.\t.\t."), None)]
    if S:
        gt = np.where(rng.random((n, S, 2)) < 0.03, ord("."), 48 + rng.integers(0, 2, (n, S, 2))).astype(np.uint8)
        sep = np.where(rng.random((n, S)) < 0.1, ord("/"), ord("|")).astype(np.uint8)
        parts.append((col(b"\tGT"), None))
        for s in range(S):
            parts += [(col(b"\t"), None), (one(gt[:, s, 0]), None), (one(sep[:, s]), None), (one(gt[:, s, 1]), None)]
    parts.append((col(b"\n"), None))
    rows = np.concatenate([p for p, _ in parts], axis=1)
    mask = np.concatenate([np.ones(p.shape, bool) if m is None else np.repeat(m[:, None], p.shape[1], axis=1)
                           for p, m in parts], axis=1)
    for k, line in ((META, b"##note=1\n"), (EMPTY, b"\n")):
        sel = kind == k
        rows[sel, :len(line)] = np.frombuffer(line, np.uint8)
        mask[sel] = np.arange(rows.shape[1]) < len(line)
    hb = np.frombuffer(head, np.uint8)
    text = np.concatenate([hb, rows[mask]])
    h_ends = np.nonzero(hb == 10)[0].astype(np.uint64) + 1
    line_end = np.concatenate([h_ends, len(hb) + np.cumsum(mask.sum(axis=1), dtype=np.uint64)])
    return text, line_end


def scan_text(S):
    """N_LINES lines (header included): contigs chr1 / chr2 / chr3, 10 % of the records dropped at random, and at each scan
    edge E (tile 1 / 2, the partials carry, the long form's threshold) line E - 1 a dropped multi-allelic record, line E a kept
    record that changes the contig, line E + 1 a dropped record that changes it again.  One '##' and one empty line"""
    head = header(S)
    H = head.count(b"\n")
    n = N_LINES - H
    rng = np.random.default_rng(40 + S)
    kind = np.where(rng.random(n) < 0.9, SNP, np.where(rng.random(n) < 0.5, MULTI, INDEL))
    change = np.zeros(n, np.int64)
    for E in (TILE, CARRY, LONG):
        kind[E - 1 - H], kind[E - H], kind[E + 1 - H] = MULTI, SNP, INDEL
        change[E - H] = change[E + 1 - H] = 1
    kind[1000 - H], kind[3_000_000 - H] = META, EMPTY
    cidx = np.cumsum(change) % 3
    pos = 100_000_000 + np.cumsum(rng.integers(1, 40, n))
    text, line_end = render(S, ["chr1", "chr2", "chr3"], cidx, kind, pos, 50 + S, head)
    beg, end = int(pos[CARRY + TILE // 2 - H]), int(pos[LONG - 2 - H])    # (inside chr2's long run, which ends at LONG - 1)
    return dict(text=text, line_end=line_end, regions=["", "chr2", f"chr2:{beg}-{end}"])


@pytest.fixture(scope="module")
def scan_texts():
    """S = 3 and S = 0 (sites only): the whole text, its first LONG lines and its first MODEST lines, on the host and the
    device; oracle results are cached per (S, cut, region)"""
    out = {}
    for S in (3, 0):
        t = scan_text(S)
        whole = t["text"]
        assert len(t["line_end"]) == N_LINES and whole.size == int(t["line_end"][-1])
        cuts = {"whole": whole, "long": whole[:int(t["line_end"][LONG - 1])], "modest": whole[:int(t["line_end"][MODEST - 1])]}
        d = _to_dev(whole)
        out[S] = dict(regions=t["regions"], host=cuts, dev={k: d[:v.size] for k, v in cuts.items()},
                      lines={"whole": N_LINES, "long": LONG, "modest": MODEST}, oracle={})
    yield out
    out.clear()
    torch.cuda.empty_cache()


def _to_dev(a):
    t = torch.empty(a.size + 64, dtype=torch.uint8, device="cuda")
    t[:a.size] = torch.from_numpy(a)
    return t[:a.size]


def want(texts, S, cut, region):
    key = (cut, region)
    if key not in texts[S]["oracle"]:
        texts[S]["oracle"][key] = oracle.vcf_encode(texts[S]["host"][cut], S, region=region, want_chrom="bytes")
    return texts[S]["oracle"][key]


def per_record_names(runs, n_kept):
    """CHROM runs [(first kept index, name)] -> uint8 [n_kept, 32], the oracle's per-record CHROM column"""
    if not runs:
        return np.zeros((0, 32), np.uint8)
    firsts = np.array([f for f, _ in runs] + [n_kept], np.int64)
    names = np.zeros((len(runs), 32), np.uint8)
    for i, (_, nm) in enumerate(runs):
        names[i, :len(nm)] = np.frombuffer(nm.encode(), np.uint8)
    assert firsts[0] == 0 or n_kept == 0, runs[:4]
    return np.repeat(names, np.diff(firsts), axis=0)      # (a decreasing first index raises here)


def assert_runs(runs, o):
    got = per_record_names(runs, o["n_kept"])
    assert got.shape == o["chrom"].shape and np.array_equal(got, o["chrom"]), "CHROM runs differ from the per-record CHROM column"


def merged(runs):
    """consecutive runs of one name as one (the continuation rule of the engine and of the Python block loop)"""
    out = []
    for first, name in runs:
        if not out or out[-1][1] != name:
            out.append((first, name))
    return out


# ---- A: both forms of the line scan -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 0])
def test_scan_forms_synchronous(ctx, scan_texts, S):
    """the synchronous form scans the exact line count: the whole text takes the three-launch form, its first 2048 x 2048
    lines the largest two-launch one"""
    T = scan_texts[S]
    for cut in ("whole", "long"):
        n = T["lines"][cut]
        assert long_form(n) == (cut == "whole")
        for region in T["regions"]:
            o = want(scan_texts, S, cut, region)
            g = gpu_encode(ctx, T["dev"][cut], S, region=region)
            assert g["stats"]["n_lines"] == n == o["stats"]["n_lines"]
            assert 0 < o["n_kept"] < o["stats"]["n_records"]
            try:
                assert_same_as_oracle(g, o)
                assert_runs(g["res"].chrom_runs, o)
            except AssertionError as e:
                raise AssertionError(f"S {S}, {cut} text, region {region!r}: {e}") from e


@pytest.mark.parametrize("S", [3, 0])
def test_scan_forms_asynchronous(ctx, scan_texts, S):
    """the asynchronous forms scan the caller's bound: short and long form on either side of 2048 x 2048, a long form whose
    last tile holds one entry, and a modest text under a bound far above its line count"""
    T = scan_texts[S]
    cases = [("whole", N_LINES + 64), ("long", LONG), ("long", LONG + 1), ("modest", MODEST), ("modest", LONG + TILE + 5)]
    for cut, max_lines in cases:
        assert long_form(max_lines) == (max_lines > LONG)
        for region in T["regions"]:
            o = want(scan_texts, S, cut, region)
            for planes in ((False, True) if S else (False,)):
                g = gpu_encode_one_pass(ctx, T["dev"][cut], S, region=region, planes=planes, max_lines=max_lines,
                                        **(dict(sc=64, vc=8192) if planes else {}))
                assert g["stats"]["n_lines"] == T["lines"][cut]
                try:
                    assert_same_as_oracle(g, o)
                    assert g["stats"]["n_chrom_runs"] <= 16   # (the result record carries 16 runs: all of them here)
                    assert_runs(g["res"].chrom_runs, o)
                except AssertionError as e:
                    raise AssertionError(f"S {S}, {cut} text, max_lines {max_lines}, region {region!r}, planes {planes}: {e}") from e


# ---- B: the ingest engine at that scale, and with many CHROM runs in one block ------------------------------------------------
def test_engine_whole_chromosome_block(ctx, tmp_path, scan_texts):
    """S = 3 as BGZF, the records twice (8.4 M lines).  Inflated on the device the blocks grow to hundreds of MiB: the line
    bound of the biggest is above 2048 x 2048, so its scans take the long form.  On the host: 64 MiB blocks, the short
    form.  Both the oracle's, whole and under a region"""
    whole = scan_texts[3]["host"]["whole"]
    text = np.concatenate([whole, whole[len(header(3)):]])
    p = str(tmp_path / "chr.vcf.gz")
    write_bgzf_native(p, text, level=1, n_threads=8)
    n_lines = 2 * N_LINES - header(3).count(b"\n")
    for region in ("", "chr2"):
        o = oracle.vcf_encode(text, 3, region=region, want_chrom="bytes")
        got = {}
        for device_inflate in (True, False):
            r = run_engine(ctx, [(p, region)], device_inflate=device_inflate)[0]
            st = r["stats"]
            assert st["n_lines"] == n_lines and bool(st["device_inflate"]) == device_inflate
            if region == "" and device_inflate:
                # a kept record here has at least 42 bytes, so the block that kept most held more than biggest * 42 bytes, and
                # the engine's line bound for it, bytes / (2 S + 17) + 64, is above 2048 x 2048 (64 MiB host blocks: below)
                biggest = max(len(x) for x in r["start"])
                assert biggest * 42 // (2 * 3 + 17) > LONG, (biggest, st)
            check_against_oracle(r, text, 3, region, 64, 8192)
            assert_runs(r["runs"], o)
            got[device_inflate] = r["runs"]
        assert got[True] == got[False]


def many_runs_case(name):
    """(text, region) of S = 3 with more than 16 CHROM runs in one block"""
    rng = np.random.default_rng(len(name))
    S = 3
    if name in ("contigs40", "contigs40_region"):
        names = [f"ctg{i:02d}" for i in range(40)]
        cidx = np.repeat(np.arange(40), 60)
        region = "ctg17" if name == "contigs40_region" else ""
    elif name == "blank_lines":
        names, cidx, region = ["chr7"], np.zeros(3000, np.int64), ""
    else:
        k = MAX_RUNS if name == "runs4096" else MAX_RUNS + 1
        names, cidx, region = [f"c{i:04d}" for i in range(k)], np.arange(k), ""
    n = len(cidx)
    kind = np.where(rng.random(n) < 0.9, SNP, MULTI)
    if name == "blank_lines":
        at = rng.choice(np.arange(10, n), 40, replace=False)
        kind[at[:20]], kind[at[20:]] = EMPTY, META
    pos = 100_000_000 + np.cumsum(rng.integers(1, 900, n))
    text, _ = render(S, names, cidx, kind, pos, 7, header(S))
    return text, region


@pytest.mark.parametrize("name", ["contigs40", "contigs40_region", "blank_lines", "runs4096"])
def test_many_runs_agree_everywhere(ctx, tmp_path, name):
    """engine, synchronous encode, Python block loop (the parse_vcf facade's stream_file(compress=False)) and oracle: the same
    per-record CHROM names, and the same run table once consecutive runs of one name are merged"""
    text, region = many_runs_case(name)
    S = 3
    o = oracle.vcf_encode(text, S, region=region, want_chrom="bytes")
    g = gpu_encode(ctx, text, S, region=region)
    assert_same_as_oracle(g, o)
    sync_runs = g["res"].chrom_runs
    assert len(sync_runs) == g["stats"]["n_chrom_runs"] > 16
    assert_runs(sync_runs, o)
    r = run_engine(ctx, [(text, region)])[0]
    check_against_oracle(r, text, S, region, 64, 8192)
    assert_runs(r["runs"], o)
    p = str(tmp_path / "t.vcf")
    text.tofile(p)
    fs = stream_file(ctx, p, region=region, compress=False)
    assert fs.n_kept == o["n_kept"]
    assert r["runs"] == fs.chrom_runs == merged(sync_runs)
    if name == "runs4096":
        assert len(sync_runs) == MAX_RUNS and len(r["runs"]) == MAX_RUNS


def test_run_limit_is_an_error(ctx):
    """one run more than MAX_CHROM_RUNS: HHGT_ERR_CAPACITY naming the limit, from the synchronous encode and the engine"""
    text, region = many_runs_case("runs4097")
    for run in (lambda: gpu_encode(ctx, text, 3, region=region), lambda: run_engine(ctx, [(text, region)])):
        with pytest.raises(HhgtError) as e:
            run()
        assert e.value.code == ERR_CAPACITY and "4097" in str(e.value) and "4096" in str(e.value), str(e.value)
        assert "not sorted" not in str(e.value)


def test_converter_ignores_empty_lines(tmp_path, golden_dir, fixture_golden):
    """VCFtoHDF5Converter on a per-chromosome file with 40 empty lines in one block writes the .h5 it writes without them"""
    from haplohyped_varawareml_amd.vcf_to_h5 import VCFtoHDF5Converter
    names = fixture_golden["samples"]
    S, n = len(names), 30000
    rng = np.random.default_rng(77)
    pos = 100_000_000 + np.cumsum(rng.integers(1, 500, n))
    kind = np.where(rng.random(n) < 0.95, SNP, INDEL)
    head = synth.header_text("chr7", names)
    plain, line_end = render(S, ["chr7"], np.zeros(n, np.int64), kind, pos, 8, head)
    behind = np.sort(rng.choice(np.arange(head.count(b"\n") + 100, len(line_end) - 1), 40, replace=False))
    with_blank = np.frombuffer(b"\n".join(x.tobytes() for x in np.split(plain, line_end[behind].astype(np.int64))), np.uint8)
    assert with_blank.size == plain.size + 40
    samples = os.path.join(golden_dir, "ipscs_samples_test.txt")
    out = {}
    for tag, text in (("plain", plain), ("blank", with_blank)):
        vcf_dir = tmp_path / tag
        vcf_dir.mkdir()
        write_bgzf(str(vcf_dir / "chr7.filtered.vcf.gz"), text.tobytes())
        conv = VCFtoHDF5Converter("c", str(vcf_dir), str(tmp_path / f"out_{tag}"), samples, 2, 1, n_gpus=1)
        assert conv.run() == conv.h5_path
        out[tag] = open(conv.h5_path, "rb").read()
    assert out["plain"] == out["blank"]


# ---- D: the line index's density cap ----------------------------------------------------------------------------------------
RECORD16 = b"1\t5\t.\tA\tC\t.\t.\t.\n"      # sites-only record of 16 bytes: 1024 newlines in every 16 KiB region


def region_counts(text):
    t = np.frombuffer(text, np.uint8)
    return np.add.reduceat((t == 10).astype(np.int64), np.arange(0, t.size, 16384))


def test_line_density_cap(ctx):
    assert len(RECORD16) == 16
    M = 1 << 16
    text = header(0) + RECORD16 * M
    assert region_counts(text).max() == 1024
    o = oracle.vcf_encode(text, 0)
    assert o["n_kept"] == M
    assert_same_as_oracle(gpu_encode(ctx, text, 0), o)
    assert_same_as_oracle(gpu_encode_one_pass(ctx, text, 0), o)
    r = run_engine(ctx, [(np.frombuffer(text, np.uint8), "")], sites_only=True)[0]
    assert r["stats"]["n_kept"] == M and np.array_equal(np.concatenate(r["start"]), o["start"])
    # one empty line more inside one region
    h = len(header(0))
    at = h + 16 * ((5 * 16384 - h) // 16 + 8)
    over = text[:at] + b"\n" + text[at:]
    assert region_counts(over).max() == 1025
    with pytest.raises(HhgtError) as e:
        gpu_encode(ctx, over, 0)
    assert e.value.code == ERR_LINE_DENSITY
    with pytest.raises(HhgtError) as e:
        gpu_encode_one_pass(ctx, over, 0)
    assert e.value.code == ERR_LINE_DENSITY
    with pytest.raises(HhgtError):
        run_engine(ctx, [(np.frombuffer(over, np.uint8), "")], sites_only=True)
