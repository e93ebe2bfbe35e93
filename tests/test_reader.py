"""CPU: the host reader (C++: mmap + zlib, BGZF blocks inflated in parallel) delivers exactly the
file's text, cut at line boundaries, for plain / gzip / multi-member gzip / BGZF inputs."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from haplohyped_varawareml_amd import synth
from haplohyped_varawareml_amd._lib import HhgtError
from haplohyped_varawareml_amd.reader import VcfReader, _lib_reader, check, parse_header, write_bgzf, write_bgzf_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20


def collect(path, **kw):
    out = []
    with VcfReader(path, **kw) as r:
        bg = r.is_bgzf
        for b in r:
            assert b.size > 0
            out.append(bytes(b))
    return out, bg


@pytest.fixture(scope="module")
def text():
    tab = synth.variant_table(3, 3000, 200)
    t, _ = synth.render_fixed_numpy("chr3", tab, 200, seed=3)
    return t      # ~2.5 MB


@pytest.mark.parametrize("kind", ["plain", "gzip", "gzip2", "bgzf"])
@pytest.mark.parametrize("block", [1 << 20, 8 << 20])
def test_roundtrip(tmp_path, text, kind, block):
    p = str(tmp_path / f"x.{kind}")
    if kind == "plain":
        open(p, "wb").write(text)
    elif kind == "gzip":
        with gzip.open(p, "wb", compresslevel=1) as f:
            f.write(text)
    elif kind == "gzip2":   # concatenated members (bgzip-less tools do this)
        cut = len(text) // 3
        with open(p, "wb") as f:
            f.write(gzip.compress(text[:cut], 1))
            f.write(gzip.compress(text[cut:], 1))
    else:
        write_bgzf(p, text)
    blocks, bg = collect(p, block_bytes=block, n_threads=4)
    assert bg == (kind == "bgzf")
    assert b"".join(blocks) == text
    assert all(b.endswith(b"\n") for b in blocks)
    if block == 1 << 20:
        assert len(blocks) >= 2


def test_no_trailing_newline_and_empty(tmp_path):
    p = str(tmp_path / "a.vcf")
    open(p, "wb").write(b"#x\nline1\nline2")
    blocks, _ = collect(p)
    assert b"".join(blocks) == b"#x\nline1\nline2"
    open(p, "wb").write(b"")
    assert collect(p)[0] == []


def test_reference_fixture_header(golden_dir, fixture_golden):
    with VcfReader(os.path.join(golden_dir, "chr22.filtered.vcf.gz")) as r:
        assert not r.is_bgzf           # the reference's fixture is plain gzip
        b = r.next_block()
        names, hdr = parse_header(b)
        assert names == fixture_golden["samples"]
        assert bytes(b[hdr:hdr + 5]) == b"chr22" and b.size == fixture_golden["text_bytes"]
        assert r.next_block() is None
        assert r.stats()["text_bytes"] == fixture_golden["text_bytes"]


def test_errors(tmp_path):
    from haplohyped_varawareml_amd._lib import HhgtError
    with pytest.raises(HhgtError):
        VcfReader(str(tmp_path / "missing.vcf.gz"))
    p = str(tmp_path / "trunc.vcf.gz")
    open(p, "wb").write(gzip.compress(b"abc\n" * 100000)[:-200])
    with pytest.raises(HhgtError, match="truncated|inflate"):
        collect(p)
    q = str(tmp_path / "long.vcf")
    open(q, "wb").write(b"x" * (3 << 20))
    with pytest.raises(HhgtError, match="longer than"):
        collect(q, block_bytes=1 << 20)


def test_bgzf_crc_mismatch_is_an_error(tmp_path, monkeypatch):
    """htslib's bgzf.c fails a member whose text does not hash to the trailer CRC32; so does the host reader
    (HHGT_BGZF_NO_CRC=1 skips the check)"""
    from haplohyped_varawareml_amd._lib import HhgtError
    text = b"".join(b"chr1\t%d\t.\tA\tG\t.\t.\t.\tGT\t0|1\n" % i for i in range(20000))
    p = str(tmp_path / "c.vcf.gz")
    write_bgzf(p, text, block_size=20000)
    raw = bytearray(open(p, "rb").read())
    assert b"".join(collect(p)[0]) == text and collect(p)[1]
    bsize = raw[16] | (raw[17] << 8)
    raw[bsize + 1 - 8] ^= 0x40                 # CRC32 field of the first member
    open(p, "wb").write(bytes(raw))
    with pytest.raises(HhgtError, match="CRC32"):
        collect(p)
    monkeypatch.setenv("HHGT_BGZF_NO_CRC", "1")
    assert b"".join(collect(p)[0]) == text


def test_crc32_matches_zlib():
    """hhgt_crc32 (PCLMULQDQ folding + table tail) against zlib's crc32 at every alignment / length class"""
    from haplohyped_varawareml_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(5)
    big = rng.integers(0, 256, 70000, dtype=np.uint8)
    for n in list(range(0, 200)) + [255, 256, 257, 1023, 4096, 65280, 65535, 65536, 69999]:
        for off in (0, 1, 7):
            a = np.ascontiguousarray(big[off:off + n])
            assert L.hhgt_crc32(a.ctypes.data, a.size) == (zlib.crc32(a.tobytes()) & 0xFFFFFFFF), (n, off)
    z = np.zeros(65536, np.uint8)
    assert L.hhgt_crc32(z.ctypes.data, z.size) == (zlib.crc32(z.tobytes()) & 0xFFFFFFFF)


@pytest.mark.parametrize("threads,blocks,block_kb", [(1, 2, 1024), (8, 3, 1024), (16, 6, 2048)])
def test_bgzf_many_blocks_in_flight(tmp_path, threads, blocks, block_kb):
    """the barrier-free BGZF path: many ring blocks open to the workers at once, held blocks released out of
    order, every byte and every line boundary intact"""
    from haplohyped_varawareml_amd import reader as rd
    rng = np.random.default_rng(11)
    lines = [b"chr1\t%d\t.\tA\tC\t" % i + bytes(rng.integers(48, 50, int(rng.integers(10, 9000)), dtype=np.uint8)) + b"\n"
             for i in range(6000)]
    text = b"".join(lines)
    p = str(tmp_path / "x.vcf.gz")
    rd.write_bgzf(p, text, level=1)
    L = rd._lib_reader()
    h = C.c_void_p()
    rd.check(L.hhgt_reader_open(p.encode(), block_kb << 10, threads, blocks, C.byref(h)))
    got, held, saw_last = [], [], False
    while True:
        ptr, n, tok, last = C.c_void_p(), C.c_uint64(0), C.c_int(-1), C.c_int(0)
        rd.check(L.hhgt_reader_acquire(h, C.byref(ptr), C.byref(n), C.byref(tok), C.byref(last)))
        if n.value == 0:
            break
        blk = C.string_at(ptr, n.value)
        assert not saw_last
        saw_last = bool(last.value)
        assert blk.endswith(b"\n")
        got.append(blk)
        held.append(tok.value)
        if len(held) >= blocks - 1:                     # keep several blocks, give the newest back first
            rd.check(L.hhgt_reader_release(h, held.pop()))
    for t in held:
        rd.check(L.hhgt_reader_release(h, t))
    L.hhgt_reader_close(h)
    assert saw_last and b"".join(got) == text and len(got) > 3


def test_bgzf_crc_mismatch_is_reported(tmp_path):
    from haplohyped_varawareml_amd import reader as rd
    text = b"".join(b"chr1\t%d\t.\tA\tC\tzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzz\n" % i for i in range(20000))
    p = str(tmp_path / "y.vcf.gz")
    rd.write_bgzf(p, text, level=6)
    raw = bytearray(open(p, "rb").read())
    bsize = raw[16] | (raw[17] << 8)
    raw[bsize + 1 - 8] ^= 0x55                           # CRC field of the first member
    open(p, "wb").write(raw)
    with pytest.raises(Exception, match="CRC32 checksum mismatch"):
        with rd.VcfReader(p, block_bytes=1 << 20, n_threads=4) as r:
            for _ in r:
                pass


def test_peek_sample_count(tmp_path):
    """pipeline.peek_sample_count: the #CHROM line of a plain or gzip / BGZF file -> number of sample columns (what the ingest
    engine is told as expect_samples before it opens)"""
    import gzip
    from haplohyped_varawareml_amd.pipeline import peek_sample_count
    hdr = b"##fileformat=VCFv4.2\n##contig=<ID=chr1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + \
        b"\t".join(b"s%d" % i for i in range(37)) + b"\nchr1\t5\t.\tA\tC\t.\t.\t.\tGT\t" + b"\t".join([b"0|1"] * 37) + b"\n"
    p = tmp_path / "a.vcf"
    p.write_bytes(hdr)
    assert peek_sample_count(str(p)) == 37
    q = tmp_path / "a.vcf.gz"
    with gzip.open(q, "wb") as f:
        f.write(hdr)
    assert peek_sample_count(str(q)) == 37
    sites = tmp_path / "sites.vcf"
    sites.write_bytes(b"##x\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nchr1\t5\t.\tA\tC\t.\t.\t.\n")
    assert peek_sample_count(str(sites)) == 0
    assert peek_sample_count(str(tmp_path / "missing.vcf")) == 0
    nohdr = tmp_path / "n.vcf"
    nohdr.write_bytes(b"chr1\t5\t.\tA\tC\t.\t.\t.\n")
    assert peek_sample_count(str(nohdr)) == 0


# ---- the reader's hand-over through hhgt_reader_acquire: exact fill, lines across members, empty input, errors ------------
EMPTY_MEMBER = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0\x1b\0\x03\0" + b"\0" * 8   # what bgzip ends a file with


def bgzf_members(data, size=0xFF00, level=1):
    """the members of write_bgzf(data), one bytes object each, without the empty end-of-file member"""
    out = []
    for i in range(0, len(data), size):
        chunk = data[i:i + size]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = co.compress(chunk) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp +
                   struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
    return out


def write_as(path, kind, data):
    if kind == "plain":
        open(path, "wb").write(data)
    elif kind == "gzip":
        open(path, "wb").write(gzip.compress(data, 1))
    else:
        open(path, "wb").write(b"".join(bgzf_members(data)) + EMPTY_MEMBER)
    return path


def acquire_all(path, n_threads=3, n_blocks=3, block_bytes=MiB):
    """every block through hhgt_reader_acquire, released at once -> ([(bytes, is_last)], stats at end of file)"""
    L = _lib_reader()
    h = C.c_void_p()
    check(L.hhgt_reader_open(str(path).encode(), block_bytes, n_threads, n_blocks, C.byref(h)))
    try:
        got = []
        while True:
            ptr, n, tok, last = C.c_void_p(), C.c_uint64(0), C.c_int(-2), C.c_int(0)
            check(L.hhgt_reader_acquire(h, C.byref(ptr), C.byref(n), C.byref(tok), C.byref(last)))
            if n.value == 0:
                assert tok.value == -1 and not last.value
                break
            got.append((C.string_at(ptr, n.value), bool(last.value)))
            check(L.hhgt_reader_release(h, tok.value))
        fb, tb = C.c_uint64(0), C.c_uint64(0)
        check(L.hhgt_reader_stats(h, C.byref(fb), C.byref(tb)))
        return got, dict(file_bytes=fb.value, text_bytes=tb.value)
    finally:
        L.hhgt_reader_close(h)


def lines64(total):
    """`total` bytes of 64-byte lines; the last line is shorter where 64 does not divide the total"""
    full = b"".join(b"%062d\t\n" % i for i in range(total // 64))
    return full + (b"x" * (total % 64 - 1) + b"\n" if total % 64 else b"")


PARENT_LENGTHS = {("stream", MiB): [MiB], ("stream", 2 * MiB): [MiB, MiB], ("stream", MiB + 1): [MiB, 1],
                  ("bgzf", 2 * MiB): [1044480, 1044480, 8192], ("bgzf", MiB + 1): [1044480, 4097]}


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf"])
@pytest.mark.parametrize("total", [MiB - 1, MiB, MiB + 1, 2 * MiB])
def test_exact_fill(tmp_path, kind, total):
    """text that fills the 1 MiB blocks to the byte, one short of it and one past it"""
    text = lines64(total)
    assert len(text) == total
    p = write_as(str(tmp_path / "x"), kind, text)
    got, st = acquire_all(p, n_threads=3)
    blocks = [b for b, _ in got]
    assert b"".join(blocks) == text
    assert all(b.endswith(b"\n") for b in blocks)
    assert [last for _, last in got] == [False] * (len(got) - 1) + [True]
    assert st["text_bytes"] == total
    if kind != "gzip":
        assert st["file_bytes"] == os.path.getsize(p)
    want = PARENT_LENGTHS.get(("bgzf" if kind == "bgzf" else "stream", total))
    if want:
        assert [len(b) for b in blocks] == want


@pytest.fixture(scope="module")
def long_lines():
    rng = np.random.default_rng(23)
    return b"".join(bytes(rng.integers(48, 58, int(rng.integers(150000, 400001)) - 1, dtype=np.uint8)) + b"\n" for _ in range(30))


@pytest.mark.parametrize("kind", ["bgzf", "gzip", "plain"])
def test_lines_across_members(tmp_path, long_lines, kind):
    """lines of several members each, empty members between them, a ring of two blocks"""
    p = str(tmp_path / "x")
    if kind == "bgzf":
        ms = bgzf_members(long_lines)
        assert len(ms) > 41
        for at in (40, 4, 3):
            ms.insert(at, EMPTY_MEMBER)
        open(p, "wb").write(b"".join(ms) + EMPTY_MEMBER)
    else:
        write_as(p, kind, long_lines)
    got, st = acquire_all(p, n_threads=4, n_blocks=2)
    assert b"".join(b for b, _ in got) == long_lines
    assert all(b.endswith(b"\n") for b, _ in got) and len(got) > 5
    assert st["text_bytes"] == len(long_lines)


@pytest.mark.parametrize("kind", ["bgzf", "gzip"])
def test_lines_across_members_no_final_newline(tmp_path, long_lines, kind):
    text = long_lines[:-1]
    got, _ = acquire_all(write_as(str(tmp_path / "x"), kind, text), n_threads=4, n_blocks=2)
    assert b"".join(b for b, _ in got) == text


@pytest.mark.parametrize("n", [1, 3])
def test_empty_bgzf(tmp_path, n):
    p = str(tmp_path / "e.vcf.gz")
    open(p, "wb").write(EMPTY_MEMBER * n)
    got, st = acquire_all(p)
    assert got == [] and st == dict(file_bytes=28 * n, text_bytes=0)


def member_offsets(raw):
    off = [0]
    while off[-1] < len(raw):
        off.append(off[-1] + (raw[off[-1] + 16] | (raw[off[-1] + 17] << 8)) + 1)
    return off


@pytest.mark.parametrize("damage,message", [("cut40", "truncated compressed input"), ("half", "truncated compressed input"),
                                            ("header", "corrupt BGZF block header"), ("payload", "inflate failed")])
def test_damaged_bgzf(tmp_path, text, damage, message):
    raw = bytearray(b"".join(bgzf_members(text)) + EMPTY_MEMBER)
    off = member_offsets(raw)
    if damage == "cut40":
        raw = raw[:-40]
    elif damage == "half":
        raw = raw[:len(raw) // 2]
    elif damage == "header":
        raw[off[2] + 12] = 0x58
    else:
        mid = (off[1] + off[2]) // 2
        raw[mid] ^= 0xFF
        raw[mid + 1] ^= 0xFF
    p = str(tmp_path / "d.vcf.gz")
    open(p, "wb").write(bytes(raw))
    with pytest.raises(HhgtError, match=message):
        acquire_all(p)


@pytest.mark.parametrize("kind", ["bgzf", "gzip"])
@pytest.mark.parametrize("head", [b"", b"ab\n"])
def test_one_line_of_three_blocks(tmp_path, kind, head):
    p = write_as(str(tmp_path / "x"), kind, head + b"x" * (3 * MiB - 1) + b"\n")
    with pytest.raises(HhgtError, match="longer than"):
        acquire_all(p)


def newline_free_carry():
    """548 KiB of lines, then one line of 1300 KiB: the second block holds a carry and members without any newline"""
    return lines64(548 << 10) + b"y" * ((1300 << 10) - 1) + b"\n"


@pytest.mark.parametrize("kind", ["bgzf", "gzip", "plain"])
def test_newline_free_carry(tmp_path, kind):
    p = write_as(str(tmp_path / "x"), kind, newline_free_carry())
    with pytest.raises(HhgtError, match="longer than"):
        acquire_all(p)


def test_native_writer_is_independent_of_its_thread_count(tmp_path, text):
    files = []
    for nt in (1, 3, 16, 0):
        p = str(tmp_path / f"w{nt}.vcf.gz")
        write_bgzf_native(p, text, level=6, n_threads=nt)
        files.append(open(p, "rb").read())
    assert all(f == files[0] for f in files[1:])
    got, st = acquire_all(str(tmp_path / "w3.vcf.gz"))
    assert b"".join(b for b, _ in got) == text and st["file_bytes"] == len(files[0])


READER_HIP = os.path.join(ROOT, "haplohyped_varawareml_amd", "csrc", "reader.hip")


def run_harness(tmp_path, text, sanitize, reader_hip=READER_HIP):
    """builds tests/reader_harness.cpp with csrc/reader.hip under a host sanitizer and runs it on files written here"""
    from haplohyped_varawareml_amd.build import _hipcc
    exe = str(tmp_path / "reader_harness")
    subprocess.check_call([_hipcc(), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-mssse3", "-Wno-unused-value"] +
                          ["-Xarch_host"] + " -Xarch_host ".join(sanitize).split() +
                          ["-o", exe, os.path.join(ROOT, "tests", "reader_harness.cpp"), reader_hip, "-lz", "-lpthread"])
    paths = [str(tmp_path / n) for n in ("text", "bgzf", "gzip", "plain", "too_long", "missing")]
    open(paths[0], "wb").write(text)
    for p, kind in zip(paths[1:4], ("bgzf", "gzip", "plain")):
        write_as(p, kind, text)
    write_as(paths[4], "bgzf", newline_free_carry())
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    return subprocess.run([exe] + paths, capture_output=True, text=True, timeout=300, env=env)


@pytest.mark.parametrize("sanitize", [["-fsanitize=thread"], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["thread", "address"])
def test_harness_under_sanitizers(tmp_path, text, sanitize):
    """the C API driven as the ingest engine drives it (tests/reader_harness.cpp), as a program of its own: scanner, workers
    and consumer under ThreadSanitizer, and under AddressSanitizer / UBSan.  Host code only: never where a device is visible"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a sanitized program must not open a device: this test runs on CPU-only hosts")
    r = run_harness(tmp_path, text, sanitize)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "Sanitizer" not in r.stderr, r.stdout + r.stderr
