"""CPU: crafted DEFLATE streams (tests/deflate_craft.py) against the arbiters and the host inflater.

* the writer itself: zlib inflates every valid case to the text the writer meant and rejects every invalid one (with
  zlib's own message where it has one); libdeflate agrees, except where listed below;
* the host decoder (csrc/fast_inflate.h, `hhgt_fast_inflate`): 0 with zlib's bytes or a negative code, never 0 on a
  stream zlib rejects, nothing written outside the output; the valid streams it leaves to zlib are listed by name;
* a libdeflate-written BGZF file through the reader, with either host inflater."""
import hashlib
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tests import deflate_craft as dc
from tests import extlibs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dc.corpus()
IDS = [c.name for c in CASES]

# streams libdeflate 1.10 accepts although zlib rejects them (zlib's verdict is the rule here):
LIBDEFLATE_ACCEPTS = {
    "repeat_past_hlit_plus_hdist",               # a code-length repeat running past HLIT + HDIST is cut, not an error
    "fixed_symbol_286",                          # literal/length symbols 286 / 287 decode as length 258
    "fixed_symbol_287",
    "single_one_bit_distance_code_unused_half",  # a single 1-bit code answers to both '0' and '1'
}
# valid streams the host decoder declines (it returns < 0, the reader inflates the member with zlib instead): a
# literal/length code of one 1-bit code (build_table with need_complete)
HOST_DECLINES = {"literal_length_code_only_eob"}


def zlib_verdict(payload):
    """-> (accepted, bytes, message): raw inflate with zlib; accepted = no error and the final block was reached"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload) + d.flush()
    except zlib.error as e:
        return False, None, str(e)
    return d.eof, out, None


def test_corpus_covers_every_status():
    got = {c.status for c in CASES}
    assert got >= {dc.OK, dc.BAD_BLOCK_TYPE, dc.BAD_STORED, dc.BAD_TABLE, dc.BAD_CODE, dc.BAD_DISTANCE, dc.OUTPUT_OVERRUN,
                   dc.SIZE_MISMATCH, dc.ANY}
    assert sum(c.status == dc.OK for c in CASES) >= 35 and sum(c.status != dc.OK for c in CASES) >= 30
    assert HOST_DECLINES <= set(IDS) and LIBDEFLATE_ACCEPTS <= set(IDS)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_zlib_is_the_arbiter(case):
    ok, out, msg = zlib_verdict(case.payload)
    if case.status == dc.OK:
        assert msg is None and ok, msg
        assert out == case.text and len(out) == case.isize
    elif case.status in (dc.OUTPUT_OVERRUN, dc.SIZE_MISMATCH):
        # a valid stream whose BGZF trailer states another size: zlib inflates it, the gzip layer rejects the member
        assert ok and out == case.text and len(out) != case.isize
        d = zlib.decompressobj(31)
        with pytest.raises(zlib.error, match="incorrect length check"):
            d.decompress(dc.bgzf_member(case.payload, case.text, case.isize))
    else:
        assert not ok
        if case.zmsg is not None:
            assert msg is not None and msg.endswith(case.zmsg), msg
    if len(case.payload) + 26 <= 65536:       # the BGZF framing: CRC-32 and ISIZE of the intended text
        m = dc.bgzf_member(case.payload, case.text, case.isize)
        assert len(m) == int.from_bytes(m[16:18], "little") + 1


def test_writer_run_length_coding():
    assert dc.expand([(18, 138), 5, (16, 6), (17, 3), (16, 3)]) == [0] * 138 + [5] * 7 + [0] * 6
    lens = [0] * 140 + [7] * 10 + [0] * 4
    assert dc.rle(lens, {}) == [(18, 138), 0, 0, 7, (16, 6), (16, 3), (17, 4)]
    assert dc.rle(lens, {141: (16, 3), 150: (17, 4)}) == [(18, 138), 0, 0, 7, (16, 3), 7, (16, 5), (17, 4)]
    with pytest.raises(AssertionError):
        dc.rle(lens, {139: (16, 3)})          # a 16 must repeat the length before it
    for lens in ([8] * 226 + [9] * 60, [5] * 28 + [4] * 2, dc.huffman_lengths([1, 2, 4, 8, 16, 32, 64, 128, 256], 5)):
        assert dc.kraft(lens) == 1 << 15
    codes = dc.canonical(dc.FIXED_LL)
    assert codes[0] == (0b00110000, 8) and codes[256] == (0, 7) and codes[144] == (0b110010000, 9)


@pytest.mark.skipif(not extlibs.have_libdeflate(), reason="libdeflate is not loadable on this box")
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_libdeflate_agrees_with_zlib(case):
    zok, zout, _ = zlib_verdict(case.payload)
    r, out = extlibs.deflate_decompress(case.payload)
    if case.name in LIBDEFLATE_ACCEPTS:
        assert not zok and r == 0, "listed as a disagreement, but libdeflate and zlib agree now"
        return
    assert (r == 0) == zok, (r, zok)
    if zok:
        assert out == zout


@pytest.fixture(scope="module")
def fast_inflate():
    from haplohyped_varawareml_amd import _lib
    return _lib.load().hhgt_fast_inflate


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_inflater_never_disagrees_with_zlib(fast_inflate, case):
    """out = ISIZE bytes between 256-byte sentinels; the decoder must keep to them whatever the stream says"""
    zok, zout, _ = zlib_verdict(case.payload)
    zaccepts = zok and len(zout) == case.isize
    src = np.frombuffer(case.payload, dtype=np.uint8).copy()
    buf = np.full(case.isize + 512, 0xA5, dtype=np.uint8)
    rc = fast_inflate(src.ctypes.data, src.size, buf.ctypes.data + 256, case.isize)
    assert (buf[:256] == 0xA5).all() and (buf[256 + case.isize:] == 0xA5).all(), "wrote outside the output"
    if rc == 0:
        assert zaccepts, "the host decoder accepts a stream zlib rejects"
        assert buf[256:256 + case.isize].tobytes() == zout
    else:
        assert rc < 0
        if case.status == dc.OK:
            assert case.name in HOST_DECLINES, f"declines a valid stream (rc {rc}) that is not listed"
    if case.name in HOST_DECLINES:
        assert rc < 0 and zaccepts, "listed as declined, but the host decoder inflates it now"


def test_bgzf_scan_of_crafted_members():
    """the host's member walk over crafted members (CRC-32 / ISIZE of the intended text)"""
    cases = [c for c in CASES if len(c.payload) + 26 <= 65536]
    raw = b"".join(dc.bgzf_member(c.payload, c.text, c.isize) for c in cases)
    from haplohyped_varawareml_amd import device as dev
    tab = dev.bgzf_scan(raw)
    assert len(tab["isize"]) == len(cases) and tab["consumed"] == len(raw)
    assert [int(x) for x in tab["comp_len"]] == [len(c.payload) for c in cases]
    assert [int(x) for x in tab["crc32"]] == [zlib.crc32(c.text) for c in cases]


def test_reader_reads_a_libdeflate_file_with_either_inflater(tmp_path):
    """bgzip linked with libdeflate: the reader's text is the same with the host decoder (HHGT_ZLIB_INFLATE=0) and with
    zlib (=1); HHGT_ZLIB_INFLATE is read once per process, so a child each"""
    if not extlibs.have_libdeflate():
        pytest.skip("libdeflate is not loadable on this box")
    from haplohyped_varawareml_amd import synth
    tab = synth.variant_table(5, 300, 700)
    text, _ = synth.render_fixed_numpy("chr5", tab, 700, seed=5)
    text = bytes(text)
    want = hashlib.sha256(text).hexdigest()
    for level in (1, 6, 12):
        p = str(tmp_path / f"l{level}.vcf.gz")
        extlibs.write_bgzf_libdeflate(p, text, level)
        code = ("import sys; sys.path.insert(0, %r)\n"
                "from haplohyped_varawareml_amd.reader import VcfReader\n"
                "import hashlib\n"
                "h = hashlib.sha256()\n"
                "with VcfReader(%r, block_bytes=1 << 20, n_threads=3) as r:\n"
                "    for b in r: h.update(bytes(b))\n"
                "print(h.hexdigest())\n") % (ROOT, p)
        for z in ("0", "1"):
            out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HHGT_ZLIB_INFLATE=z),
                                 capture_output=True, text=True, timeout=300)
            assert out.stdout.strip() == want, (level, z, out.stderr[-2000:])
