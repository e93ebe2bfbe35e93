"""CPU: the hand-built LZ4 streams and Blosc framing of tests/lz4_streams.py against liblz4 and c-blosc, so that they
can judge the device decoder (tests/test_gpu_decode_foreign.py).  Every boundary stream liblz4 accepts decodes to the
same bytes in the plain interpreter; every stream the interpreter refuses, liblz4 refuses too."""
import numpy as np
import pytest

from oracle import oracle
from tests import extlibs
from tests import lz4_streams as L

need_lz4 = pytest.mark.skipif(not extlibs.have_lz4(), reason="liblz4 not loadable (independent leg absent)")
need_blosc = pytest.mark.skipif(not extlibs.have_blosc(), reason="c-blosc not loadable (independent leg absent)")


def liblz4(stream, n):
    """LZ4_decompress_safe into exactly n bytes -> the bytes, or None when it fails or decodes to another size"""
    try:
        out = extlibs.lz4_decompress(stream, n)
    except RuntimeError:
        return None
    return out if out.size == n else None


@need_lz4
@pytest.mark.parametrize("n", [16384, 32768, 65536])
def test_boundary_streams_match_liblz4(n):
    table = L.boundary_streams(n)
    kinds = {k: sum(1 for _, _, kk in table if kk == k) for k in ("valid", "eob")}
    assert kinds["valid"] > 60 and kinds["eob"] >= 5
    for name, s, kind in table:
        mine, ref = L.interpret(s, n), liblz4(s, n)
        assert mine is not None, name
        if kind == "valid":
            assert ref is not None and np.array_equal(mine, ref), name
        else:
            assert ref is None, name           # liblz4 enforces the end-of-block rules the interpreter leaves out
    names = {name for name, _, _ in table}
    assert {"lit0", "lit16", "lit16080", "ml273", "off1", "npot_long", "e1_run"} <= names
    assert ("ml20000" in names) == (n >= 32768) and ("off65524" in names) == (n == 65536)


@need_lz4
@pytest.mark.parametrize("n", [4096, 32768])
def test_malformed_streams_refused_by_both(n):
    table = L.malformed_streams(n)
    assert len(table) >= 9
    for name, s in table:
        assert L.interpret(s, n) is None, name
        if name == "off0":
            # the LZ4 block format makes offset 0 invalid, but LZ4_decompress_safe 1.9.3 does not check it (it copies
            # from the write head): pinned here so that the interpreter, not liblz4, stays the judge of this case
            assert liblz4(s, n) is not None
            continue
        assert liblz4(s, n) is None, name


def test_writer_encodes_every_extension_byte():
    s = L.write_stream([(b"\x01" * (15 + 255 * 64), 1, 4 + 15 + 255 * 2 + 1)], b"\x02" * 20)
    assert s[0] == 0xFF and np.all(s[1:65] == 255) and s[65] == 0          # 64 bytes of 255, then 0
    lit_end = 66 + 15 + 255 * 64
    assert list(s[lit_end:lit_end + 2]) == [1, 0] and list(s[lit_end + 2:lit_end + 5]) == [255, 255, 1]
    assert list(s[lit_end + 5:lit_end + 7]) == [0xF0, 5]
    n = L.decoded_size([(b"\x01" * (15 + 255 * 64), 1, 4 + 15 + 255 * 2 + 1)], b"\x02" * 20)
    out = L.interpret(s, n)
    assert out is not None and out.size == n and np.all(out[:-20] == 1) and np.all(out[-20:] == 2)
    assert L.interpret(s, n - 1) is None and L.interpret(s, n + 1) is None
    assert L.decoded_size([], L.interpret(L.write_stream([], b"", pad_to=100), 100)) == 100


@pytest.mark.parametrize("fmt", [oracle.BLOSC1, oracle.BLOSC2])
@pytest.mark.parametrize("typesize,blocksize,nbytes", [(2, 8192, 3 * 8192 + 1400), (1, 4096, 2 * 4096 + 77),
                                                       (4, 2048, 2048 * 3), (2, 128, 1000)])
def test_framer_reproduces_oracle_chunks(fmt, typesize, blocksize, nbytes):
    """the framer re-frames the oracle's streams into the oracle's own chunk, byte for byte (both header formats)"""
    rng = np.random.default_rng(typesize + blocksize)
    data = (rng.random(nbytes) < 0.07).astype(np.uint8)
    ck = oracle.blosc_compress(data, typesize, blocksize, fmt)
    hdr, blocks = L.streams_of(ck)
    assert not hdr["flags"] & L.MEMCPYED
    again = L.frame(blocks, typesize, hdr["blocksize"], nbytes, fmt=fmt, shuffle=bool(hdr["flags"] & 1 if fmt == 1
                                                                                     else ck[21]),
                    split=not hdr["flags"] & L.DONT_SPLIT)
    assert np.array_equal(again, ck)


@need_blosc
@need_lz4
def test_framed_liblz4_streams_decode_in_cblosc():
    """liblz4 HC / fast planes framed as Blosc1 split chunks: c-blosc decodes them to the input"""
    rng = np.random.default_rng(3)
    bs, nbytes = 8192, 3 * 8192 + 1400
    data = (rng.random(nbytes) < 0.07).astype(np.uint8)
    for comp in [lambda b: extlibs.lz4_compress_hc(b, 9), lambda b: extlibs.lz4_compress_fast(b, 7)]:
        blocks = []
        for b in range(-(-nbytes // bs)):
            blk = data[b * bs:(b + 1) * bs]
            if blk.size == bs:
                sh = oracle.shuffle(blk, 2)
                blocks.append([comp(sh[:bs // 2]), comp(sh[bs // 2:])])
            else:
                blocks.append([comp(oracle.shuffle(blk, 2))])
        ck = L.frame(blocks, 2, bs, nbytes)
        assert np.array_equal(extlibs.blosc1_decompress(ck, nbytes), data)


@need_blosc
def test_splitmode_is_restored():
    data = (np.random.default_rng(1).random(1 << 15) < 0.05).astype(np.uint8)
    with pytest.raises(ZeroDivisionError):
        with extlibs.splitmode(extlibs.BLOSC_NEVER_SPLIT):
            assert extlibs.blosc1_compress(data, 2, 8192, 5, 1, b"lz4hc")[2] & L.DONT_SPLIT
            1 / 0
    assert not extlibs.blosc1_compress(data, 2, 8192, 5, 1, b"lz4hc")[2] & L.DONT_SPLIT
