"""Optional independent decoders that ship with the base image (NOT part of the reference, NOT part
of this repository): system liblz4 1.9.3, c-blosc 1.21 and libdeflate 1.10 (what htslib's bgzip deflates with).  Tests use them when they can be loaded
and skip otherwise; nothing in the product path touches them."""
import ctypes as C

import numpy as np


def _try(paths):
    for p in paths:
        try:
            return C.CDLL(p)
        except OSError:
            continue
    return None


_lz4 = _try(["/usr/lib/x86_64-linux-gnu/liblz4.so.1", "liblz4.so.1"])
_blosc = _try(["/opt/conda/lib/libblosc.so.1", "libblosc.so.1"])
_deflate = _try(["/lib/x86_64-linux-gnu/libdeflate.so.0", "/usr/lib/x86_64-linux-gnu/libdeflate.so.0", "libdeflate.so.0"])

if _lz4 is not None:
    _lz4.LZ4_decompress_safe.restype = C.c_int
    _lz4.LZ4_decompress_safe.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    _lz4.LZ4_compress_default.restype = C.c_int
    _lz4.LZ4_compress_default.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    _lz4.LZ4_compressBound.restype = C.c_int
    _lz4.LZ4_compressBound.argtypes = [C.c_int]
if _blosc is not None:
    _blosc.blosc_decompress.restype = C.c_int
    _blosc.blosc_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    _blosc.blosc_compress_ctx.restype = C.c_int
    _blosc.blosc_compress_ctx.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_char_p, C.c_size_t, C.c_int]
    _blosc.blosc_decompress_ctx.restype = C.c_int
    _blosc.blosc_decompress_ctx.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
if _deflate is not None:
    _deflate.libdeflate_alloc_compressor.restype = C.c_void_p
    _deflate.libdeflate_alloc_compressor.argtypes = [C.c_int]
    _deflate.libdeflate_free_compressor.restype = None
    _deflate.libdeflate_free_compressor.argtypes = [C.c_void_p]
    _deflate.libdeflate_deflate_compress.restype = C.c_size_t
    _deflate.libdeflate_deflate_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    _deflate.libdeflate_deflate_compress_bound.restype = C.c_size_t
    _deflate.libdeflate_deflate_compress_bound.argtypes = [C.c_void_p, C.c_size_t]
    _deflate.libdeflate_alloc_decompressor.restype = C.c_void_p
    _deflate.libdeflate_alloc_decompressor.argtypes = []
    _deflate.libdeflate_free_decompressor.restype = None
    _deflate.libdeflate_free_decompressor.argtypes = [C.c_void_p]
    _deflate.libdeflate_deflate_decompress.restype = C.c_int
    _deflate.libdeflate_deflate_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                       C.POINTER(C.c_size_t)]


# how often each independent leg actually ran in this session (tests/conftest.py prints it in the terminal summary, so a
# run's log says which legs the parity tests really had — a leg that is absent is otherwise a silent `if`)
used = {"liblz4": 0, "c-blosc": 0, "libdeflate": 0}


def have_lz4():
    return _lz4 is not None


def have_blosc():
    return _blosc is not None


def have_libdeflate():
    return _deflate is not None


def legs():
    """-> {name: (present, what it is)} of the independent decoders the tests use when they can be loaded"""
    from tests.test_h5file import have_h5py
    return {"liblz4": (have_lz4(), "system liblz4 (LZ4_decompress_safe on every LZ4 stream)"),
            "c-blosc": (have_blosc(), "c-blosc 1.x (blosc_decompress_ctx on Blosc-1 chunks; shuffle + header + bstarts)"),
            "libdeflate": (have_libdeflate(), "libdeflate 1.x (raw DEFLATE: bgzip's compressor, and a second inflater beside zlib)"),
            "libhdf5": (have_h5py(), "h5py / libhdf5 under /opt/conda (the .h5 container, read_direct_chunk, filter pipeline)")}


def lz4_decompress(comp, nbytes):
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    out = np.empty(max(nbytes, 1), np.uint8)
    used["liblz4"] += 1
    n = _lz4.LZ4_decompress_safe(comp.ctypes.data, out.ctypes.data, comp.size, nbytes)
    if n < 0:
        raise RuntimeError(f"LZ4_decompress_safe rc={n}")
    return out[:n]


def lz4_compress(buf):
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    cap = _lz4.LZ4_compressBound(buf.size)
    out = np.empty(cap, np.uint8)
    n = _lz4.LZ4_compress_default(buf.ctypes.data, out.ctypes.data, buf.size, cap)
    assert n > 0
    return out[:n].copy()


def blosc1_decompress(chunk, nbytes):
    chunk = np.ascontiguousarray(chunk, dtype=np.uint8)
    out = np.empty(max(nbytes, 1), np.uint8)
    used["c-blosc"] += 1
    n = _blosc.blosc_decompress_ctx(chunk.ctypes.data, out.ctypes.data, nbytes, 1)
    if n < 0:
        raise RuntimeError(f"blosc_decompress_ctx rc={n}")
    return out[:n]


def blosc1_compress(buf, typesize, blocksize=0, clevel=5, shuffle=1, cname=b"lz4", tight=False):
    """tight: a destination of nbytes + 16 (BLOSC_MAX_OVERHEAD), c-blosc's own sizing, under which it stores
    incompressible input as a memcpyed chunk"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    out = np.empty(buf.size + 16 + (0 if tight else 4096), np.uint8)
    n = _blosc.blosc_compress_ctx(clevel, shuffle, typesize, buf.size, buf.ctypes.data, out.ctypes.data, out.size,
                                  cname, blocksize, 1)
    assert n > 0
    return out[:n].copy()


if _lz4 is not None:
    _lz4.LZ4_compress_HC.restype = C.c_int
    _lz4.LZ4_compress_HC.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    _lz4.LZ4_compress_fast.restype = C.c_int
    _lz4.LZ4_compress_fast.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
if _blosc is not None:
    _blosc.blosc_set_splitmode.restype = None
    _blosc.blosc_set_splitmode.argtypes = [C.c_int]

# c-blosc 1.x split modes (blosc.h)
BLOSC_ALWAYS_SPLIT, BLOSC_NEVER_SPLIT, BLOSC_AUTO_SPLIT, BLOSC_FORWARD_COMPAT_SPLIT = 1, 2, 3, 4


def _lz4_call(fn, buf, arg):
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    cap = _lz4.LZ4_compressBound(buf.size)
    out = np.empty(max(cap, 1), np.uint8)
    n = fn(buf.ctypes.data, out.ctypes.data, buf.size, cap, arg)
    assert n > 0
    return out[:n].copy()


def lz4_compress_hc(buf, level):
    """liblz4's LZ4HC at `level` (1..12): the block coder behind c-blosc's lz4hc"""
    return _lz4_call(_lz4.LZ4_compress_HC, buf, level)


def lz4_compress_fast(buf, accel):
    """liblz4's fast coder with acceleration `accel` (1 = LZ4_compress_default)"""
    return _lz4_call(_lz4.LZ4_compress_fast, buf, accel)


class splitmode:
    """with splitmode(BLOSC_NEVER_SPLIT): c-blosc's block splitting for the compressions inside; process-global state, so
    FORWARD_COMPAT (c-blosc 1.21's default, which other tests rely on) is restored on the way out, also after an error"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        _blosc.blosc_set_splitmode(self.mode)
        return self

    def __exit__(self, *exc):
        _blosc.blosc_set_splitmode(BLOSC_FORWARD_COMPAT_SPLIT)
        return False


# ---- libdeflate (raw DEFLATE, RFC 1951) ----
def deflate_compress(buf, level):
    """libdeflate at `level` (0..12; 0 = stored blocks only) -> raw DEFLATE bytes"""
    buf = bytes(buf)
    c = _deflate.libdeflate_alloc_compressor(int(level))
    assert c, level
    try:
        cap = _deflate.libdeflate_deflate_compress_bound(c, len(buf))
        out = C.create_string_buffer(cap)
        n = _deflate.libdeflate_deflate_compress(c, buf, len(buf), out, cap)
        assert n > 0
        return out.raw[:n]
    finally:
        _deflate.libdeflate_free_compressor(c)


def deflate_decompress(comp, max_out=1 << 18):
    """libdeflate_deflate_decompress -> (result, bytes): result 0 success, 1 bad data, 2 short output, 3 insufficient
    space (libdeflate's enum); the bytes are those written up to the verdict (meaningful on success only)"""
    comp = bytes(comp)
    used["libdeflate"] += 1
    d = _deflate.libdeflate_alloc_decompressor()
    assert d
    try:
        out = C.create_string_buffer(max(max_out, 1))
        n = C.c_size_t(0)
        r = _deflate.libdeflate_deflate_decompress(d, comp, len(comp), out, max_out, C.byref(n))
        return r, out.raw[:n.value] if r == 0 else b""
    finally:
        _deflate.libdeflate_free_decompressor(d)


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_libdeflate(data, level=6, block_size=0xFF00):
    """BGZF bytes as htslib's bgzip writes them when it links libdeflate: 0xFF00 input bytes per member, each deflated by
    libdeflate (stored instead, as bgzf.c does, if the deflated member would not fit 64 KiB), then the 28-byte EOF member"""
    import struct
    import zlib
    data = bytes(data)
    out = []
    for i in range(0, len(data), block_size):
        chunk = data[i:i + block_size]
        comp = deflate_compress(chunk, level)
        if len(comp) + 26 > 65536:
            comp = deflate_compress(chunk, 0)
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp +
                   struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
    return b"".join(out) + BGZF_EOF


def write_bgzf_libdeflate(path, data, level=6):
    with open(path, "wb") as f:
        f.write(bgzf_libdeflate(data, level))
