"""Hand-built LZ4 blocks and Blosc chunks for the decoder tests (tests/test_lz4_streams.py pins these helpers against
liblz4; tests/test_gpu_decode_foreign.py feeds their output to the device decoder).

  write_stream  explicit sequences (literals, offset, match length) + the final literal run -> LZ4 block bytes, every
                length-extension byte written out; `pad_to` adds one filler sequence so the block decodes to exactly n bytes
  interpret     the plain byte-by-byte decoder: decoded bytes, or None for offset 0, an offset past the bytes produced,
                truncation, or a decoded size other than n.  It does NOT apply LZ4's end-of-block rules (last 5 bytes
                literals, last match starting 12 bytes before the end), which liblz4 enforces
  frame         raw streams -> one Blosc1 or Blosc2 chunk (header, bstarts, csize words)
"""
import struct

import numpy as np

MEMCPYED, DOSHUFFLE, DOBITSHUFFLE, DONT_SPLIT = 0x2, 0x1, 0x4, 0x10
LZ4_FORMAT = 1 << 5


def _b(x):
    return x if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, np.uint8).tobytes()


def _ext(n):
    """length-extension bytes of a length whose nibble is 15: n = the length minus 15"""
    return b"\xff" * (n // 255) + bytes([n % 255])


def _seq(lit, off, ml):
    lit = bytes(lit)
    ll, mt = len(lit), ml - 4
    tok = (min(ll, 15) << 4) | min(mt, 15)
    out = bytes([tok]) + (_ext(ll - 15) if ll >= 15 else b"") + lit + struct.pack("<H", off)
    return out + (_ext(mt - 15) if mt >= 15 else b"")


def decoded_size(seqs, last=b""):
    return sum(len(lit) + ml for lit, _, ml in seqs) + len(last)


def write_stream(seqs, last=b"", pad_to=None, fill=0x3C):
    """seqs: [(literals, offset, match_len >= 4)], then the final literal-only sequence `last`.  pad_to = n: one filler
    sequence (a literal `fill` byte and an offset-1 match) goes in front of `last` so the block decodes to n bytes.
    Offsets are written as given (0 and offsets past the produced bytes included): the malformed streams come from here."""
    seqs = list(seqs)
    if pad_to is not None:
        r = pad_to - decoded_size(seqs, last)
        assert r == 0 or r >= 5, f"cannot pad {r} bytes with a sequence"
        if r:
            seqs.append((bytes([fill]), 1, r - 1))
    body = b"".join(_seq(lit, off, ml) for lit, off, ml in seqs)
    last = bytes(last)
    tail = bytes([min(len(last), 15) << 4]) + (_ext(len(last) - 15) if len(last) >= 15 else b"") + last
    return np.frombuffer(body + tail, np.uint8).copy()


def _read_len(s, ip, v):
    """length v with its extension bytes at s[ip:] -> (length, ip) or None when the extension runs past the end"""
    if v != 15:
        return v, ip
    while True:
        if ip >= len(s):
            return None
        b = s[ip]
        ip += 1
        v += b
        if b != 255:
            return v, ip


def interpret(stream, n):
    """plain LZ4 block decode of `stream` into exactly n bytes -> uint8 array, or None (see the module doc)"""
    s = _b(stream)
    out = bytearray()
    ip = 0
    while True:
        if ip >= len(s):
            return None                      # empty stream, or a stream that ends with a match
        tok = s[ip]
        ip += 1
        r = _read_len(s, ip, tok >> 4)
        if r is None:
            return None
        ll, ip = r
        if ip + ll > len(s):
            return None
        out += s[ip:ip + ll]
        ip += ll
        if ip == len(s):
            break
        if ip + 2 > len(s):
            return None
        off = s[ip] | (s[ip + 1] << 8)
        ip += 2
        if off == 0 or off > len(out):
            return None
        r = _read_len(s, ip, tok & 15)
        if r is None:
            return None
        ml, ip = r
        ml += 4
        if len(out) + ml > n:
            return None
        for _ in range(ml):                  # byte by byte: an overlapping match repeats its own output
            out.append(out[-off])
        if len(out) > n:
            return None
    if len(out) != n:
        return None
    return np.frombuffer(bytes(out), np.uint8).copy()


def frame(blocks, typesize, blocksize, nbytes, fmt=1, shuffle=True, split=True, codec=1):
    """blocks: per Blosc block, the list of its raw streams (uint8 arrays / bytes); a stream is stored with csize = its
    length.  split: the header leaves DONT_SPLIT clear, so a whole block of typesize >= 2 must hold typesize streams
    (its byte planes when shuffled); otherwise, and for the short last block, one stream.  fmt 1 = Blosc1 (16-byte
    header), 2 = Blosc2 extended header as the oracle writes it (32 bytes, shuffle as filters[5]).  codec: the format
    code of flags bits 5-7 (1 = LZ4).  -> uint8 array (cbytes = its length)"""
    nblocks = -(-nbytes // blocksize)
    assert len(blocks) == nblocks
    hl = 32 if fmt == 2 else 16
    pos = hl + 4 * nblocks
    starts, body = [], []
    for b, streams in enumerate(blocks):
        bsize = min(blocksize, nbytes - b * blocksize)
        want = typesize if split and typesize >= 2 and bsize == blocksize else 1
        assert len(streams) == want, (b, len(streams), want)
        starts.append(pos)
        for st in streams:
            st = _b(st)
            body.append(struct.pack("<I", len(st)) + st)
            pos += 4 + len(st)
    flags = (codec << 5) | (0 if split else DONT_SPLIT)
    if fmt == 2:
        hdr = bytearray(32)
        hdr[0:4] = bytes([5, 1, flags | DOSHUFFLE | DOBITSHUFFLE, typesize])
        hdr[21] = 1 if shuffle else 0
    else:
        hdr = bytearray(16)
        hdr[0:4] = bytes([2, 1, flags | (DOSHUFFLE if shuffle else 0), typesize])
    hdr[4:16] = struct.pack("<III", nbytes, blocksize, pos)
    out = bytes(hdr) + struct.pack(f"<{nblocks}I", *starts) + b"".join(body)
    assert len(out) == pos
    return np.frombuffer(out, np.uint8).copy()


def streams_of(chunk):
    """the inverse of frame() for a compressed chunk (either header format): -> (header fields, [[stream bytes]])"""
    c = _b(chunk)
    flags, ts = c[2], c[3]
    nbytes, bs, cbytes = struct.unpack("<III", c[4:16])
    hl = 32 if (flags & DOSHUFFLE and flags & DOBITSHUFFLE) else 16
    nblocks = -(-nbytes // bs)
    starts = struct.unpack(f"<{nblocks}I", c[hl:hl + 4 * nblocks])
    blocks = []
    for b in range(nblocks):
        bsize = min(bs, nbytes - b * bs)
        ns = ts if not flags & DONT_SPLIT and ts >= 2 and bsize == bs else 1
        p, sts = starts[b], []
        for _ in range(ns):
            (n,) = struct.unpack("<I", c[p:p + 4])
            sts.append(c[p + 4:p + 4 + n])
            p += 4 + n
        blocks.append(sts)
    return dict(flags=flags, typesize=ts, nbytes=nbytes, blocksize=bs, cbytes=cbytes, hl=hl), blocks


# ---- the boundary table: streams at the edges of lz4_wave_decode's fast path and of its general path -----------------
# kind "valid": a well-formed block (liblz4 decodes it to the same n bytes); "eob": well-formed but for LZ4's end-of-block
# rules (liblz4 refuses it, the interpreter decodes it); "bad": malformed (both refuse it).

LIT_LENS = list(range(17)) + [269, 270, 271] + [15 + 255 * k + r for k in (63, 64, 65) for r in (0, 7)]
MATCH_LENS = list(range(4, 21)) + [272, 273, 274, 275, 16384 + 700, 20000]
OFFSETS = list(range(1, 10)) + [13, 16, 31, 32, 33, 63, 64, 65, 127, 128, 4096]
NPOT = [o for o in range(3, 64) if o & (o - 1)]


def _rand(rng, k):
    return rng.integers(0, 256, k, dtype=np.uint8).tobytes()


def boundary_streams(n, seed=0):
    """-> [(name, stream, kind)], every stream sized for a block of n decoded bytes (cases that do not fit n are left out)"""
    rng = np.random.default_rng(seed)
    R = lambda k: _rand(rng, k)  # noqa: E731
    pre = [(R(20), 7, 9)]                                   # 29 bytes of output before the case's own sequences
    cases = []                                              # (name, seqs, last, kind)
    for L in LIT_LENS:
        cases.append((f"lit{L}", pre + [(R(L), 13, 6), (R(3), 2, 9)], R(8), "valid"))
        cases.append((f"lastlit{L}", pre + [(R(2), 29, 40)], R(L), "valid" if L >= 5 else "eob"))
    for M in MATCH_LENS:
        long = M > 1000                                     # one match of it (non-power-of-two offset), not three
        seqs = [(R(5), 5, M)] if long else [(R(5), 5, M), (R(1), 29, M), (b"", 40, M)]
        cases.append((f"ml{M}", pre + seqs, R(8), "valid"))
    for O in OFFSETS:
        cases.append((f"off{O}", [(R(max(O, 20)), O, 70), (R(2), O, 5), (b"", O, 300), (R(13), O, 19)], R(8), "valid"))
    # the largest offset a 64 KiB block can hold: the last match starts 12 bytes before the end (offset 65535 itself needs
    # a longer block; one past the produced bytes is in malformed_streams)
    cases.append(("off65524", [(R(1000), 1000, 64524), (b"", 65524, 4)], R(8), "valid"))
    # offsets that reach the block's first byte exactly: fast path (ll <= 13) and general path (ll = 14)
    cases.append(("reach0_fast", pre + [(R(5), 34, 30)], R(8), "valid"))
    cases.append(("reach0_slow", pre + [(R(14), 43, 30)], R(8), "valid"))
    # every non-power-of-two offset below 64: matches longer than a 64-byte step, and matches within the first step
    cases.append(("npot_long", [(R(64), 64, 4)] + [(R(1), o, 150 + o) for o in NPOT], R(8), "valid"))
    cases.append(("npot_short", [(R(64), 64, 4)] + [(R(1), o, min(o + 7, 64)) for o in NPOT], R(8), "valid"))
    # a run of fast-path sequences back to back, each with one match-length extension byte (e1 = 0 .. 254)
    cases.append(("e1_run", pre + [(R(k % 14), 1 + k % 29, 19 + (k * 37) % 255) for k in range(60)], R(8), "valid"))
    # end-of-block rules broken: the last match ends within the last 5 bytes / starts within the last 12 bytes
    cases.append(("eob_match_at_end", pre + [(R(3), 11, 9)], R(2), "eob"))
    cases.append(("eob_late_match", pre + [(R(3), 11, 4)], R(5), "eob"))
    out = []
    for name, seqs, last, kind in cases:
        if name.startswith("eob_"):
            if decoded_size(seqs, last) > n:
                continue
            seqs = [(R(1), 1, n - decoded_size(seqs, last) - 1)] + seqs if decoded_size(seqs, last) < n else seqs
            out.append((name, write_stream(seqs, last), kind))
            continue
        if not (decoded_size(seqs, last) == n or decoded_size(seqs, last) + 5 <= n):
            continue
        out.append((name, write_stream(seqs, last, pad_to=n), kind))
    return out


def malformed_streams(n, seed=1):
    """-> [(name, stream)]: streams that decode to something other than n bytes, or not at all"""
    rng = np.random.default_rng(seed)
    R = lambda k: _rand(rng, k)  # noqa: E731
    pre = [(R(20), 7, 9)]
    ok = lambda seqs, last=R(8), m=n: write_stream(seqs, last, pad_to=m)  # noqa: E731
    P = len(write_stream(pre)) - 1                                     # bytes of the prefix sequence
    out = [("off0", ok(pre + [(R(3), 0, 10)])),
           ("off_past", ok([(R(10), 11, 5)])),
           ("off_past_late", ok(pre + [(R(6), 36, 5)])),             # op + ll + 1 after the prefix
           ("size_n_minus_1", ok(pre, m=n - 1)),
           ("size_n_plus_1", ok(pre, m=n + 1)),
           ("ends_in_match", ok(pre, last=b"")[:-1])]                # the final (empty) literal token removed
    s = ok(pre + [(R(40), 10, 20)])
    out.append(("trunc_in_literals", s[:P + 2 + 20]))                    # token, extension byte, 20 of 40 literals
    s = ok(pre + [(R(5), 3, 10)])
    out.append(("trunc_in_offset", s[:P + 1 + 5 + 1]))                     # one byte of the offset
    s = ok(pre + [(R(5), 3, 4 + 15 + 255 * 3 + 10)])
    out.append(("trunc_in_match_ext", s[:P + 1 + 5 + 2 + 2]))              # two of the four extension bytes
    L = 15 + 255 * 70 + 3
    if L + 100 < n:
        s = ok(pre + [(R(L), 3, 10)])
        out.append(("trunc_in_literal_ext", s[:P + 1 + 66]))               # 66 of the 71 extension bytes: past one ballot
    return out
