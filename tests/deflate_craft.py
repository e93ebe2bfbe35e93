"""Test-only, bit-level DEFLATE (RFC 1951) writer and a corpus of crafted streams for the two BGZF inflaters
(csrc/inflate.hip on the device, csrc/fast_inflate.h on the host).

zlib and libdeflate write only a few of the stream shapes RFC 1951 allows, and never an invalid one.  The writer here
takes every choice a compressor makes as an explicit argument: the code lengths of each alphabet (complete,
incomplete or over-subscribed), HLIT / HDIST / HCLEN, how the code lengths are run-length coded (16 / 17 / 18 and their
repeat counts, runs across the literal/length -> distance boundary), and the symbols themselves (literals, matches,
or raw symbol + extra-bit pairs, so that symbols no compressor emits can be written).

`corpus()` returns named cases.  A valid case carries the text its stream must inflate to (tracked by the writer from
the symbols it wrote, not by decoding); an invalid case carries one defect and the status the device inflater must
report for it (include/hhgt.h: 1 block type, 2 stored block, 3 code table, 4 invalid code, 5 distance,
6 output overrun, 8 size != ISIZE; ANY = some non-zero status) and, where zlib rejects the stream with a message of its
own, that message.  zlib is the arbiter of what is valid (tests/test_deflate_craft.py checks every case against it).
"""
import struct
import zlib
from collections import namedtuple

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
EOB = 256

# device statuses (include/hhgt.h); ANY: a truncated stream may be caught at several places
OK, BAD_BLOCK_TYPE, BAD_STORED, BAD_TABLE, BAD_CODE, BAD_DISTANCE, OUTPUT_OVERRUN, INPUT_OVERRUN, SIZE_MISMATCH = range(9)
ANY = -1


# ---------------------------------------------------------------------------------------------- bits and codes
class BitWriter:
    """LSB-first bit packer (RFC 1951 3.1.1): whole bytes go to a bytearray, at most 7 bits wait in `acc`"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.nacc = 0

    def bits(self, v, n):
        assert 0 <= v < (1 << n) or (n == 0 and v == 0), (v, n)
        self.acc |= v << self.nacc
        self.nacc += n
        while self.nacc >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.nacc -= 8

    def code(self, c, n):
        """a Huffman code: packed starting with its most significant bit"""
        self.bits(int(format(c, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.nacc:
            self.out.append(self.acc)
            self.acc = self.nacc = 0

    def raw(self, data):
        assert self.nacc == 0
        self.out += data

    @property
    def nbits(self):
        return 8 * len(self.out) + self.nacc

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.nacc else b"")


def canonical(lens):
    """symbol -> (code, length) of the canonical code with these lengths (RFC 1951 3.2.2).  Over-subscribed sets
    get codes too (wrapped to their length), so that invalid tables can still be used to write a stream."""
    count = [0] * 16
    for l in lens:
        if l:
            count[l] += 1
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return out


def kraft(lens):
    """sum of 2^(15 - l) over the used codes: 2^15 for a complete code"""
    return sum(1 << (15 - l) for l in lens if l)


def huffman_lengths(freqs, maxlen):
    """length-limited Huffman code lengths (package-merge); a single used symbol gets a second, unused one beside it
    so that the code stays complete"""
    used = [(f, s) for s, f in enumerate(freqs) if f > 0]
    lens = [0] * len(freqs)
    if not used:
        return lens
    if len(used) == 1:
        s = used[0][1]
        lens[s] = 1
        lens[1 if s == 0 else 0] = 1
        return lens
    leaves = sorted((f, [s]) for f, s in used)
    cur = list(leaves)
    for _ in range(maxlen - 1):
        pk = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + pk, key=lambda x: x[0])
    for _, ss in cur[:2 * len(used) - 2]:
        for s in ss:
            lens[s] += 1
    assert kraft(lens) == 1 << 15 and max(lens) <= maxlen
    return lens


def len_code(length, sym=None):
    """-> (symbol, extra value, extra bits) of a match length; sym forces the length symbol (e.g. 284 for 258)"""
    if sym is None:
        sym = 285 if length == 258 else 257 + max(i for i in range(28) if LEN_BASE[i] <= length)
    i = sym - 257
    extra = length - LEN_BASE[i]
    assert 0 <= extra < (1 << LEN_EXTRA[i]) or (extra == 0 and LEN_EXTRA[i] == 0), (length, sym)
    return sym, extra, LEN_EXTRA[i]


def dist_code(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, dist - DIST_BASE[s], DIST_EXTRA[s]


# ---------------------------------------------------------------------------------------------- symbols
Match = namedtuple("Match", "length dist lsym")
Match.__new__.__defaults__ = (None,)
Sym = namedtuple("Sym", "sym extra")          # raw literal/length symbol (+ its extra bits, if any, from LEN_EXTRA)
Sym.__new__.__defaults__ = (0,)
DSym = namedtuple("DSym", "sym extra")        # raw distance symbol (+ extra bits from DIST_EXTRA; 30/31 take none)
DSym.__new__.__defaults__ = (0,)


def _items(seq):
    for x in seq:
        if isinstance(x, (bytes, bytearray)):
            yield from x
        else:
            yield x


def ll_freqs(seq):
    """literal/length symbol counts of a sequence, EOB included"""
    f = [0] * 288
    for x in _items(seq):
        if isinstance(x, int):
            f[x] += 1
        elif isinstance(x, Match):
            f[len_code(x.length, x.lsym)[0]] += 1
        elif isinstance(x, Sym):
            f[x.sym] += 1
    f[EOB] += 1
    return f


def d_freqs(seq):
    f = [0] * 32
    for x in _items(seq):
        if isinstance(x, Match):
            f[dist_code(x.dist)[0]] += 1
        elif isinstance(x, DSym):
            f[x.sym] += 1
    return f


# ---------------------------------------------------------------------------------------------- stream
class Stream:
    """One DEFLATE stream, block by block.  `text` follows what a correct inflater must produce from the symbols
    written (literals appended, matches copied byte by byte); `text_ok` turns False once a match reaches before the
    start (the text is then meaningless)."""

    def __init__(self):
        self.w = BitWriter()
        self.text = bytearray()
        self.text_ok = True

    def getvalue(self):
        return self.w.getvalue()

    def _header(self, final, btype):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def _copy(self, length, dist):
        if dist > len(self.text) or dist < 1:
            self.text_ok = False
            return
        for _ in range(length):
            self.text.append(self.text[-dist])

    def stored(self, data, final=False, len_=None, nlen=None):
        self._header(final, 0)
        self.w.align()
        n = len(data) if len_ is None else len_
        self.w.bits(n, 16)
        self.w.bits((~n & 0xFFFF) if nlen is None else nlen, 16)
        self.w.raw(data)
        self.text += data
        return self

    def _symbols(self, seq, llc, dc, eob):
        w = self.w
        pend = None  # length of a raw length symbol, waiting for its distance
        for x in list(_items(seq)) + ([EOB] if eob else []):
            if isinstance(x, int):
                x = Sym(x)
            if isinstance(x, Match):
                s, e, n = len_code(x.length, x.lsym)
                w.code(*llc[s])
                w.bits(e, n)
                s, e, n = dist_code(x.dist)
                w.code(*dc[s])
                w.bits(e, n)
                self._copy(x.length, x.dist)
            elif isinstance(x, Sym):
                w.code(*llc[x.sym])
                if x.sym < 256:
                    self.text.append(x.sym)
                elif 257 <= x.sym <= 285:
                    n = LEN_EXTRA[x.sym - 257]
                    w.bits(x.extra, n)
                    pend = LEN_BASE[x.sym - 257] + x.extra
            elif isinstance(x, DSym):
                w.code(*dc[x.sym])
                if x.sym < 30:
                    w.bits(x.extra, DIST_EXTRA[x.sym])
                    if pend is not None:
                        self._copy(pend, DIST_BASE[x.sym] + x.extra)
                else:
                    self.text_ok = False
                pend = None
            else:
                raise TypeError(x)

    def fixed(self, seq, final=False, eob=True):
        self._header(final, 1)
        self._symbols(seq, canonical(FIXED_LL), canonical(FIXED_D), eob)
        return self

    def dynamic(self, seq, final=False, ll=None, d=None, hlit=None, hdist=None, ops=None, at=None, cl=None,
                hclen=None, eob=True):
        """ll / d: code lengths (default: Huffman over the symbols of seq, complete; distances all zero when seq has no
        match).  hlit / hdist: the counts written (257 + HLIT, 1 + HDIST; up to 288 / 32, i.e. also invalid ones).
        ops: the code-length sequence as written, ints 0..15 and (16|17|18, repeat) (default: run-length coding of
        ll[:hlit] + d[:hdist], with the ops of `at` = {position: op} forced where they start).
        cl: the 19 code-length-code lengths by symbol (default: Huffman over ops, at most 7 bits).  hclen: number of
        them written (4..19, in CL_ORDER; default: as few as cover every non-zero one)."""
        if ll is None:
            ll = huffman_lengths(ll_freqs(seq)[:286], 15)
        ll = list(ll) + [0] * (288 - len(ll))
        if d is None:
            df = d_freqs(seq)
            d = huffman_lengths(df[:30], 15) if any(df) else [0]
        d = list(d) + [0] * (32 - len(d))
        if hlit is None:
            hlit = max(257, max(s for s in range(288) if ll[s]) + 1)
        if hdist is None:
            hdist = max([1] + [s + 1 for s in range(32) if d[s]])
        if ops is None:
            ops = rle(ll[:hlit] + d[:hdist], at or {})
        if cl is None:
            f = [0] * 19
            for o in ops:
                f[o if isinstance(o, int) else o[0]] += 1
            cl = huffman_lengths(f, 7)
        if hclen is None:
            hclen = max([4] + [i + 1 for i in range(19) if cl[CL_ORDER[i]]])
        w = self.w
        self._header(final, 2)
        w.bits(hlit - 257, 5)
        w.bits(hdist - 1, 5)
        w.bits(hclen - 4, 4)
        for i in range(hclen):
            w.bits(cl[CL_ORDER[i]], 3)
        clc = canonical(cl)
        for o in ops:
            s, rep = (o, None) if isinstance(o, int) else o
            w.code(*clc[s])
            if s == 16:
                w.bits(rep - 3, 2)
            elif s == 17:
                w.bits(rep - 3, 3)
            elif s == 18:
                w.bits(rep - 11, 7)
        self._symbols(seq, canonical(ll), canonical(d), eob)
        return self


def expand(ops):
    """the code lengths a code-length sequence stands for (a 16 in first place repeats a 0 here; it is invalid)"""
    out = []
    for o in ops:
        if isinstance(o, int):
            out.append(o)
        else:
            s, rep = o
            out += [out[-1] if (s == 16 and out) else 0] * rep
    return out


def rle(lens, at):
    """run-length code a code-length sequence as zlib does, within runs and across the boundary of the two alphabets
    alike; at = {position: op} forces op where it starts (it must stand for exactly the lengths there)"""
    ops, i, n = [], 0, len(lens)
    while i < n:
        if i in at:
            s, rep = at[i]
            want = lens[i - 1] if s == 16 else 0
            assert i + rep <= n and all(l == want for l in lens[i:i + rep]) and (s != 16 or i > 0), (i, at[i])
            ops.append((s, rep))
            i += rep
            continue
        v, j = lens[i], i
        while j < n and lens[j] == v and (j == i or j not in at):
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                ops.append((18, r))
                run -= r
            if run >= 3:
                ops.append((17, run))
                run = 0
            ops += [0] * run
        else:
            ops.append(v)
            run -= 1
            while run >= 3:
                r = min(run, 6)
                ops.append((16, r))
                run -= r
            ops += [v] * run
        i = j
    assert expand(ops) == list(lens)
    return ops


# ---------------------------------------------------------------------------------------------- BGZF
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_member(payload, text, isize=None):
    """one BGZF member (RFC 1952 + the "BC" extra subfield) around a raw DEFLATE payload; CRC-32 and ISIZE are those of
    the INTENDED text (isize overrides the size)"""
    assert len(payload) + 26 <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(payload) + 25) + payload +
            struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text) if isize is None else isize))


# ---------------------------------------------------------------------------------------------- corpus
Case = namedtuple("Case", "name payload text status zmsg isize")




def _case(name, st, status=OK, zmsg=None, isize=None, trail=b""):
    if status == OK:
        assert st.text_ok, name
    text = bytes(st.text)
    return Case(name, st.getvalue() + trail, text, status, zmsg, len(text) if isize is None else isize)


def _text(n, seed, alphabet=b"ACGT\t|01.\n"):
    import random
    r = random.Random(seed)
    return bytes(r.choice(alphabet) for _ in range(n))


def _rand(n, seed):
    import random
    return random.Random(seed).randbytes(n)


def _lens(n, used):
    """n code lengths, `used` = {symbol: length}, the rest 0"""
    out = [0] * n
    for s, l in used.items():
        out[s] = l
    return out


def _fill(used, free):
    """complete a literal/length code: the code space `used` leaves goes to the symbols of `free`, largest piece first"""
    used = dict(used)
    left = (1 << 15) - kraft(used.values())
    free = [s for s in free if s not in used]
    while left:
        l = 16 - left.bit_length()
        used[free.pop(0)] = l
        left -= 1 << (15 - l)
    return used


def _length_matches(used, dist):
    """one match per length symbol of `used`, at its smallest length"""
    return [Match(LEN_BASE[s - 257], dist) for s in sorted(used) if 257 <= s <= 285]


def valid_cases():
    cs = []

    # -- codes of length 15 in both alphabets, used in the data (EOB included): lengths 1..13 plus four of 15
    ll = _lens(288, {s: k + 1 for k, s in enumerate(b"ABCDEFGHIJKLM")} | {ord("N"): 15, EOB: 15, 257: 15, 258: 15})
    d = _lens(30, {k: k + 1 for k in range(13)} | {13: 15, 14: 15, 15: 15, 16: 15})
    seq = [_text(400, 1, b"ABCDEFGHIJKLMN"), Match(3, 100), Match(4, 150), Match(3, 200), Match(4, 300), b"N",
           Match(3, 1), Match(4, 60)]
    cs.append(_case("codes_of_length_15", Stream().dynamic(seq, final=True, ll=ll, d=d)))

    # -- code-length codes: one with 7-bit codes, one that uses all 19 symbols; all 19 lengths written (HCLEN 19).
    # The literal/length code has every length 1..15; 16 / 17 / 18 repeat zeros, a 16 right after a 17.
    ll = _lens(288, {s: k + 1 for k, s in enumerate(b"abcdefghijklmn")} | {ord("o"): 15, EOB: 15})
    d = _lens(30, {0: 1, 3: 1})
    seq = [_text(200, 3, b"abcdefghijklmno")]
    lens = ll[:262] + d
    ops = rle(lens, {112: (18, 11), 123: (16, 3), 126: (17, 3), 129: (16, 4)})
    f = [0] * 19
    for o in ops:
        f[o if isinstance(o, int) else o[0]] += 1
    assert all(f)
    cl7 = huffman_lengths([x * 4 ** k for k, x in enumerate(f)], 7)
    assert max(cl7) == 7
    cs.append(_case("cl_code_7_bits_hclen_19", Stream().dynamic(seq, final=True, ll=ll, d=d, hlit=262, hdist=30,
                                                                 ops=ops, cl=cl7, hclen=19)))
    cs.append(_case("cl_code_all_19_symbols", Stream().dynamic(seq, final=True, ll=ll, d=d, hlit=262, hdist=30,
                                                                ops=ops, cl=[4] * 13 + [5] * 6, hclen=19)))

    def runs(name, ll_used, d_used, hlit, hdist, at, seq):
        ll, d = _lens(288, ll_used), _lens(32, d_used)
        assert kraft(ll) == kraft(d) == 1 << 15, name
        cs.append(_case(name, Stream().dynamic(seq, final=True, ll=ll, d=d, hlit=hlit, hdist=hdist,
                                               ops=rle(ll[:hlit] + d[:hdist], at))))

    # -- 18 x 138 (literals 40..177 unused), and an 18 across the literal/length -> distance boundary
    u = _fill({s: 9 for s in list(range(0, 40)) + list(range(178, 256)) + [EOB]}, range(257, 286))
    top = max(u)
    seq = [bytes(range(0, 40)) * 3, bytes(range(178, 256)) * 2] + _length_matches(u, 4) + [Match(3, 5), Match(4, 7)]
    runs("run_18x138_and_18_across", u, {3: 1, 4: 2, 5: 2}, top + 12, 6, {40: (18, 138), top + 1: (18, 14)}, seq)
    # -- 17 x 10 across: the last three literal/length lengths and the first seven distance lengths are 0
    u = _fill({s: 9 for s in list(range(256)) + [EOB]}, range(257, 286))
    top = max(u)
    seq = [_text(500, 5)] + _length_matches(u, 13) + [Match(4, 17), Match(5, 25), Match(6, 32)]
    runs("run_17x10_across", u, {7: 1, 8: 2, 9: 2}, top + 4, 10, {top + 1: (17, 10)}, seq)
    # -- 16 across: the literal/length code ends in three 5-bit lengths, the distance code starts with 5-bit ones
    u = _fill({s: 9 for s in range(240)} | {s: 8 for s in range(240, 256)} | {EOB: 8, 283: 5, 284: 5, 285: 5},
              range(257, 283))
    dl = {k: 5 for k in range(28)} | {28: 4, 29: 4}
    seq = [_text(700, 6), Match(258, 1), Match(200, 30), Match(258, 700)] + _length_matches(u, 9) + \
          [Match(3 + k % 6, DIST_BASE[k]) for k in range(20)] + [Match(230, 5)]
    runs("run_16x6_across", u, dl, 286, 30, {284: (16, 6)}, seq)
    runs("run_16x3_at_the_boundary", u, dl, 286, 30, {286: (16, 3)}, seq)
    # -- a 16 right after an 18 and right after a 17 (it repeats the 0 the run wrote)
    u = _fill({s: 9 for s in list(range(0, 60)) + list(range(100, 256)) + [EOB]}, range(257, 286))
    seq = [bytes(range(0, 60)) + bytes(range(100, 256)), _text(100, 7, bytes(range(100, 120)))] + \
          _length_matches(u, 4) + [Match(3, 1), Match(3, 2), Match(3, 3), Match(3, 4)]
    dl = {0: 1, 1: 2, 2: 3, 3: 3}
    runs("run_16_after_18", u, dl, max(u) + 1, 4, {60: (18, 20), 80: (16, 6), 86: (16, 6), 92: (17, 8)}, seq)
    runs("run_16_after_17", u, dl, max(u) + 1, 4, {60: (17, 10), 70: (16, 3), 73: (18, 27)}, seq)

    # -- HLIT 257, HDIST 1 with length 0: literals only
    seq = [_text(500, 8, bytes(range(32, 127)))]
    cs.append(_case("hlit_257_hdist_1_literals_only", Stream().dynamic(seq, final=True, d=[0], hlit=257, hdist=1)))

    # -- HLIT 286 and HDIST 30, every symbol of both alphabets used (lengths at their largest extra values)
    ll = [8] * 226 + [9] * 60
    d = [4] * 2 + [5] * 28
    seq = [bytes(range(256)), Match(258, 1)]
    while 256 + 258 * (len(seq) - 1) < 32768:
        seq.append(Match(258, 256))
    seq += [Match(LEN_BASE[i] + (1 << LEN_EXTRA[i]) - 1, 1 + i % 7) for i in range(29)]
    seq += [Match(3 + k, DIST_BASE[k] + (1 << DIST_EXTRA[k]) - 1) for k in range(30)]
    cs.append(_case("hlit_286_hdist_30_all_used", Stream().dynamic(seq, final=True, ll=ll, d=d, hlit=286, hdist=30)))

    # -- one distance code, of length 1 (its code is '0'); HDIST 6
    seq = [_text(64, 9), Match(20, 7), b"xy", Match(40, 8), Match(258, 7)]
    cs.append(_case("single_distance_code_of_length_1",
                    Stream().dynamic(seq, final=True, d=[0, 0, 0, 0, 0, 1], hdist=6)))

    # -- a literal/length code that holds only EOB, of length 1 (an empty block); a fixed block behind it
    st = Stream().dynamic([], ll=_lens(257, {EOB: 1}), d=[0], hlit=257, hdist=1)
    st.fixed([b"after the empty block"], final=True)
    cs.append(_case("literal_length_code_only_eob", st))

    # -- every distance code at its smallest and its largest extra value (up to 32768)
    seq = [_rand(32768, 10)]
    for k in range(30):
        seq += [Match(3, DIST_BASE[k]), Match(4, DIST_BASE[k] + (1 << DIST_EXTRA[k]) - 1)]
    cs.append(_case("every_distance_smallest_and_largest", Stream().dynamic(seq, final=True)))
    cs.append(_case("every_distance_fixed_block", Stream().fixed(seq, final=True)))

    # -- distances 1..64 with length 258; distances equal to the output so far
    seq = [_rand(64, 11)]
    for dist in range(1, 65):
        seq += [Match(258, dist), bytes([dist])]
    cs.append(_case("length_258_at_distances_1_to_64", Stream().dynamic(seq, final=True)))
    seq = [b"0|0\t1|0\t", Match(8, 8), Match(16, 16), Match(32, 32), Match(64, 64), Match(128, 128)]
    cs.append(_case("distance_equal_to_output_so_far", Stream().fixed(seq, final=True)))

    # -- length 258 via code 285 and via 284 + 31 extra bits
    seq = [b"abc", Match(258, 3), Match(258, 3, lsym=284), Match(258, 1, lsym=284), Match(258, 1)]
    cs.append(_case("length_258_via_285_and_284", Stream().fixed(seq, final=True)))
    cs.append(_case("length_258_via_285_and_284_dynamic", Stream().dynamic(seq, final=True)))

    # -- stored blocks: LEN 0, LEN 65535 (too long for a BGZF member; the device inflater takes it), behind a Huffman
    # block at each of the 8 bit phases, several empty ones in a row
    cs.append(_case("stored_len_0", Stream().stored(b"", final=True)))
    cs.append(_case("stored_len_65535", Stream().stored(_rand(65535, 12), final=True)))
    for phase in range(8):
        st = Stream()
        st.fixed([b"\x90" * ((phase - 2) % 8), b"x"])      # 3 + 9 k + 8 + 7 bits
        assert st.w.nbits % 8 == phase
        st.stored(_rand(100 + phase, 13 + phase))
        st.fixed([b"tail"], final=True)
        cs.append(_case("stored_after_huffman_at_bit_%d" % phase, st))
    st = Stream()
    for _ in range(5):
        st.stored(b"")
    st.stored(b"data after five empty stored blocks")
    st.stored(b"", final=True)
    cs.append(_case("empty_stored_blocks_in_a_row", st))

    # -- hundreds of tiny fixed blocks in one member
    st = Stream()
    for k in range(400):
        st.fixed([bytes([65 + k % 26])] + ([Match(3, 1)] if k % 3 == 0 else []) + ([] if k % 5 else [b"\n"]))
    st.fixed([], final=True)
    cs.append(_case("four_hundred_tiny_fixed_blocks", st))

    # -- dynamic (286 symbols) -> fixed -> stored -> dynamic (four 2-bit codes): no part of an earlier table may remain
    st = Stream()
    st.dynamic([bytes(range(256)), Match(258, 256)] + [Match(LEN_BASE[i], 1 + i % 9) for i in range(29)],
               ll=[8] * 226 + [9] * 60)
    st.fixed([b"fixed", Match(5, 5)])
    st.stored(b"stored")
    st.dynamic([b"zyzyx", b"xx"], ll=_lens(257, {ord("x"): 2, ord("y"): 2, ord("z"): 2, EOB: 2}), d=[0], hlit=257,
               hdist=1, final=True)
    cs.append(_case("dynamic_fixed_stored_dynamic_shrinking_tables", st))
    st = Stream()
    st.dynamic([_text(3000, 14), Match(100, 1000), Match(30, 2)])
    st.dynamic([b"qq", Match(3, 1)], ll=_lens(258, {ord("q"): 1, EOB: 2, 257: 2}), d=[1, 1], final=True)
    cs.append(_case("dynamic_then_one_and_two_bit_dynamic", st))

    # -- trailing bytes after the final block, inside the payload
    cs.append(_case("trailing_bytes_after_final_block", Stream().fixed([b"trailing"], final=True),
                    trail=b"\xde\xad\xbe\xef\x00\xff\x12"))

    # -- members of 0, 1 and 65536 bytes
    cs.append(_case("member_of_0_bytes", Stream().fixed([], final=True)))
    cs.append(_case("member_of_0_bytes_dynamic", Stream().dynamic([], final=True)))
    cs.append(_case("member_of_1_byte", Stream().fixed([b"\n"], final=True)))
    n = 1 + 254 * 258
    seq = [b"a"] + [Match(258, 1)] * 254 + [Match(65536 - n, 1)]
    cs.append(_case("member_of_65536_bytes", Stream().dynamic(seq, final=True)))
    st = Stream().stored(_rand(65000, 15))
    st.fixed([Match(258, 32768), Match(258, 30000), Match(20, 1)], final=True)
    cs.append(_case("member_of_65536_bytes_stored_then_matches", st))
    return cs


def invalid_cases():
    cs = []
    ok_seq = [b"0|0\t0|1\t", Match(16, 8), b"\n"]
    ll8 = [8] * 257         # a literal/length table that the code-length cases never get to

    # BTYPE 3
    st = Stream()
    st._header(True, 3)
    st.w.bits(0, 16)
    cs.append(_case("btype_3", st, BAD_BLOCK_TYPE, "invalid block type"))
    st = Stream().fixed([b"ok"])
    st._header(True, 3)
    st.w.bits(0, 16)
    cs.append(_case("btype_3_after_a_block", st, BAD_BLOCK_TYPE, "invalid block type"))
    # stored: NLEN is not ~LEN; LEN reaches past the payload
    cs.append(_case("stored_nlen_mismatch", Stream().stored(b"abcd", final=True, nlen=0x1234), BAD_STORED,
                    "invalid stored block lengths"))
    cs.append(_case("stored_len_past_payload", Stream().stored(b"abcd", final=True, len_=40), BAD_STORED, isize=40))
    # HLIT / HDIST above 286 / 30
    for hlit, hdist in ((287, 30), (288, 30), (286, 31), (286, 32)):
        cs.append(_case("hlit_%d_hdist_%d" % (hlit, hdist),
                        Stream().dynamic([b"x"], final=True, ll=[8] * 226 + [9] * 60 + [8, 8], d=[5] * 32, hlit=hlit,
                                         hdist=hdist), BAD_TABLE, "too many length or distance symbols"))
    # over-subscribed codes
    cs.append(_case("cl_code_oversubscribed", Stream().dynamic([b"ab"], final=True, ll=ll8, d=[0],
                                                               cl=_lens(19, {0: 1, 8: 1, 16: 1, 18: 2})),
                    BAD_TABLE, "invalid code lengths set"))
    cs.append(_case("literal_length_code_oversubscribed", Stream().dynamic([b"ab"], final=True, ll=[8] * 286, hlit=286),
                    BAD_TABLE, "invalid literal/lengths set"))
    cs.append(_case("distance_code_oversubscribed", Stream().dynamic(ok_seq, final=True, d=[0, 0, 0, 0, 0, 1, 1, 1]),
                    BAD_TABLE, "invalid distances set"))
    # incomplete codes: zlib (inflate_table) and libdeflate both reject them, except a single code of length 1 for the
    # literal/length and distance alphabets and an empty distance code
    # (the literal/length code behind it is complete: 226 x 8 + 60 x 9 bits, written with 8, 9, 16 and a 0)
    cs.append(_case("cl_code_incomplete", Stream().dynamic([b"ab"], final=True, ll=[8] * 226 + [9] * 60, d=[0],
                                                           cl=_lens(19, {0: 2, 8: 3, 9: 3, 16: 2})),
                    BAD_TABLE, "invalid code lengths set"))
    cs.append(_case("literal_length_code_incomplete", Stream().dynamic([b"ab"], final=True, ll=[9] * 256 + [2], d=[0]),
                    BAD_TABLE, "invalid literal/lengths set"))
    cs.append(_case("distance_code_incomplete_two_codes", Stream().dynamic(ok_seq, final=True, d=[0, 0, 0, 2, 0, 2]),
                    BAD_TABLE, "invalid distances set"))
    cs.append(_case("distance_code_single_of_length_2", Stream().dynamic(ok_seq, final=True, d=[0, 0, 0, 0, 0, 2]),
                    BAD_TABLE, "invalid distances set"))
    # the literal/length lengths of the fixed code in a dynamic block: with 286 symbols (HLIT cannot say 288) the code
    # misses two 8-bit codes, so it is incomplete too; HCLEN 7 (16 17 18 0 8 7 9), no distance code
    st = Stream().dynamic([b"fixed lengths, dynamic block"], final=True, ll=FIXED_LL[:286], d=[0], hlit=286, hdist=1)
    assert int.from_bytes(st.getvalue()[:3], "little") >> 13 & 15 == 7 - 4
    cs.append(_case("dynamic_with_fixed_lengths_hlit_286", st, BAD_TABLE, "invalid literal/lengths set"))
    # code-length sequence defects: a 16 first, a repeat past HLIT + HDIST, EOB without a code
    ll = huffman_lengths(ll_freqs([b"ab"])[:286], 15)
    ops = rle(ll[:257] + [0], {})
    assert ops[-1] == 0 and ops[0] == (18, 97)
    cs.append(_case("repeat_16_first", Stream().dynamic([b"ab"], final=True, ll=ll, d=[0], hlit=257, hdist=1,
                                                        ops=[(16, 3)] + ops[1:]), BAD_TABLE, "invalid bit length repeat"))
    cs.append(_case("repeat_past_hlit_plus_hdist", Stream().dynamic([b"ab"], final=True, ll=ll, d=[0], hlit=257, hdist=1,
                                                                    ops=ops[:-1] + [(18, 20)]),
                    BAD_TABLE, "invalid bit length repeat"))
    cs.append(_case("eob_without_a_code", Stream().dynamic([b"ab"], final=True, ll=_lens(257, {97: 1, 98: 1}), d=[0],
                                                           hlit=257, hdist=1, eob=False),
                    BAD_TABLE, "invalid code -- missing end-of-block"))
    # symbols the fixed code has but the alphabets do not
    for s in (286, 287):
        cs.append(_case("fixed_symbol_%d" % s, Stream().fixed([b"abc", Sym(s), DSym(0)], final=True), BAD_CODE,
                        "invalid literal/length code"))
    for s in (30, 31):
        cs.append(_case("fixed_distance_%d" % s, Stream().fixed([b"abc", Sym(257), DSym(s)], final=True), BAD_CODE,
                        "invalid distance code"))
    # the unused half of a single 1-bit distance code: its code is '0', a '1' is no code
    seq = [b"abcdefgh", Match(4, 7)]
    ll = huffman_lengths(ll_freqs(seq)[:286], 15)
    st = Stream().dynamic(seq, final=True, ll=ll, d=[0, 0, 0, 0, 0, 1], hdist=6, eob=False)
    llc = canonical(ll)
    st.w.code(*llc[len_code(4)[0]])
    st.w.bits(1, 1)                 # the distance code '1'
    st.w.bits(0, 1)                 # (the extra bit distance code 5 would take)
    st.w.code(*llc[EOB])
    cs.append(_case("single_one_bit_distance_code_unused_half", st, BAD_CODE, "invalid distance code"))
    # a distance past the start of the member
    cs.append(_case("distance_past_start", Stream().fixed([b"abcd", Match(3, 5)], final=True), BAD_DISTANCE,
                    "invalid distance too far back"))
    st = Stream().stored(b"x" * 100)
    st.fixed([Match(10, 101)], final=True)
    cs.append(_case("distance_past_start_after_stored", st, BAD_DISTANCE, "invalid distance too far back"))
    # ISIZE disagrees with the stream: more output than it says (by a literal, by a match), less
    cs.append(_case("more_output_than_isize", Stream().fixed([b"0123456789"], final=True), OUTPUT_OVERRUN, isize=9))
    cs.append(_case("more_output_than_isize_by_a_match", Stream().fixed([b"01", Match(20, 2)], final=True),
                    OUTPUT_OVERRUN, isize=12))
    cs.append(_case("less_output_than_isize", Stream().fixed([b"0123456789"], final=True), SIZE_MISMATCH, isize=11))
    # truncated payloads
    t = _case("", Stream().dynamic([_text(2000, 16), Match(50, 100)], final=True))
    for cut in (1, 3, 40):
        cs.append(t._replace(name="truncated_by_%d_bytes" % cut, payload=t.payload[:-cut], status=ANY))
    t = _case("", Stream().stored(_rand(300, 17), final=True))
    cs.append(t._replace(name="stored_truncated", payload=t.payload[:-1], status=ANY))
    return cs


def corpus():
    cs = valid_cases() + invalid_cases()
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return cs
