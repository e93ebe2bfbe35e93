"""-m gpu: the emission path of the bit-plane LZ4 coder (csrc/lz4bits.hip: bp_queue_and_drain, bp_emit_batch, bp_put_entry)
on planes crafted for it.  One chunk of 256 planes per case; every stream must be byte-identical to tools/sim/gapenc_ref.c and
the chunk must decode to the planes (oracle.blosc_decompress, inside run_planes_from_bits / run_planes).

What the planes are crafted for is looked up in the REFERENCE's streams first: its LZ4 sequences are parsed on the CPU and
every case below must occur in at least one plane of the chunk before the GPU is asked — a chunk that misses a case fails.

  lit6 / lit7      a literal run of exactly 6 / 7 bytes: the last the owning lane stores itself, the first the wave stores
  lit64 / lit65    ... of exactly 64 / 65 bytes: one and two rounds of the wave's literal loop
  lit270           ... of >= 270 bytes: more than one extension byte of the literal length
  stage_overflow   one sequence larger than the staging area (576 bytes, 448 with missing calls): its batch goes to global
                   memory directly
  T274 / M274      an offset-1 run / a table match of >= 274 bytes: more than one extension byte of the match length
  M_T_rs_e         a match that ends in zeros with the run behind it (no literal in between): an entry with M and T
  M_T_rs_e1        a match that ends with its last one, >= 5 zeros behind it: the run's one literal is the constant 0
  run_dropped      >= 4 zeros behind a match, and the next match was pulled back over them: no run in between
  entries>100      more emitting entries in a plane than the queue holds: it is drained and refilled several times
  entries>=300,no_match   the same with runs only (irregular gaps of 5-9 zeros)

Which of them a depth can show.  Without candidates (depth 0) there is no table match, so M274, M_T_*, run_dropped cannot
occur.  With candidates a long literal run needs many ones in a row that find no match worth taking; two ones that share
their first gap nearly always do (forward part >= 4 and a gain as soon as one more gap or two zeros agree), so on 0/1 planes
no run past ~30 bytes was found by search, and lit64 / lit65 / lit270 / stage_overflow are asked for at depth 0 only.  With
missing calls two ones agree only if their classes do, and a cluster whose classes keep every candidate from agreeing was
found by a search against the reference at depths 2 and 12, with and without the lazy rule (CLUSTER below: every prefix of it
stays one literal run at all four): planes with missing calls show every case at every depth.

Depths 0, 2 and 12 come from clevel 1, 5 and 9; clevel 9 adds the lazy rule.  Depth 2 with and depth 12 without it are
reached through HHGT_LZ4_LAZY, which the library reads once per process: those two run in a child process each."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_lz4_bitplanes import run_planes, run_planes_from_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
MISSING = 0xF7
LAZY = 0x100
STAGE = {"plain": 576, "missing": 448}
MAXONES = {"plain": 636, "missing": 540}
N_PLANES = 256
# (depth argument of gapenc_ref) -> (HHGT_LZ4_LAZY of the process, clevel); None: this process
CONFIGS = {0: (None, 1), 2: (None, 5), 2 | LAZY: ("1", 5), 12: ("0", 9), 12 | LAZY: (None, 9)}
LONG = ["lit64", "lit65", "lit270", "stage_overflow"]
# ones of a cluster at the start of a plane, one digit each: 2 x (zeros in front of the one) + (1: a missing call)
CLUSTER = ("0642733130541310312004041570104303231317201343320300121132121030112140111123601000001330161300011001400113100001331201"
           "0000001200001113320132121100010000101111012001110000010100013000001013100121312000130113320132112120012100001011011000"
           "0010001010000013113130101200001130010100100001300000010121011201320012000113013001111101101001120012100120000110001130"
           "00132101404")


def expected_cases(kind, depth):
    c = ["lit6", "lit7", "T274", "entries>100"]
    if depth & 0xFF == 0:
        return c + LONG + ["entries>=300,no_match"]
    return c + ["M274", "M_T_rs_e", "M_T_rs_e1", "run_dropped"] + (LONG if kind == "missing" else [])


def parse_lz4(st):
    """LZ4 block of a plane -> [(where its literals start in the plane, literals, match length, offset)]; the last sequence
    has no match (length 0)"""
    st = [int(b) for b in st]
    seqs, ip, op = [], 0, 0

    def more(v):
        nonlocal ip
        while v >= 15:
            v += st[ip]
            ip += 1
            if st[ip - 1] != 255:
                break
        return v
    while True:
        tok = st[ip]
        ip += 1
        ll = more(tok >> 4)
        at = op
        ip += ll
        op += ll
        if ip == len(st):
            seqs.append((at, ll, 0, 0))
            break
        off = st[ip] | (st[ip + 1] << 8)
        ip += 2
        ml = more(tok & 15) + 4
        seqs.append((at, ll, ml, off))
        op += ml
    assert op == N and ip == len(st)
    return seqs


def cases_in(pl, st, kind):
    """the cases of the module's docstring that the stream st of plane pl shows"""
    out = set()
    body = parse_lz4(st)[:-1]
    nzpos = np.flatnonzero(pl)
    # a run copies zeros at offset 1; a table match covers its one (a nonzero byte)
    kinds = ["T" if off == 1 and not pl[at + ll:at + ll + ml].any() else "M" for at, ll, ml, off in body]
    entries = 0
    for i, (at, ll, ml, off) in enumerate(body):
        e = at + ll + ml
        if ll in (6, 7, 64, 65):
            out.add("lit%d" % ll)
        if ll >= 270:
            out.add("lit270")
        if 3 + ll > STAGE[kind]:
            out.add("stage_overflow")
        if ml >= 274:
            out.add(kinds[i] + "274")
        behind_m = False   # a run without a literal, or with the one zero behind the match's last one: the same entry's T
        if kinds[i] == "T" and i > 0 and kinds[i - 1] == "M":
            if ll == 0:
                out.add("M_T_rs_e")
                behind_m = True
            elif ll == 1 and pl[at] == 0:
                out.add("M_T_rs_e1")
                behind_m = True
        entries += not behind_m
        if kinds[i] == "M" and i + 1 < len(body) and kinds[i + 1] == "M":
            k = np.searchsorted(nzpos, e)
            re = min(int(nzpos[k]) if k < len(nzpos) else N, N - 5)
            rs = e + (1 if pl[e - 1] else 0)
            if re - rs >= 4 and rs <= N - 12 and body[i + 1][0] + body[i + 1][1] < re:
                out.add("run_dropped")
    if entries > 100:
        out.add("entries>100")
    if entries >= 300 and "M" not in kinds:
        out.add("entries>=300,no_match")
    return out


def cluster(n_ones, last=None):
    """positions and bytes of the first n_ones ones of CLUSTER (and one more, `last`)"""
    pos, val, p = [], [], -1
    for ch in CLUSTER[:n_ones]:
        p += 1 + int(ch) // 2
        pos.append(p)
        val.append(MISSING if int(ch) & 1 else 1)
    if last:
        pos.append(last[0])
        val.append(last[1])
    return pos, val


class Lcg:
    """the planes must not move with a library's generator"""

    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFF

    def next(self, n):
        self.s = (self.s * 1664525 + 1013904223) & 0xFFFFFFFF
        return (self.s >> 8) % n


def crafted_planes(kind):
    """256 planes of 0 / 1 (kind "missing": and 0xF7, every seventh nonzero byte or so), at most 636 / 540 nonzero bytes each:
    planes of irregular gaps of 5-9 zeros; mixtures of dense clusters (gaps of 0-3 zeros, some hundreds of bytes long), motifs
    repeated up to 120 times, stretches of up to 400 zeros and sparse ones; with missing calls, every fourth plane starts with
    a prefix of CLUSTER (literal runs of 64, 65, ~300 and > 448 bytes at every depth) and 300 zeros"""
    exc = kind == "missing"
    planes = []
    for k in range(N_PLANES):
        g = Lcg(1000 + k)
        a = np.zeros(N, np.uint8)
        pos = ones = 0
        mode = k % 4
        if exc and k % 16 in (5, 6, 7, 9):
            cp, cv = {5: cluster(len(CLUSTER)), 6: cluster(31, (62, MISSING)), 7: cluster(32, (63, 1)), 9: cluster(220)}[k % 16]
            a[cp] = cv
            ones = len(cp)
            pos = cp[-1] + 300

        def put(p):
            nonlocal ones
            if p < N and ones < MAXONES[kind]:
                a[p] = MISSING if exc and g.next(7) == 0 else 1
                ones += 1
        if mode == 0:
            while pos < N:
                put(pos)
                pos += 6 + g.next(5)
        while mode and pos < N and ones < MAXONES[kind]:
            what = g.next(6)
            if what <= 1:      # a dense cluster (modes 3: the first one is very long)
                span = 300 + 350 * (k % 8 >= 4) if mode == 3 and pos < 100 else 3 + g.next(70)
                end = pos + span
                while pos < end:
                    put(pos)
                    pos += 1 + g.next(4)
                pos += 5 + g.next(30)
            elif what == 2:    # a motif repeated: long matches
                per = 2 + g.next(9)
                for _ in range(3 + g.next(120 if mode == 2 else 12)):
                    put(pos)
                    if per > 4 and g.next(2):
                        put(pos + 2)
                    pos += per
                pos += g.next(12)
            elif what == 3:    # a long stretch of zeros
                put(pos)
                pos += 10 + g.next(400 if mode == 2 else 60)
            else:              # sparse ones
                for _ in range(1 + g.next(20)):
                    put(pos)
                    pos += 5 + g.next(9)
        planes.append(a)
    return planes


@pytest.fixture(scope="module")
def planes():
    return {kind: crafted_planes(kind) for kind in ("plain", "missing")}


@pytest.fixture(scope="module")
def ref_streams(tmp_path_factory, planes):
    """(kind, depth) -> the reference's streams of the 256 planes, each computed once"""
    so = str(tmp_path_factory.mktemp("gapenc_emit") / "libgapenc.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "sim", "gapenc_ref.c")])
    L = C.CDLL(so)
    L.gapenc_ref.restype = C.c_int
    L.gapenc_ref.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    cache = {}

    def get(kind, depth):
        if (kind, depth) not in cache:
            out = []
            for pl in planes[kind]:
                buf = np.zeros(N + 64, np.uint8)
                n = L.gapenc_ref(pl.ctypes.data, N, buf.ctypes.data, depth)
                assert 0 < n < N, "a crafted plane the coder would refuse or store verbatim"
                out.append(buf[:n].copy())
            cache[(kind, depth)] = out
        return cache[(kind, depth)]
    return get


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from haplohyped_varawareml_amd import device as dev
from tests.test_gpu_lz4_bitplanes import run_planes_from_bits
from tests.test_gpu_lz4_emit import crafted_planes
ctx = dev.Context(0)
ctx.set_clevel(int(sys.argv[1]))
out = {}
for kind in ("plain", "missing"):
    got, _ = run_planes_from_bits(ctx, crafted_planes(kind))
    out[kind + "_sizes"] = np.array([g.size for g in got])
    out[kind + "_bytes"] = np.concatenate(got)
np.savez(sys.argv[2], **out)
"""


@pytest.fixture(scope="module")
def gpu_streams(ctx, planes, tmp_path_factory):
    """(kind, depth) -> the kernel's streams of the chunk, from the bit-plane form (k_lz4_bitplanes_uni); the chunk has decoded
    to the planes (run_planes_from_bits asserts it)"""
    cache = {}

    def get(kind, depth):
        lazy_env, clevel = CONFIGS[depth]
        if (kind, depth) in cache:
            return cache[(kind, depth)]
        if lazy_env is None:
            ctx.set_clevel(clevel)
            try:
                cache[(kind, depth)] = run_planes_from_bits(ctx, planes[kind])[0]
            finally:
                ctx.set_clevel(5)
        else:   # one child for both kinds
            npz = str(tmp_path_factory.mktemp("emit_child") / "streams.npz")
            r = subprocess.run([sys.executable, "-c", CHILD % ROOT, str(clevel), npz], env=dict(os.environ, HHGT_LZ4_LAZY=lazy_env),
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            z = np.load(npz)
            for kd in ("plain", "missing"):
                cache[(kd, depth)] = np.split(z[kd + "_bytes"], np.cumsum(z[kd + "_sizes"])[:-1])
        return cache[(kind, depth)]
    return get


def assert_cases(kind, depth, planes, want):
    seen = set()
    for pl, st in zip(planes, want):
        seen |= cases_in(pl, st, kind)
    missing = sorted(set(expected_cases(kind, depth)) - seen)
    assert not missing, f"{kind}, depth {depth:#x}: no plane of the chunk shows {missing}"


@pytest.mark.parametrize("depth", sorted(CONFIGS))
@pytest.mark.parametrize("kind", ["plain", "missing"])
def test_crafted_chunk_matches_the_reference(planes, ref_streams, gpu_streams, kind, depth):
    want = ref_streams(kind, depth)
    assert max(int((pl != 0).sum()) for pl in planes[kind]) <= MAXONES[kind]
    assert_cases(kind, depth, planes[kind], want)
    got = gpu_streams(kind, depth)
    assert len(got) == N_PLANES
    for k in range(N_PLANES):
        assert np.array_equal(got[k], want[k]), f"{kind}, depth {depth:#x}: plane {k} differs from gapenc_ref ({got[k].size} vs {want[k].size} bytes)"


@pytest.mark.parametrize("depth", [0, 2, 12 | LAZY])
def test_crafted_chunk_from_int8_input(ctx, planes, ref_streams, depth):
    """the same 0/1 planes as int8 bytes: k_lz4_bitplanes shares the emission phases"""
    want = ref_streams("plain", depth)
    assert_cases("plain", depth, planes["plain"], want)
    ctx.set_clevel(CONFIGS[depth][1])
    try:
        got, _ = run_planes(ctx, planes["plain"])
    finally:
        ctx.set_clevel(5)
    for k in range(N_PLANES):
        assert np.array_equal(got[k], want[k]), f"int8 input, depth {depth:#x}: plane {k} differs from gapenc_ref"
