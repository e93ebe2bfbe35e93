"""-m gpu: the candidate phases of the bit-plane LZ4 coder (csrc/lz4bits.hip: bp_lane_one, bp_pick, bp_extend_and_price) on
planes crafted for the 16-bit halves the extension keeps its pairs in.  One chunk of 256 planes per case set
(tests/lz4_pk16_cases.py); every stream must be byte-identical to tools/sim/gapenc_ref.c and the chunk must decode to the
planes (oracle.blosc_decompress, inside run_planes_from_bits / run_planes).

What the planes are crafted for is looked up in the REFERENCE first.  tests/lz4_pk16_cases.py states gapenc_ref.c in Python and
records, per one, what its extension and its pricing saw; that statement is held to the C reference byte for byte on every plane
of the chunk, and every case below must occur in at least one plane before the GPU is asked — a chunk that misses a case fails.

  one_at_0 / _1 / _4094 / _4095   P holds 1, 2, 4095, 4096 in front of the sentinels 4097; the last one followed by nothing
  single_one, gap_4094             a plane of one one; two ones 4095 apart
  gap_254 / 255 / 256 / 4000       such gaps in the plane — and in the extension: equal_gaps_254_agree (an equal pair of 254
                                   zeros is walked over), equal_gaps_255_stop / _256_stop (an equal pair the clip of the gap
                                   byte ends the extension at, though the unclipped gaps from P agree), gap_4000_in_extension
  past_third_gap, steps_limit      periodic planes: the extension goes on behind the pick's three gaps, to BP_STEPS
  clamped                          ... and the match is cut at the stream's match limit
  front_candidate_larger / front_one_larger, pull_back_0 / 63 / 64 / 65
                                   zeros in front of the one and of its candidate: the smaller wins, 64 at most
  gain_-1 / gain_0 / gain_+1       a candidate whose match is worth exactly that against literals: taken only at +1
  tie_nearer_wins                  two candidates of equal score at different distances
  ones_636 / 637 (540 / 541 with missing calls)   the longest list the coder takes, and one more: the byte-wise coder's plane

Without candidates (depth 0) only the cases that are properties of the plane can occur.  With missing calls the planes with more
than 540 nonzero bytes are the byte-wise coder's.  Depths 0, 2 and 12 come from clevel 1, 5 and 9; clevel 9 adds the lazy rule.
Depth 2 with and depth 12 without it are reached through HHGT_LZ4_LAZY, which the library reads once per process: one child
process codes both kinds of chunk at both."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.lz4_pk16_cases import LAZY, MISSING, N, cases_of, chunk_planes, coder_constants, gapenc_model
from tests.test_gpu_lz4_bitplanes import run_planes, run_planes_from_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PLANES = 256
# (depth argument of gapenc_ref) -> (HHGT_LZ4_LAZY of the process, clevel); None: this process
CONFIGS = {0: (None, 1), 2: (None, 5), 2 | LAZY: ("1", 5), 12: ("0", 9), 12 | LAZY: (None, 9)}
OF_THE_PLANE = ["one_at_0", "one_at_1", "one_at_4094", "one_at_4095", "single_one", "gap_4094", "gap_254", "gap_255", "gap_256", "gap_4000"]
OF_THE_CANDIDATES = ["equal_gaps_254_agree", "equal_gaps_255_stop", "equal_gaps_256_stop", "gap_4000_in_extension", "past_third_gap",
                     "steps_limit", "clamped", "front_candidate_larger", "front_one_larger", "pull_back_0", "pull_back_63", "pull_back_64",
                     "pull_back_65", "gain_-1", "gain_0", "gain_+1", "tie_nearer_wins"]


def expected_cases(kind, depth):
    limits = ["ones_540", "ones_541"] if kind == "missing" else ["ones_636", "ones_637"]
    return OF_THE_PLANE + limits + (OF_THE_CANDIDATES if depth & 0xFF else [])


@pytest.fixture(scope="module")
def planes():
    return {kind: chunk_planes(kind, N_PLANES) for kind in ("plain", "missing")}


@pytest.fixture(scope="module")
def reference(tmp_path_factory, planes):
    """(kind, depth) -> (the reference's streams of the 256 planes — None where the plane is the byte-wise coder's —, the cases
    the chunk shows), each computed once; the Python statement that names the cases has given the same bytes as the C reference"""
    so = str(tmp_path_factory.mktemp("gapenc_pk16") / "libgapenc.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "sim", "gapenc_ref.c")])
    L = C.CDLL(so)
    L.gapenc_ref.restype = C.c_int
    L.gapenc_ref.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    K = coder_constants()
    cache, models = {}, {}

    def get(kind, depth):
        if (kind, depth) in cache:
            return cache[(kind, depth)]
        streams, seen = [], set()
        for pl in planes[kind]:
            buf = np.zeros(N + 64, np.uint8)
            n = L.gapenc_ref(pl.ctypes.data, N, buf.ctypes.data, depth)
            want = None if n < 0 else buf[:n].copy()
            key = (pl.tobytes(), depth)
            if key not in models:      # (the chunk repeats its planes shifted; equal planes are stated once)
                models[key] = gapenc_model(pl, depth, K)
            st, recs = models[key]
            assert (st is None) == (want is None)
            assert want is None or np.array_equal(st, want), "the Python statement of gapenc_ref.c differs from it"
            assert want is None or want.size < N, "a crafted plane the coder would store verbatim"
            streams.append(want)
            seen |= cases_of(pl, recs)
        cache[(kind, depth)] = (streams, seen)
        return cache[(kind, depth)]
    return get


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from haplohyped_varawareml_amd import device as dev
from tests.test_gpu_lz4_bitplanes import run_planes_from_bits
from tests.lz4_pk16_cases import chunk_planes
ctx = dev.Context(0)
ctx.set_clevel(int(sys.argv[1]))
out = {}
for kind in ("plain", "missing"):
    got, _ = run_planes_from_bits(ctx, chunk_planes(kind, 256))
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
            npz = str(tmp_path_factory.mktemp("pk16_child") / "streams.npz")
            r = subprocess.run([sys.executable, "-c", CHILD % ROOT, str(clevel), npz], env=dict(os.environ, HHGT_LZ4_LAZY=lazy_env),
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            z = np.load(npz)
            for kd in ("plain", "missing"):
                cache[(kd, depth)] = np.split(z[kd + "_bytes"], np.cumsum(z[kd + "_sizes"])[:-1])
        return cache[(kind, depth)]
    return get


def assert_cases(kind, depth, seen):
    missing = sorted(set(expected_cases(kind, depth)) - seen)
    assert not missing, f"{kind}, depth {depth:#x}: no plane of the chunk shows {missing}"


def assert_streams(tag, planes, got, want):
    assert len(got) == len(want) == N_PLANES
    coded = 0
    for k in range(N_PLANES):
        if want[k] is None:      # more ones than the list holds: the byte-wise coder's stream (the chunk has decoded to the planes)
            continue
        coded += 1
        assert np.array_equal(got[k], want[k]), f"{tag}: plane {k} differs from gapenc_ref ({got[k].size} vs {want[k].size} bytes)"
    assert coded >= N_PLANES - 16


@pytest.mark.parametrize("depth", sorted(CONFIGS))
@pytest.mark.parametrize("kind", ["plain", "missing"])
def test_crafted_chunk_matches_the_reference(planes, reference, gpu_streams, kind, depth):
    want, seen = reference(kind, depth)
    if kind == "missing":
        assert sum(bool((pl == MISSING).any()) for pl in planes[kind]) >= N_PLANES - 8
    assert_cases(kind, depth, seen)
    assert_streams(f"{kind}, depth {depth:#x}", planes[kind], gpu_streams(kind, depth), want)


@pytest.mark.parametrize("depth", [0, 2, 12 | LAZY])
def test_crafted_chunk_from_int8_input(ctx, planes, reference, depth):
    """the same 0/1 planes as int8 bytes: k_lz4_bitplanes shares the candidate phases"""
    want, seen = reference("plain", depth)
    assert_cases("plain", depth, seen)
    ctx.set_clevel(CONFIGS[depth][1])
    try:
        got, _ = run_planes(ctx, planes["plain"])
    finally:
        ctx.set_clevel(5)
    assert_streams(f"int8 input, depth {depth:#x}", planes["plain"], got, want)
