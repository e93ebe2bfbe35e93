"""-m gpu: the bit-plane LZ4 coder (csrc/lz4bits.hip) from a window's coded ones to the stream's bytes — selection
(bp_select_coded), the queue (bp_queue_and_drain), layout and emission of a batch (bp_emit_batch, bp_put_entry: staged and
direct form) — on planes crafted for each path.  One chunk of 256 planes per kind (tests/lz4_stage_model.py); every stream must
be byte-identical to tools/sim/gapenc_ref.c and the chunk must decode to the planes (oracle.blosc_decompress, inside
run_planes_from_bits / run_planes).

What a plane is a case of is looked up on the CPU first.  tests/lz4_stage_model.py states the kernel's batching in Python —
windows of 64 ones, a batch when 65 entries are queued, 64 entries per batch, queue and staging area of the sizes in the
source — on top of tests/lz4_pk16_cases.gapenc_model's statement of the parse; its bytes are held to the C reference on every
plane of the chunk, and every case below must occur in at least one plane before the GPU is asked: a chunk that misses a case
fails.  (tests/test_lz4_stage_model.py holds the statement to examples worked by hand.)

  staged_at_0 / staged_behind          a batch staged with nothing / with bytes in front of it in the staging area
  fits_exactly / over_by_one_flushes   staged bytes + the batch = the area's size (240; 104 with missing calls): no flush; one
                                       byte more: what is staged leaves first
  total_fills_stage / total_one_more_direct   a batch of exactly the area's size is staged, one byte more goes to the slot directly
  lit_run_0 .. lit_run_7               first-sequence literal runs of that many bytes (up to 6 the lane stores itself)
  f7_at_0 .. f7_at_5                   with missing calls: a 0xF7 at each of the self-stored positions
  lane63_two_sequences / lane63_one_sequence   the entry in lane 63 of a full batch with and without a second sequence
  window_all_coded                     all 64 ones of a window coded
  lane63_hands_over                    the coded one in lane 63 hands over to the next window
  reach_1 / reach_2 / reach_16         a match reaching from its window over that many ones of the next
  ones_1 / 63 / 64 / 65 / 127 / 128 / 129   planes of that many ones
  queue_fits_exactly / queue_over_by_one     queued entries + the window's = the queue's 80: no batch; one more: a batch makes room
  queue_64_at_window_end / queue_65_at_window_end   ... no batch yet / the first batch leaves
  last_window_one_entry                the last batch has one entry

Which of them a depth cannot show at all, and why, stands at lz4_stage_model.NOT_AT_DEPTH_0 / NOT_AT_104_BYTES / OF_MATCHES.
Depths 0, 2 and 12 come from clevel 1, 5 and 9; clevel 9 adds the lazy rule.  Depth 2 with and depth 12 without it are reached
through HHGT_LZ4_LAZY, which the library reads once per process: one child process codes both kinds of chunk at both."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.lz4_pk16_cases import LAZY, MISSING, N
from tests.lz4_stage_model import cases_of, chunk_planes, expected_cases, stage_constants, stage_model
from tests.test_gpu_lz4_bitplanes import run_planes, run_planes_from_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PLANES = 256
# (depth argument of gapenc_ref) -> (HHGT_LZ4_LAZY of the process, clevel); None: this process
CONFIGS = {0: (None, 1), 2: (None, 5), 2 | LAZY: ("1", 5), 12: ("0", 9), 12 | LAZY: (None, 9)}


@pytest.fixture(scope="module")
def planes():
    return {kind: chunk_planes(kind, N_PLANES) for kind in ("plain", "missing")}


@pytest.fixture(scope="module")
def reference(tmp_path_factory, planes):
    """(kind, depth) -> (the reference's streams of the 256 planes, the cases the chunk shows), each computed once; the Python
    statement that names the cases has given the same bytes as the C reference"""
    so = str(tmp_path_factory.mktemp("gapenc_stage") / "libgapenc.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "sim", "gapenc_ref.c")])
    L = C.CDLL(so)
    L.gapenc_ref.restype = C.c_int
    L.gapenc_ref.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    K = stage_constants()
    cache, stated = {}, {}

    def get(kind, depth):
        if (kind, depth) in cache:
            return cache[(kind, depth)]
        streams, seen = [], set()
        for pl in planes[kind]:
            key = (pl.tobytes(), depth)
            if key not in stated:      # (the chunk repeats its planes: each is stated once)
                buf = np.zeros(N + 64, np.uint8)
                n = L.gapenc_ref(pl.ctypes.data, N, buf.ctypes.data, depth)
                assert 0 < n < N, "a crafted plane the coder would not take, or would store verbatim"
                st, windows, batches = stage_model(pl, depth, K)
                assert np.array_equal(st, buf[:n]), "the Python statement of the batching gives other bytes than gapenc_ref.c"
                stated[key] = (buf[:n].copy(), cases_of(pl, windows, batches, K))
            streams.append(stated[key][0])
            seen |= stated[key][1]
        cache[(kind, depth)] = (streams, seen)
        return cache[(kind, depth)]
    return get


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from haplohyped_varawareml_amd import device as dev
from tests.test_gpu_lz4_bitplanes import run_planes_from_bits
from tests.lz4_stage_model import chunk_planes
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
            npz = str(tmp_path_factory.mktemp("stage_child") / "streams.npz")
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


def assert_streams(tag, got, want):
    assert len(got) == len(want) == N_PLANES
    for k in range(N_PLANES):
        assert np.array_equal(got[k], want[k]), f"{tag}: plane {k} differs from gapenc_ref ({got[k].size} vs {want[k].size} bytes)"


@pytest.mark.parametrize("depth", sorted(CONFIGS))
@pytest.mark.parametrize("kind", ["plain", "missing"])
def test_crafted_chunk_matches_the_reference(planes, reference, gpu_streams, kind, depth):
    want, seen = reference(kind, depth)
    if kind == "missing":
        assert all(bool((pl == MISSING).any()) for pl in planes[kind])
    assert_cases(kind, depth, seen)
    assert_streams(f"{kind}, depth {depth:#x}", gpu_streams(kind, depth), want)


@pytest.mark.parametrize("depth", [0, 2, 12 | LAZY])
def test_crafted_chunk_from_int8_input(ctx, planes, reference, depth):
    """the same 0/1 planes as int8 bytes: k_lz4_bitplanes shares the phases"""
    want, seen = reference("plain", depth)
    assert_cases("plain", depth, seen)
    ctx.set_clevel(CONFIGS[depth][1])
    try:
        got, _ = run_planes(ctx, planes["plain"])
    finally:
        ctx.set_clevel(5)
    assert_streams(f"int8 input, depth {depth:#x}", got, want)
