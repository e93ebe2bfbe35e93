"""-m gpu: hhgt_reserve covers what the calls it names allocate.  The ingest engine reserves once so that no hipMalloc (which
stalls every stream) falls into its first pass; the test holds the library to that: after a reserve for the largest encode
and compress call to come, those calls make no workspace of their own but the one word the LZ4 launch keeps its flag in."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARKER = "-- reserved --"
LZ_FLAGS_BYTES = 4 + 4 // 8 + 256     # what DevBuf::ensure(4) asks of hipMalloc

# 70 samples in chunks of 64 x 4096: two sample chunks, the second partial, in one chunk column
CHILD = r"""
import sys
sys.path.insert(0, %r)
import ctypes as C
import torch
from haplohyped_varawareml_amd import device as dev, synth
from haplohyped_varawareml_amd._lib import check
from tests.gpu_util import to_dev

S, V, sc, vc = 70, 300, 64, 4096
ctx = dev.Context(0)
text = to_dev(synth.render_fixed_numpy("chr5", synth.variant_table(5, V, S), S, seed=5)[0])
max_lines = 4096     # (every per-line workspace is then 16 KiB, well over what the parent allows a late allocation)
lay = dev.make_layout(S, vc, sc=sc, vc=vc)
z = lambda n, dt: torch.zeros(n, dtype=dt, device=ctx.device)
new = lambda G, P: dev.EncodeResult(G, lay, z(vc, torch.int32), z(vc, torch.int32), z(vc, torch.uint8), z(vc, torch.uint8), 0, {}, [], P)
planes, matrix = new(None, z(dev.planes_bytes(lay), torch.uint8)), new(z(dev.layout_bytes(lay), torch.uint8), None)
check(ctx.lib.hhgt_reserve(ctx.h, text.numel(), max_lines, 2, sc * vc * 2, 2, 8192))
torch.cuda.synchronize()
sys.stderr.write(%r + "\n")
sys.stderr.flush()

cursor = z(1, torch.int64)
rec = ctx.encode_text_planes_async(text, S, planes, cursor, max_lines=max_lines).wait()
assert rec.stats.n_kept == V
ctx.pad_tail_planes_cursor(planes, cursor)
_, off, total = ctx.compress_planes(planes)
assert off.numel() == 3 and total > 0

cursor = z(1, torch.int64)
rec = ctx.encode_text_async(text, S, matrix, cursor, max_lines=max_lines).wait()
assert rec.stats.n_kept == V
_, off, total = ctx.compress(matrix.G, sc * vc * 2)
assert off.numel() == 3 and total > 0
ctx.close()
""" % (ROOT, MARKER)


def test_reserved_calls_allocate_nothing():
    """one fresh child: HHGT_ALLOC_DEBUG is read once per process"""
    env = dict(os.environ, HHGT_ALLOC_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=120)
    print(r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    before, marker, after = r.stderr.partition(MARKER)
    assert marker, "the child never reserved"
    sizes = lambda s: [int(n) for n in re.findall(r"^\[alloc\].* hipMalloc (\d+) took", s, flags=re.M)]
    assert sizes(before), "HHGT_ALLOC_DEBUG shows nothing: the switch is dead"
    # the one-word lz_flags buffer of workspace set 0 is made by the first LZ4 launch: under 4 KiB, and nothing else — so
    # that the small workspaces (a few regions' counts, the run tables, the framing sizes of two chunks) are held to it too
    late = sizes(after)
    assert all(n < 4096 for n in late), f"allocations behind hhgt_reserve: {late} bytes"
    assert late in ([], [LZ_FLAGS_BYTES]), f"allocations behind hhgt_reserve besides lz_flags: {late} bytes"
