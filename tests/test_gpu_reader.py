"""-m gpu: the reader's pinned ring and the pool closed readers park their blocks in (include/hhgt_reader.h) — the only reader
code a host without a device cannot reach; everything else is in tests/test_reader.py."""
import pytest
import torch

from haplohyped_varawareml_amd import synth
from haplohyped_varawareml_amd.reader import VcfReader, _lib_reader, write_bgzf

pytestmark = pytest.mark.gpu
MiB = 1 << 20


def read_to_device(path, text, block_bytes):
    """every block through hhgt_reader_copy_async on the current stream -> the bytes that arrived on the device"""
    dst = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    at = 0
    with VcfReader(path, block_bytes=block_bytes, n_threads=3, n_blocks=3) as r:
        for b in r:
            assert at + b.size <= len(text)
            r.copy_async(b, dst.data_ptr() + at, stream.cuda_stream)
            stream.synchronize()      # the block goes back to the ring with the next one
            at += b.size
    return dst[:at].cpu().numpy().tobytes()


def test_pinned_ring_and_pool(ctx, tmp_path):
    L = _lib_reader()
    tab = synth.variant_table(3, 3000, 200)
    text, _ = synth.render_fixed_numpy("chr3", tab, 200, seed=3)      # ~2.5 MB
    p = str(tmp_path / "x.vcf.gz")
    write_bgzf(p, text, level=1)
    L.hhgt_reader_trim_pool()
    assert L.hhgt_reader_prewarm(MiB, 3) == 3
    assert read_to_device(p, text, MiB) == text          # the ring is the three prewarmed blocks
    assert L.hhgt_reader_prewarm(MiB, 0) == 3            # ... and they went back
    assert read_to_device(p, text, 2 * MiB) == text      # no block of this size in the pool: pinned afresh
    L.hhgt_reader_trim_pool()
    assert L.hhgt_reader_prewarm(MiB, 0) == 0 and L.hhgt_reader_prewarm(2 * MiB, 0) == 0
