"""-m gpu: the bit-plane encoder's 252-sample bands (csrc/encode.hip k_encode_planes).  A band of a line is read as one
16-byte-aligned 1 KiB window, and each lane rebuilds its four fields from its chunk and its neighbour's by the phase at
which the line's sample columns start.  The planes, expanded, must equal the oracle's matrix:
* for every phase of the sample columns against 16 bytes (the INFO column's width walks through 32 values);
* for sample counts around the band and lane edges (last bands of 1..3 samples, S = 2504);
* with the last line ending exactly at the end of a text whose length is not a multiple of 16;
* with '/' and '.' calls, GT:DP records whose columns are all of one width, and third alleles (variable-width kernel);
* appended in several blocks at a device cursor (tiles straddle the append position), and into a ring of columns."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests.gpu_util import to_dev
from tests.test_gpu_planes import _blocks, _dense_from_bytes, _encode_planes, _new_result
from haplohyped_varawareml_amd import device as dev

pytestmark = pytest.mark.gpu

CALLS = np.array([b"0|0", b"0|1", b"1|0", b"1|1", b"0/1", b".|.", b"./0", b"1|."])
WEIGHTS = np.array([70, 8, 8, 6, 3, 2, 2, 1], np.float64)


def _text(S, V, seed, mixed=False):
    """a GT-only VCF text of V records x S samples on chr7; the INFO width cycles through 0..31 extra bytes, so the sample
    columns start at every phase against 16 bytes.  mixed: some GT:DP records of one column width, and third alleles."""
    rng = np.random.default_rng(seed)
    head = ["##fileformat=VCFv4.2", "##contig=<ID=chr7>", '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
            '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Read Depth">',
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"S{i}" for i in range(S))]
    out = ["\n".join(head) + "\n"]
    p = WEIGHTS / WEIGHTS.sum()
    for v in range(V):
        calls = CALLS[rng.choice(len(CALLS), size=S, p=p)].astype(object)
        fmt = "GT"
        if mixed and v % 7 == 3:
            fmt = "GT:DP"
            calls = np.array([c + b":" + b"%02d" % d for c, d in zip(calls, rng.integers(10, 99, S))], dtype=object)
        if mixed and v % 11 == 5:
            calls[rng.integers(0, S)] = b"2|0"
        info = "AC=1" + "x" * ((v * 7) % 32)
        line = f"chr7\t{1000 + 10 * v}\t.\tA\tC\t.\tPASS\t{info}\t{fmt}\t" + "\t".join(c.decode() for c in calls) + "\n"
        out.append(line)
    text = "".join(out).encode()
    if len(text) % 16 == 0:      # the last line ends exactly at the end of a text of n != 0 (mod 16) bytes
        out[1] = out[1].replace("AC=1", "AC=1;", 1)
        text = "".join(out).encode()
    assert len(text) % 16 != 0
    return text


def _phases(text):
    """the phases (mod 16) at which the records' sample columns start in the text"""
    ph, at = set(), 0
    for ln in text.split(b"\n"):
        if ln.startswith(b"chr7"):
            ph.add((at + sum(len(f) + 1 for f in ln.split(b"\t")[:9])) % 16)
        at += len(ln) + 1
    return ph


def _check(ctx, text, S, nblk, V):
    o = oracle.vcf_encode(text, S, region="chr7", cap=V)
    nk = o["n_kept"]
    lay = dev.make_layout(S, -(-nk // 4096) * 4096, sc=64, vc=4096)
    res, n, _ = _encode_planes(ctx, text, S, lay, "chr7", nblk, max_lines=lambda t_: t_.numel() // 16 + 8)
    assert n == nk
    G = _dense_from_bytes(ctx.planes_expand(res), lay, nk)
    assert np.array_equal(G, o["G"])
    return o


@pytest.mark.parametrize("S", [1, 3, 63, 64, 251, 252, 253, 255, 256, 257, 503, 504, 505, 2504])
def test_bands_all_phases_vs_oracle(ctx, S):
    V = 700 if S < 1000 else 300
    text = _text(S, V, seed=S)
    assert _phases(text) == set(range(16))
    o = _check(ctx, text, S, 3, V)
    assert o["n_kept"] == V and (o["G"] == -9).any()


@pytest.mark.parametrize("S", [63, 255, 505])
def test_bands_mixed_records_vs_oracle(ctx, S):
    """GT:DP records of one width (second level, at their stride) and third alleles (variable-width kernel)"""
    V = 900
    text = _text(S, V, seed=7 * S, mixed=True)
    o = _check(ctx, text, S, 4, V)
    assert o["n_kept"] == V and (o["G"] == 2).any()


def test_bands_ring_of_columns(ctx):
    """blocks of odd sizes appended into a ring of chunk columns, S with a last band of one sample"""
    S, V, vc, ring = 505, 9000, 4096, 3
    text = _text(S, V, seed=55)
    o = oracle.vcf_encode(text, S, region="chr7")
    assert o["n_kept"] == V
    lay = dev.make_ring_layout(S, ring, sc=64, vc=vc)
    res = _new_result(ctx, lay, with_g=False, poison=True)
    ctx.pad_tail_planes(res, lay.v_capacity, 0, ring)
    cursor = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    n_sc = -(-S // 64)
    col_bytes = n_sc * 64 * vc * 2
    got = np.zeros((n_sc * 64, -(-V // vc) * vc, 2), np.int8)
    scratch = torch.zeros(dev.layout_bytes(lay), dtype=torch.uint8, device=ctx.device)

    def take(col):
        slot = col % ring
        ctx.planes_expand(res, col0=slot, n_cols=1, out=scratch)
        raw = scratch[slot * col_bytes:(slot + 1) * col_bytes]
        got[:, col * vc:(col + 1) * vc] = raw.view(torch.int8).view(n_sc, 64, vc, 2).reshape(n_sc * 64, vc, 2).cpu().numpy()

    done = 0
    for blk in _blocks(text, 13):
        rec = ctx.encode_text_planes_async(to_dev(blk), S, res, cursor, region="chr7").wait()
        for col in range(done, rec.cursor_after // vc):
            take(col)
        done = rec.cursor_after // vc
    assert int(cursor.item()) == V
    ctx.pad_tail_planes_cursor(res, cursor)
    take(done)
    assert np.array_equal(got[:S, :V], o["G"])
