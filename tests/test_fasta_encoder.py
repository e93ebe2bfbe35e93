"""fasta_encoder.  CPU: spec parsing like the reference (fasta_encoder.py:32-45) and the CLI
options (:189-193).  -m gpu: one-hot rows vs a numpy restatement of :47-78 (upper-case, non-ACGT -> N, sorted
columns A,C,G,N,T), store round trip through get_sequence, on the reference's own tests/data/chr22.fasta-shaped
input (1 Mbp synthetic FASTA written here; the reference file itself is ~1 MB of random bases)."""
import os

import numpy as np
import pytest


def test_parse_encode_list_and_cli():
    from haplohyped_varawareml_amd.fasta_encoder import ReferenceGenome, main
    assert ReferenceGenome.parse_encode_list(None) == [b"A", b"C", b"G", b"T", b"N"]
    assert ReferenceGenome.parse_encode_list("ACGT") == [b"A", b"C", b"G", b"T"]
    assert ReferenceGenome.parse_encode_list(["A", b"C"]) == [b"A", b"C"]
    with pytest.raises(TypeError):
        ReferenceGenome.parse_encode_list(123)
    assert ReferenceGenome(encode_spec=None).columns() == ["A", "C", "G", "N", "T"]      # sorted, :60
    assert {p.name for p in main.params} == {"fasta", "outdir", "cores"}


def expected_onehot(seq, cols):
    s = np.char.upper(np.frombuffer(seq, dtype="|S1"))
    s = np.where(np.isin(s, [b"A", b"C", b"G", b"T"]), s, b"N")
    out = np.zeros((len(s), len(cols)), np.uint8)
    for j, c in enumerate(cols):
        out[:, j] = s == c.encode()
    return out


@pytest.mark.gpu
def test_encode_and_store_roundtrip(ctx, tmp_path):
    from haplohyped_varawareml_amd.fasta_encoder import ReferenceGenome
    rng = np.random.default_rng(5)
    seqs = {"chr21": b"".join(rng.choice([b"A", b"C", b"G", b"T", b"N", b"a", b"c", b"g", b"t", b"n", b"R"], 300_001).tolist()),
            "chr22": b"".join(rng.choice([b"A", b"C", b"G", b"T"], 1_000_000).tolist())}
    fa = tmp_path / "g.fasta"
    with open(fa, "wb") as f:
        for name, s in seqs.items():
            f.write(b">" + name.encode() + b" test\n")
            for i in range(0, len(s), 80):
                f.write(s[i:i + 80] + b"\n")
    rg = ReferenceGenome(fasta_file=str(fa), output_dir=str(tmp_path / "store"), ctx=ctx)
    assert np.array_equal(rg.encode_sequence("ACGTNacgtnX"), expected_onehot(b"ACGTNacgtnX", rg.columns()))
    assert rg.encode_sequence("ACGTN")[4, 3] == 1            # N column is index 3 in sorted order
    done = rg.load_genome_parallel()
    assert sorted(done) == ["chr21", "chr22"]
    for name, s in seqs.items():
        exp = expected_onehot(s, rg.columns())
        for a, b in ((0, 1000), (262_100, 262_300), (len(s) - 500, len(s) + 50), (123_456, 200_000)):
            got = rg.get_sequence(name, a, b)
            assert got.dtype == np.int8 and np.array_equal(got.view(np.uint8), exp[a:min(b, len(s))])
        assert np.array_equal(rg.get_sequence(name, 0, len(s)).sum(axis=1), np.ones(len(s)))


@pytest.mark.gpu
def test_load_chromosome_past_one_kernel_pass(ctx, tmp_path):
    """a 70 Mbp contig is one hhgt_onehot_bases_u8 call of 350 MB, more than five grid passes of 2^26 bytes: the rows
    that straddle each pass boundary (2^26 is not a multiple of 5), read back through the store"""
    from haplohyped_varawareml_amd.fasta_encoder import ReferenceGenome
    from tests.test_dataset import write_fasta
    n, step = 70_000_003, 1 << 26
    rng = np.random.default_rng(70)
    seq = np.frombuffer(b"ACGTACGTACGTacgtNnR", np.uint8)[rng.integers(0, 19, n)]
    write_fasta(tmp_path / "big.fa", "chr2", seq)
    rg = ReferenceGenome(fasta_file=str(tmp_path / "big.fa"), output_dir=str(tmp_path / "store"), ctx=ctx)
    rg.load_chromosome("chr2")
    cols = rg.columns()
    windows = [(t * step // 5 - 3000, t * step // 5 + 3000) for t in range(1, -(-n * 5 // step))]
    assert len(windows) == 5
    for a, b in windows + [(0, 4000), (n - 4000, n + 10)]:
        got = rg.get_sequence("chr2", a, b)
        assert np.array_equal(got.view(np.uint8), expected_onehot(seq[a:b].tobytes(), cols)), (a, b)
