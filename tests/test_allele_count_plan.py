"""CPU: store.plan_counts (the selections of GenotypeStore.allele_counts) against brute force — every (sample, variant) of
a request covered exactly once, nothing outside it, pad rows and pad variants never — and the allele_freq TSV formatter
against literal text."""
import numpy as np
import pytest

from haplohyped_varawareml_amd.allele_freq import HEADER, format_rows, parse_region
from haplohyped_varawareml_amd.store import AC, AN, HET, HOM_ALT, plan_counts


def coverage(plan, n_samples, sc, vc, n_variants, v_lo, bs):
    """how often each (sample, variant) is counted, and where its counts go: [S, V] counts and output rows"""
    vb = bs // 2
    hits = np.zeros((-(-n_samples // sc) * sc, -(-max(n_variants, 1) // vc) * vc), np.int64)
    dest = np.full(hits.shape, -1, np.int64)
    for p in plan:
        assert 0 <= p["lo"] < p["hi"] <= vb and p["part"] < vc * 2 // bs
        rows = [r for r in range(64) if int(p["row_mask"]) >> r & 1]
        assert rows and max(rows) < sc
        v0 = int(p["vcol"]) * vc + int(p["part"]) * vb
        for r in rows:
            s = int(p["scol"]) * sc + r
            hits[s, v0 + p["lo"]:v0 + p["hi"]] += 1
            dest[s, v0 + p["lo"]:v0 + p["hi"]] = int(p["out_row"]) + np.arange(p["hi"] - p["lo"])
    return hits, dest


@pytest.mark.parametrize("n_samples,n_variants,sc,vc,bs", [
    (1000, 20_000, 64, 8192, 8192),      # 24 pad rows, a partial last chunk column
    (2504, 9000, 64, 8192, 8192),        # 2504 = 39 x 64 + 8
    (130, 1000, 64, 256, 512),           # one block per row
    (70, 700, 16, 128, 64),              # four blocks per row
])
def test_plan_covers_request_exactly_once(n_samples, n_variants, sc, vc, bs):
    rng = np.random.default_rng(n_samples + n_variants)
    vb = bs // 2
    edges = [e + d for e in (vb, 2 * vb, vc, vc + vb) for d in (-1, 0, 1) if 0 <= e + d <= n_variants]
    ranges = [(0, n_variants), (n_variants - 1, n_variants)] + [(a, b) for a in edges for b in edges if a < b][:12]
    ranges += [tuple(sorted(rng.integers(0, n_variants + 1, 2).tolist())) for _ in range(4)]
    subsets = [np.arange(n_samples), np.array([n_samples - 1]), rng.choice(n_samples, 37, replace=False),
               np.array([0, 0, 5, 5, n_samples - 1])]                                          # duplicates count once
    for lo, hi in ranges:
        for samples in subsets:
            plan = plan_counts(samples, n_samples, sc, vc, n_variants, lo, hi, blocksize=bs)
            hits, dest = coverage(plan, n_samples, sc, vc, n_variants, lo, bs)
            want = np.zeros_like(hits)
            want[np.unique(samples), lo:hi] = 1
            assert np.array_equal(hits, want), (lo, hi)
            m = want.astype(bool)
            assert np.array_equal(dest[m], (np.nonzero(m)[1] - lo))
            assert not hits[n_samples:].any() and not hits[:, n_variants:].any()       # pad rows / pad variants
            # the selections of one chunk are adjacent, chunk columns in order
            key = plan["vcol"] * 1000 + plan["scol"]
            assert np.all(np.diff(plan["vcol"]) >= 0)
            assert len(np.unique(key)) == 1 + int(np.count_nonzero(np.diff(key)))


def test_plan_cuts_at_block_and_chunk_edges():
    for edge in (4096, 8192, 12288):
        for d in (-1, 0, 1):
            plan = plan_counts([3], 64, 64, 8192, 20_000, edge + d - 1, edge + d + 1)
            segs = sorted((int(p["vcol"]) * 8192 + int(p["part"]) * 4096 + int(p["lo"]), int(p["out_row"])) for p in plan)
            # [edge - 2, edge) and [edge, edge + 2) stay in one block, [edge - 1, edge + 1) is cut at the edge
            assert segs == ([(edge - 1, 0), (edge, 1)] if d == 0 else [(edge + d - 1, 0)])
            assert all(int(p["row_mask"]) == 1 << 3 for p in plan)


def test_plan_empty_requests():
    assert len(plan_counts([], 1000, 64, 8192, 20_000, 0, 20_000)) == 0
    assert len(plan_counts(np.arange(1000), 1000, 64, 8192, 20_000, 500, 500)) == 0
    assert len(plan_counts(np.arange(1000), 1000, 64, 8192, 0, 0, 0)) == 0


def test_plan_rejects_bad_requests():
    with pytest.raises(IndexError):
        plan_counts([1000], 1000, 64, 8192, 20_000, 0, 10)
    with pytest.raises(IndexError):
        plan_counts([0], 1000, 64, 8192, 20_000, 0, 20_001)
    with pytest.raises(ValueError):
        plan_counts([0], 1000, 128, 8192, 20_000, 0, 10)                  # more than 64 rows per chunk
    with pytest.raises(ValueError):
        plan_counts([0], 1000, 64, 8192, 20_000, 0, 10, blocksize=6000)    # rows not cut into whole blocks


def test_tsv_rows_literal():
    counts = np.zeros((4, 4), np.int64)
    counts[:, AN] = [2000, 0, 3, 1998]
    counts[:, AC] = [1, 0, 1, 1998]
    counts[:, HET] = [1, 0, 1, 0]
    counts[:, HOM_ALT] = [0, 0, 0, 999]
    text = format_rows(np.array(["chr5", "chr5", "chr5", "chrX"]), np.array([10177, 10235, 10352, 155270560]),
                       np.frombuffer(b"ACGT", np.uint8), np.array([b"G", b"T", b"A", b"C"]), counts)
    assert text == ("chr5\t10177\tA\tG\t1\t2000\t0.0005\t1\t0\n"
                    "chr5\t10235\tC\tT\t0\t0\tNA\t0\t0\n"
                    "chr5\t10352\tG\tA\t1\t3\t0.333333\t1\t0\n"
                    "chrX\t155270560\tT\tC\t1998\t1998\t1\t0\t999\n")
    assert format_rows([], [], [], [], np.zeros((0, 4))) == ""
    assert HEADER == "#CHROM\tPOS\tREF\tALT\tALT_CTS\tOBS_CT\tALT_FREQS\tHET_CT\tHOM_ALT_CT\n"


def test_region_parse():
    assert parse_region("chr5:1000-2000") == ("5", 999, 2000)
    assert parse_region("22:1,000,001-1,000,001") == ("22", 1_000_000, 1_000_001)
    for bad in ("chr5", "chr5:0-10", "chr5:20-10"):
        with pytest.raises(Exception):
            parse_region(bad)
