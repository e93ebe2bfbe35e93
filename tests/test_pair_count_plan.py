"""CPU: store.plan_planes (the selections of GenotypeStore.pair_counts' first stage) against a brute-force restatement —
every selected (sample, counted block) owned by exactly one selection, plane rows compacted by chunk row, out_word by
block —, store.plane_windows, the kinship and identity-by-state arithmetic on hand-made tables and against a brute-force
count on random genotypes with missing, half-missing and allele-2/3 calls (numpy only), and the kinship TSV formatter."""
import numpy as np
import pytest

from haplohyped_varawareml_amd.kinship import HEADER, format_rows
from haplohyped_varawareml_amd.store import (HET1, HETHET, IBS0, NSNP, ibs_counts, kinship_from_counts, mask_words_per_block,
                                             plan_counts, plan_planes, plane_rows, plane_windows)
from tests.test_gpu_allele_counts import GEOMS

SHARED = ("vcol", "scol", "part", "row_mask", "lo", "hi")


def check_plan(samples, n_samples, sc, vc, n_variants, v_lo, v_hi, bs, block0=None):
    plan = plan_planes(samples, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize=bs, block0=block0)
    cut = plan_counts(samples, n_samples, sc, vc, n_variants, v_lo, v_hi, blocksize=bs)
    assert len(plan) == len(cut)
    for f in SHARED:
        assert np.array_equal(plan[f], cut[f]), f
    vb, wpb = bs // 2, mask_words_per_block(bs)
    first = v_lo // vb if block0 is None else block0
    uniq = np.unique(np.asarray(samples, np.int64))
    scols, rows = plane_rows(uniq, sc)
    blocks = range(v_lo // vb, (v_hi - 1) // vb + 1) if v_hi > v_lo and len(uniq) else range(0)
    assert len(plan) == len(scols) * len(blocks)                       # nothing but the selections found below
    for s, row in zip(uniq.tolist(), rows.tolist()):
        for B in blocks:
            vcol, part = B * vb // vc, (B * vb % vc) // vb
            own = [p for p in plan if p["scol"] == s // sc and p["vcol"] == vcol and p["part"] == part
                   and int(p["row_mask"]) >> (s % sc) & 1]
            assert len(own) == 1, (s, B)
            p = own[0]
            assert (int(p["lo"]), int(p["hi"])) == (max(v_lo, B * vb) - B * vb, min(v_hi, (B + 1) * vb) - B * vb)
            assert int(p["out_row"]) + s % sc == row
            assert int(p["out_word"]) == (B - first) * wpb and int(p["mask_word"]) == B * wpb
    return plan


@pytest.mark.parametrize("sc,vc,bs", GEOMS)
def test_plan_planes_brute_force(sc, vc, bs):
    rng = np.random.default_rng(sc + vc + bs)
    n_samples, n_variants = 5 * sc + 7, 3 * vc + vc // 3
    vb = bs // 2
    edges = [e + d for e in (vb, vc, vc + vb) for d in (-1, 0, 1) if 0 <= e + d <= n_variants]
    ranges = [(0, n_variants), (n_variants - 1, n_variants), (vb // 2 + 1, n_variants - vb // 3)]
    ranges += [(a, b) for a in edges for b in edges if a < b][:6]
    subsets = [np.arange(n_samples), np.array([n_samples - 1]), rng.choice(n_samples, 9, replace=False),
               np.array([0, 0, 3 * sc + 1, 3 * sc + 1, sc - 1])]                    # skips chunk rows; names twice
    for v_lo, v_hi in ranges:
        for samples in subsets:
            check_plan(samples, n_samples, sc, vc, n_variants, v_lo, v_hi, bs)
    check_plan(subsets[2], n_samples, sc, vc, n_variants, vc + 5, 2 * vc, bs, block0=1)
    with pytest.raises(IndexError):
        plan_planes(subsets[2], n_samples, sc, vc, n_variants, 0, vc, blocksize=bs, block0=1)


def test_plane_rows_compact_by_chunk_row():
    scols, rows = plane_rows([5, 900, 5, 64, 130], 64)
    assert scols.tolist() == [0, 1, 2, 14] and rows.tolist() == [5, 3 * 64 + 900 % 64, 5, 64, 128 + 2]
    scols, rows = plane_rows(np.arange(2504)[::251], 64)                 # 10 samples of 2504: at most 10 chunk rows
    assert len(scols) <= 10 and len(set(rows.tolist())) == 10 and rows.max() < len(scols) * 64
    scols, rows = plane_rows([], 64)
    assert len(scols) == 0 and len(rows) == 0


def test_plan_empty_inputs():
    assert len(plan_planes([], 1000, 64, 8192, 20_000, 0, 20_000)) == 0
    assert len(plan_planes(np.arange(1000), 1000, 64, 8192, 20_000, 500, 500)) == 0
    assert len(plan_planes(np.arange(1000), 1000, 64, 8192, 0, 0, 0)) == 0
    assert plane_windows(7, 7, 8192, 64, 1 << 20) == []


@pytest.mark.parametrize("bs,n_rows,budget", [(8192, 64, 1 << 30), (8192, 128, 3 * 128 * 128 * 4 * 2), (8192, 128, 1),
                                             (64, 20, 3 * 20 * 4 * 5), (96, 40, 3 * 40 * 8 * 3 + 5)])
def test_plane_windows_cover_once_at_block_boundaries(bs, n_rows, budget):
    vb, wpb = bs // 2, mask_words_per_block(bs)
    for v_lo, v_hi in ((0, 11 * vb + 5), (vb // 2 + 1, 7 * vb - 3), (3 * vb, 4 * vb), (vb - 1, vb + 1)):
        wins = plane_windows(v_lo, v_hi, bs, n_rows, budget)
        assert wins[0][0] == v_lo and wins[-1][1] == v_hi
        for (a, b), (c, _) in zip(wins, wins[1:] + [(v_hi, None)]):
            assert a < b and b == c                                        # in order, no gap, no overlap
            assert b == v_hi or b % vb == 0                                # cut at block boundaries only
            n_blocks = (b - 1) // vb - a // vb + 1
            assert n_blocks == 1 or 3 * n_rows * n_blocks * wpb * 4 <= budget


# ---- the arithmetic ------------------------------------------------------------------------------------------------------
def np_pair_table(g):
    """int8 [S, V, 2] -> int64 [S, S, 4]: the contract, restated"""
    a, b = g[..., 0], g[..., 1]
    done = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
    het = (done & (a != b)).astype(np.float64)                            # (float64 products of 0 / 1: exact below 2^53)
    ref = (done & (a == 0) & (b == 0)).astype(np.float64)
    alt = (done & (a == 1) & (b == 1)).astype(np.float64)
    m = done.astype(np.float64)
    t = np.zeros((g.shape[0], g.shape[0], 4), np.int64)
    t[..., NSNP] = m @ m.T
    t[..., HETHET] = het @ het.T
    t[..., IBS0] = ref @ alt.T + alt @ ref.T
    t[..., HET1] = het @ m.T
    return t


def random_genotypes(rng, S, V):
    g = (rng.random((S, V, 2)) < 0.3).astype(np.int8)
    g[rng.random((S, V, 2)) < 0.03] = -9                                   # half-missing (and, by chance, missing)
    g[rng.random((S, V)) < 0.02] = -9                                      # missing
    g[rng.random((S, V, 2)) < 0.02] = 2
    g[rng.random((S, V, 2)) < 0.01] = 3
    return g


def test_ibs_identity_against_brute_force():
    rng = np.random.default_rng(3)
    g = random_genotypes(rng, 12, 700)
    g[7] = g[2]                                                            # a duplicate
    assert all((g == x).any() for x in (0, 1, -9, 2, 3)) and ((g[..., 0] == -9) != (g[..., 1] == -9)).any()
    t = np_pair_table(g)
    for col in (NSNP, HETHET, IBS0):
        assert np.array_equal(t[..., col], t[..., col].T)
    ibs0, ibs1, ibs2 = ibs_counts(t)
    a, b = g[..., 0].astype(np.int64), g[..., 1].astype(np.int64)
    done = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
    dose = a + b
    for i in range(len(g)):
        for j in range(len(g)):
            both = done[i] & done[j]
            diff = np.abs(dose[i] - dose[j])[both]
            assert (int(ibs0[i, j]), int(ibs1[i, j]), int(ibs2[i, j])) == (int((diff == 2).sum()), int((diff == 1).sum()),
                                                                           int((diff == 0).sum())), (i, j)
    phi = kinship_from_counts(t)
    assert phi.dtype == np.float64 and phi[2, 7] == 0.5 and phi[7, 2] == 0.5 and (np.diag(phi) == 0.5).all()
    assert np.array_equal(phi, phi.T)
    import torch
    assert np.array_equal(kinship_from_counts(torch.from_numpy(t)).numpy(), phi)
    assert all(np.array_equal(x.numpy(), y) for x, y in zip(ibs_counts(torch.from_numpy(t.astype(np.int32))), (ibs0, ibs1, ibs2)))


def test_kinship_hand_made():
    t = np.zeros((3, 3, 4), np.int64)
    # samples 0 and 1: 100 shared variants, 20 / 30 heterozygotes, 10 both, 4 opposite homozygotes; sample 2 has no HET
    t[0, 0], t[1, 1], t[2, 2] = (100, 20, 0, 20), (100, 30, 0, 30), (90, 0, 0, 0)
    t[0, 1], t[1, 0] = (100, 10, 4, 20), (100, 10, 4, 30)
    t[0, 2], t[2, 0] = (90, 0, 7, 18), (90, 0, 7, 0)
    t[1, 2], t[2, 1] = (90, 0, 9, 25), (90, 0, 9, 0)
    phi = kinship_from_counts(t)
    assert phi[0, 0] == 0.5 and phi[1, 1] == 0.5
    assert phi[0, 1] == phi[1, 0] == 0.5 - (4 * 4 + 20 + 30 - 2 * 10) / (4.0 * 20)
    assert np.isnan(phi[2, 2]) and np.isnan(phi[0, 2]) and np.isnan(phi[2, 1])          # min(HET1) = 0
    ibs0, ibs1, ibs2 = ibs_counts(t)
    assert ibs2[0, 1] == 2 * 10 + 100 - 20 - 30 - 4 and ibs1[0, 1] == 100 - 4 - ibs2[0, 1] and ibs0[0, 1] == 4
    assert ibs2[0, 0] == 100 and ibs1[0, 0] == 0


def test_tsv_rows_literal():
    rec = np.zeros(3, dtype=[("sample1", "S7"), ("sample2", "S7"), ("nsnp", np.int64), ("hethet", np.int64),
                             ("ibs0", np.int64), ("het1", np.int64), ("het2", np.int64), ("kinship", np.float64)])
    rec[0] = (b"HG00096", b"HG00097", 1000, 10, 4, 20, 30, 0.5 - 46 / 80.0)
    rec[1] = (b"HG00096", b"s3", 90, 0, 7, 18, 0, np.nan)
    rec[2] = (b"a", b"b", 123456, 500, 0, 500, 500, 0.5)
    assert format_rows(rec) == ("HG00096\tHG00097\t1000\t10\t4\t20\t30\t-0.075\n"
                                "HG00096\ts3\t90\t0\t7\t18\t0\tnan\n"
                                "a\tb\t123456\t500\t0\t500\t500\t0.5\n")
    assert format_rows(rec[:0]) == ""
    assert HEADER == "#IID1\tIID2\tNSNP\tHETHET\tIBS0\tHET1\tHET2\tKINSHIP\n"
