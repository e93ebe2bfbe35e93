"""CPU: store_plan.plan_rows — the one cut behind plan_counts, plan_sample_counts and plan_planes — against the records the
three planners gave when each made its own, restated here by brute force (a loop over chunk columns, chunk rows and
blocks; nothing of the code under test), field for field and in order; and through the brute-force checks the planners'
own tests keep (coverage of tests/test_allele_count_plan.py, check_plan of tests/test_pair_count_plan.py)."""
import numpy as np
import pytest

from haplohyped_varawareml_amd.store import plan_counts, plan_planes, plan_rows, plan_sample_counts
from tests.test_allele_count_plan import coverage
from tests.test_pair_count_plan import check_plan

CUT = ("vcol", "scol", "part", "row_mask", "lo", "hi")
ALL = CUT + ("out_row", "mask_word", "out_word")


def brute(kind, samples, sc, vc, v_lo, v_hi, bs, block0=None):
    """the selections as tuples in the order of ALL: chunk columns in order, within one the chunk rows that hold a listed
    sample, within a chunk the blocks the range touches; out_row by `kind` (plan_rows' out_row)"""
    vb = bs // 2
    wpb = -(-vb // 32)
    uniq = sorted(set(int(s) for s in samples))
    scols = sorted({s // sc for s in uniq})
    first = v_lo // vb if block0 is None else block0
    recs = []
    for vcol in range(v_lo // vc, (v_hi - 1) // vc + 1) if v_hi > v_lo else ():
        for k, scol in enumerate(scols):
            mask = sum(1 << (s % sc) for s in uniq if s // sc == scol)
            for part in range(vc // vb):
                B = vcol * (vc // vb) + part
                lo, hi = max(v_lo, B * vb), min(v_hi, (B + 1) * vb)
                if lo < hi:
                    out_row = {"variant": lo - v_lo, "sample": scol * sc, "plane": k * sc}[kind]
                    recs.append((vcol, scol, part, mask, lo - B * vb, hi - B * vb, out_row, B * wpb, (B - first) * wpb))
    return recs


def rows_of(plan, fields):
    return [tuple(int(p[f]) for f in fields) for p in plan]


@pytest.mark.parametrize("bs", [64, 8192])
@pytest.mark.parametrize("vc", [4096, 8192])
@pytest.mark.parametrize("sc", [1, 3, 64])
def test_one_cut_gives_the_three_plans(sc, vc, bs):
    rng = np.random.default_rng(sc + vc + bs)
    vb = bs // 2
    n_samples, n_variants = 2 * sc + 1, 2 * vc + vc // 3
    ranges = [(0, n_variants), (max(vc - vb - 3, 1), vc + vb + 5), (vc - 1, vc + 1), (vb // 2, vb // 2 + 3),  # mid-block ends,
              (vc, 2 * vc), (n_variants - 1, n_variants), (7, 7)]                            # across a chunk column; empty
    subsets = [np.arange(n_samples), np.array([n_samples - 1, 0, 0, n_samples - 1]), rng.choice(n_samples, 2, replace=False),
               np.array([], np.int64)]
    geom = (n_samples, sc, vc, n_variants)
    for v_lo, v_hi in ranges:
        for samples in subsets:
            args = (samples,) + geom + (v_lo, v_hi)
            for kind, plan, fields in (("variant", plan_counts(*args, blocksize=bs), CUT + ("out_row",)),
                                       ("sample", plan_sample_counts(*args, blocksize=bs), CUT + ("out_row", "mask_word")),
                                       ("plane", plan_planes(*args, blocksize=bs), ALL)):
                want = brute(kind, samples, sc, vc, v_lo, v_hi, bs)
                n = len(fields)
                assert rows_of(plan, fields) == [w[:n] for w in want], (kind, v_lo, v_hi)
                assert rows_of(plan_rows(*args, blocksize=bs, out_row=kind), ALL) == want, (kind, v_lo, v_hi)
                assert (len(want) == 0) == (len(samples) == 0 or v_hi == v_lo)
    # a plane buffer that begins before the range: block0 before the block of v_lo, and the first block of all
    v_lo, v_hi = vc + vb // 2, 2 * vc
    for block0 in (v_lo // vb - 1, 0):
        plan = plan_planes(subsets[1], *geom, v_lo, v_hi, blocksize=bs, block0=block0)
        assert rows_of(plan, ALL) == brute("plane", subsets[1], sc, vc, v_lo, v_hi, bs, block0)
        assert int(plan["out_word"].min()) == (v_lo // vb - block0) * -(-vb // 32)
    with pytest.raises(IndexError):
        plan_planes(subsets[1], *geom, v_lo, v_hi, blocksize=bs, block0=v_lo // vb + 1)
    # the planners' own brute-force checks, on the cut's narrow ranges (they walk every sample and block)
    for v_lo, v_hi in ranges[1:4]:
        plan = plan_rows(subsets[0], *geom, v_lo, v_hi, blocksize=bs, out_row="variant")
        hits, dest = coverage(plan, n_samples, sc, vc, n_variants, v_lo, bs)
        want = np.zeros_like(hits)
        want[:n_samples, v_lo:v_hi] = 1
        assert np.array_equal(hits, want) and np.array_equal(dest[want.astype(bool)], np.nonzero(want)[1] - v_lo)
        check_plan(subsets[1], n_samples, sc, vc, n_variants, v_lo, v_hi, bs)


def test_default_blocksize_is_one_place():
    for vc in (16, 4096, 8192):
        a = plan_rows([0], 1, 1, vc, 3 * vc, 0, 3 * vc)
        b = plan_rows([0], 1, 1, vc, 3 * vc, 0, 3 * vc, blocksize=min(vc * 2, 8192))
        assert len(a) and np.array_equal(a, b)
