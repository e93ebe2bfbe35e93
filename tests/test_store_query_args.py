"""CPU: what GenotypeStore's six queries make of bad arguments — read_windows, allele_counts, sample_counts, pair_counts,
ld_counts, ld_prune, all through store_plan.query_args — on a store that is metadata only (no chunk is ever read, no
device touched: every call below fails at its arguments).  The exception types and texts are those each query raised when
it still checked its arguments itself; and the sample index arrays query_args returns."""
import json
import types

import numpy as np
import pytest

from haplohyped_varawareml_amd.store import MAX_PAIR_TABLE_BYTES, GenotypeStore, _table_budget, query_args

SAMPLES = [f"s{i}" for i in range(5)]
BOTH = ["chr_1", "chr_2"]


@pytest.fixture(scope="module")
def st(tmp_path_factory):
    d = tmp_path_factory.mktemp("meta_only")
    g = lambda n: dict(n_variants=n, n_vcol=-(-n // 8), n_scol=3, n_chunks=3 * -(-n // 8))
    json.dump(dict(format="hhgt-store", samples=SAMPLES, sc=2, vc=8, typesize=2, blocksize=16,
                   groups={"chr_1": g(20), "chr_2": g(5)}), open(d / "meta.json", "w"))
    return GenotypeStore(str(d), ctx=types.SimpleNamespace(device="cpu"))


# each query called with (group or groups, samples, v_lo, v_hi, variant_mask); read_windows takes one sample and no mask,
# allele_counts no mask
CALL = dict(
    read_windows=lambda st, g, s, lo, hi, m: st.read_windows([(g, (s or ["s0"])[0], lo, 20 if hi is None else hi)]),
    allele_counts=lambda st, g, s, lo, hi, m: st.allele_counts(g, s, lo, hi),
    sample_counts=lambda st, g, s, lo, hi, m: st.sample_counts(g, s, lo, hi, variant_mask=m),
    pair_counts=lambda st, g, s, lo, hi, m: st.pair_counts(g, s, lo, hi, variant_mask=m),
    ld_counts=lambda st, g, s, lo, hi, m: st.ld_counts(g, s, lo, hi, variant_mask=m),
    ld_prune=lambda st, g, s, lo, hi, m: st.ld_prune(g, s, lo, hi, variant_mask=m))
SIX, MANY, LD = tuple(CALL), ("sample_counts", "pair_counts"), ("ld_counts", "ld_prune")
ONE_GROUP = tuple(q for q in SIX if q not in MANY)
MASKED = MANY + LD

# (the queries it holds for, the arguments, the exception, its text; {who} is the query's name)
CASES = [
    (SIX, ("chr_1", None, 3, 21, None), IndexError, "variants [3, 21) outside chr_1 (0..20)"),
    (SIX, ("chr_1", ["s1"], 5, 4, None), IndexError, "variants [5, 4) outside chr_1 (0..20)"),
    (SIX, ("chr_1", ["s1"], -1, 4, None), IndexError, "variants [-1, 4) outside chr_1 (0..20)"),
    (SIX, ("chr_1", ["nobody", "s1"], 0, 4, None), KeyError, "'nobody'"),
    (SIX, ("chr_1", [5], 0, 4, None), IndexError, "sample 5 out of range (0..4)"),
    (SIX, ("chr_9", None, 0, None, None), KeyError, "'chr_9'"),
    # v_lo / v_hi with several groups: the queries over one group take a list for no group at all
    (MANY, (BOTH, None, 1, None, None), ValueError, "{who}: v_lo / v_hi need a single group"),
    (MANY, (BOTH, None, 0, 5, None), ValueError, "{who}: v_lo / v_hi need a single group"),
    (LD, (BOTH, None, 1, None, None), KeyError, "['chr_1', 'chr_2']"),
    (("read_windows", "allele_counts"), (BOTH, None, 1, None, None), TypeError, "unhashable type: 'list'"),
    (MANY, (BOTH, None, 0, None, np.ones(20, bool)), ValueError,
     "{who}: one variant_mask needs a single group (several: a dict group -> mask)"),
    # a mask of the wrong length
    (MASKED, ("chr_1", None, 0, None, np.ones(7, bool)), ValueError, "variant_mask of chr_1: shape (7,), expected (20,)"),
    (MASKED, ("chr_1", None, 2, 9, np.ones(20, bool)), ValueError, "variant_mask of chr_1: shape (20,), expected (7,)"),
    (MASKED, ("chr_1", None, 0, None, np.ones((20, 1), bool)), ValueError,
     "variant_mask of chr_1: shape (20, 1), expected (20,)"),
    (MANY, (BOTH, None, 0, None, {"chr_2": np.ones(4, bool)}), ValueError,
     "variant_mask of chr_2: shape (4,), expected (5,)"),
    # a dict mask that names a foreign group; the LD queries take one mask, which a dict is not
    (MANY, ("chr_1", None, 0, None, {"chr_2": np.ones(5, bool)}), KeyError, "'chr_2'"),
    (LD, ("chr_1", None, 0, None, {"chr_2": np.ones(5, bool)}), AttributeError, "'dict' object has no attribute 'ndim'"),
]


@pytest.mark.parametrize("who", SIX)
def test_bad_arguments_raise_what_they_raised(st, who):
    n = 0
    for queries, args, exc, text in CASES:
        if who in queries:
            with pytest.raises(exc) as e:
                CALL[who](st, *args)
            assert type(e.value) is exc and str(e.value) == text.format(who=who), (who, args)
            n += 1
    assert n >= 7


def test_window_and_r2_come_with_the_query_name(st):
    for who in LD:
        with pytest.raises(ValueError) as e:
            getattr(st, who)("chr_1", window=0)
        assert str(e.value) == f"{who}: window 0 (1 to 1024)"
    with pytest.raises(ValueError) as e:
        st.ld_prune("chr_1", r2=1.5)
    assert str(e.value) == "ld_prune: r2 1.5 (0 to 1)"


def test_sample_indices_and_group_ranges(st):
    index = {s: i for i, s in enumerate(SAMPLES)}
    for single in (False, True):
        idx, q = query_args(st.meta, index, "x", "chr_1", None, 0, None, None, single=single)
        assert idx.dtype.kind == "i" and idx.tolist() == [0, 1, 2, 3, 4] and q == [("chr_1", 0, 20, 20, None)]
        idx, q = query_args(st.meta, index, "x", "chr_1", ["s3", 0, "s3", 4, 0], 2, 9, None, single=single)
        assert idx.dtype == np.int64 and idx.tolist() == [3, 0, 3, 4, 0] and q == [("chr_1", 2, 9, 20, None)]   # as named
        idx, q = query_args(st.meta, index, "x", "chr_2", [], 5, 5, None, single=single)
        assert idx.dtype == np.int64 and idx.shape == (0,) and q == [("chr_2", 5, 5, 5, None)]
    assert st._query("x", "chr_1", ["s3", 0])[0].tolist() == [3, 0]
    # several groups: each whole, in the order asked (None: the store's); a dict mask goes to its group, as given
    m = np.ones(5, bool)
    idx, q = query_args(st.meta, index, "x", None, [1], 0, None, {"chr_2": m})
    assert idx.tolist() == [1] and q[0] == ("chr_1", 0, 20, 20, None) and q[1][:4] == ("chr_2", 0, 5, 5) and q[1][4] is m
    assert [x[0] for x in query_args(st.meta, index, "x", ["chr_2", "chr_1"])[1]] == ["chr_2", "chr_1"]
    m = np.ones(7, bool)
    assert query_args(st.meta, index, "x", "chr_1", None, 2, 9, m)[1][0][4] is m


def test_table_budget():
    for given, limit in ((1000, 1000), (None, MAX_PAIR_TABLE_BYTES)):
        _table_budget("q", "a table of 5 x 5 pairs ({} bytes) exceeds", limit, given)
        with pytest.raises(ValueError, match="max_table_bytes") as e:
            _table_budget("q", "a table of 5 x 5 pairs ({} bytes) exceeds", limit + 1, given)
        assert str(e.value) == f"q: a table of 5 x 5 pairs ({limit + 1} bytes) exceeds max_table_bytes = {limit}"


def test_table_budget_messages_of_the_three_queries(st):
    # 5 samples at sc = 2: 3 chunk rows, 6 plane rows; the budget fails before any device is asked for
    for who, text in (("pair_counts", "pair_counts: a table of 6 x 6 pairs (576 bytes) exceeds max_table_bytes = 575"),
                      ("grm_sums", "grm_sums: tables of 6 x 6 pairs (864 bytes) exceed max_table_bytes = 863")):
        with pytest.raises(ValueError) as e:
            getattr(st, who)("chr_1", max_table_bytes=int(text.split("= ")[1]))
        assert str(e.value) == text
