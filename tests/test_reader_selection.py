"""CPU: the three helpers VCFH5Reader's queries share — _variant_masks (which variants take part: the calls it makes of
GenotypeStore.variant_mask and ld_prune, their arguments and their order), _variant_columns (the variant columns of a
record array against columns written out by hand) and _donor_column — on a fake store that records what it is asked."""
import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd.h5_reader import VCFH5Reader

RUNS = [[0, "1"], [3, "chr1_alt"], [5, "1"]]
START = np.array([10, 20, 30, 40, 50, 60, 70], np.uint32)
REF, ALT = np.frombuffer(b"ACGTACG", np.uint8), np.frombuffer(b"CGTACGT", np.uint8)
CHROM = [b"1", b"1", b"1", b"chr1_alt", b"chr1_alt", b"1", b"1"]


class FakeStore:
    def __init__(self):
        self.samples = ["a", "b", "c"]
        self.meta = dict(groups={"chr_1": dict(n_variants=7), "chr_2": dict(n_variants=7)})
        self.calls = []

    def groups(self):
        return list(self.meta["groups"])

    def variants(self, group):
        return START, REF, ALT, RUNS

    # (GenotypeStore's signatures; a call is recorded as the arguments it amounts to)
    def variant_mask(self, group, samples=None, v_lo=0, v_hi=None, min_maf=None, max_ac=None, min_ac=None):
        self.calls.append(("variant_mask", group, samples, v_lo, v_hi, min_maf, min_ac, max_ac))
        self.mask = np.ones(7, bool) if len(self.calls) % 2 else torch.ones(7, dtype=torch.bool)
        return self.mask

    def ld_prune(self, group, samples=None, v_lo=0, v_hi=None, variant_mask=None, window=50, r2=0.2):
        self.calls.append(("ld_prune", group, samples, v_lo, v_hi, variant_mask, window, r2))
        self.kept = torch.zeros(7, dtype=torch.bool)
        return self.kept


@pytest.fixture
def reader():
    r = VCFH5Reader.__new__(VCFH5Reader)
    r.store = FakeStore()
    return r


def mask_call(group, who, lo=0, hi=None, min_maf=None, ac=None):
    return ("variant_mask", group, who, lo, hi, min_maf, ac, ac)


def test_no_filter_no_call(reader):
    assert reader._variant_masks(["chr_1", "chr_2"], None) == {}
    assert reader._variant_masks(["chr_1"], ["a"], spans={"chr_1": (1, 3)}, ld_r2=0.5) == {}
    assert reader.store.calls == []


def test_min_maf_and_singletons(reader):
    who = ["b", "a"]
    masks = reader._variant_masks(["chr_1"], who, min_maf=0.05)
    assert list(masks) == ["chr_1"] and masks["chr_1"] is reader.store.mask
    masks = reader._variant_masks(["chr_1"], who, singletons=True)
    assert masks["chr_1"] is reader.store.mask
    reader._variant_masks(["chr_1"], who, min_maf=0.1, singletons=True)
    assert reader.store.calls == [mask_call("chr_1", who, min_maf=0.05), mask_call("chr_1", who, ac=1),
                                  mask_call("chr_1", who, min_maf=0.1, ac=1)]
    assert all(c[2] is who for c in reader.store.calls)


def test_ld_window_alone_prunes_every_variant(reader):
    masks = reader._variant_masks(["chr_1"], None, ld_window=30)
    assert reader.store.calls == [("ld_prune", "chr_1", None, 0, None, None, 30, 0.2)]
    assert masks == {"chr_1": reader.store.kept} and masks["chr_1"] is reader.store.kept


def test_ld_prune_takes_the_mask_itself(reader):
    masks = reader._variant_masks(["chr_1"], ["c"], min_maf=0.01, ld_window=50, ld_r2=0.4)
    first, (name, group, who, v_lo, v_hi, mask, window, r2) = reader.store.calls
    assert first == mask_call("chr_1", ["c"], min_maf=0.01) and mask is reader.store.mask
    assert (name, group, who, v_lo, v_hi, window, r2) == ("ld_prune", "chr_1", ["c"], 0, None, 50, 0.4)
    assert masks["chr_1"] is reader.store.kept


def test_spans_reach_variant_mask(reader):
    reader._variant_masks(["chr_1"], None, spans={"chr_1": (2, 6)}, min_maf=0.2)
    reader._variant_masks(["chr_2"], None, spans={"chr_1": (2, 6)}, min_maf=0.2)
    assert reader.store.calls == [mask_call("chr_1", None, 2, 6, min_maf=0.2), mask_call("chr_2", None, min_maf=0.2)]


@pytest.mark.parametrize("who", [None, ["c", "a"]])
def test_two_groups_one_sequence_each_in_the_order_asked(reader, who):
    masks = reader._variant_masks(["chr_2", "chr_1"], who, min_maf=0.05, ld_window=10)
    assert list(masks) == ["chr_2", "chr_1"]
    assert [c[:2] for c in reader.store.calls] == [("variant_mask", "chr_2"), ("ld_prune", "chr_2"),
                                                   ("variant_mask", "chr_1"), ("ld_prune", "chr_1")]
    assert all(c[2] is who for c in reader.store.calls)


def want_columns(at, width, pos):
    return (np.array([CHROM[i][:width] for i in at], f"S{width}"), START[at].astype(np.int64) + (1 if pos else 0),
            np.array([b"ACGTACG"[i:i + 1] for i in at], "S10"), np.array([b"CGTACGT"[i:i + 1] for i in at], "S10"))


@pytest.mark.parametrize("pos", [False, True])
@pytest.mark.parametrize("how", ["slice", "at"])
@pytest.mark.parametrize("width", [8, 3])
def test_variant_columns(reader, how, pos, width):
    at = [2, 3, 4, 5] if how == "slice" else [0, 3, 6]
    dtype = [("chrom", f"S{width}"), ("pos" if pos else "start", np.uint32), ("ref", "S10"), ("alt", "S10"), ("x", np.int32)]
    rec = np.zeros(len(at), dtype=dtype)
    rec["x"] = 7
    if how == "slice":
        reader._variant_columns(rec, reader.store.variants("chr_1"), width, lo=2, hi=6, pos=pos)
    else:
        reader._variant_columns(rec, reader.store.variants("chr_1"), width, at=np.array(at), pos=pos)
    chrom, where, ref, alt = want_columns(at, width, pos)
    assert np.array_equal(rec["chrom"], chrom) and np.array_equal(rec["pos" if pos else "start"], where)
    assert np.array_equal(rec["ref"], ref) and np.array_equal(rec["alt"], alt) and (rec["x"] == 7).all()
    if width == 3:
        assert rec["chrom"].tolist()[1] == b"chr"


def test_variant_columns_fill_stop_where_the_records_have_one(reader):
    rec = np.zeros(7, dtype=[("chrom", "S8"), ("start", np.uint32), ("stop", np.uint32), ("ref", "S10"), ("alt", "S10")])
    reader._variant_columns(rec, reader.store.variants("chr_1"), 8)
    assert rec["chrom"].tolist() == CHROM and rec["start"].tolist() == START.tolist()
    assert rec["stop"].tolist() == (START + 1).tolist() and rec["ref"].tolist() == [b"A", b"C", b"G", b"T", b"A", b"C", b"G"]


def test_donor_column(reader):
    empty = reader._donor_column([])
    assert empty.dtype == np.dtype("S1") and empty.shape == (0,)
    names = ["NA12878", "Zoë", "日本"]
    col = reader._donor_column(names)
    assert col.dtype == np.dtype("S7") and col.tolist() == [x.encode() for x in names]
    assert reader._donor_column(["日本語の名前"]).dtype == np.dtype(f"S{len('日本語の名前'.encode())}") == np.dtype("S18")
