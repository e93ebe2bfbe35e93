"""CPU: store.plan_sample_counts (the selections of GenotypeStore.sample_counts) against store.plan_counts, whose cuts it
takes over — the cases of tests/test_allele_count_plan.py —, store.pack_variant_mask against a bit-by-bit restatement, the
sample_stats TSV formatter against literal text, the exported symbol, and the gfx950 code of k_count_samples (cross-compiled,
no GPU needed): no scratch, no more VGPRs than k_count_alleles, its row table reached with LDS instructions, integer adds
its only global atomics."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd.sample_stats import HEADER, format_rows
from haplohyped_varawareml_amd.store import (AC, AN, HET, HOM_ALT, mask_words_per_block, pack_variant_mask, plan_counts,
                                             plan_sample_counts)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = ("vcol", "scol", "part", "row_mask", "lo", "hi")


def check_against_plan_counts(samples, n_samples, sc, vc, n_variants, lo, hi, bs):
    cut = plan_counts(samples, n_samples, sc, vc, n_variants, lo, hi, blocksize=bs)
    plan = plan_sample_counts(samples, n_samples, sc, vc, n_variants, lo, hi, blocksize=bs)
    assert len(plan) == len(cut)
    for f in SHARED:
        assert np.array_equal(plan[f], cut[f]), f
    assert np.array_equal(plan["out_row"], cut["scol"] * sc)
    # the block of a selection, counted over the whole group, times the words a block owns
    vb = bs // 2
    block = (cut["vcol"] * vc + cut["part"].astype(np.int64) * vb) // vb
    assert np.array_equal(plan["mask_word"], block * -(-vb // 32))
    return plan


@pytest.mark.parametrize("n_samples,n_variants,sc,vc,bs", [
    (1000, 20_000, 64, 8192, 8192),      # 24 pad rows, a partial last chunk column
    (2504, 9000, 64, 8192, 8192),        # 2504 = 39 x 64 + 8
    (130, 1000, 64, 256, 512),           # one block per row
    (70, 700, 16, 128, 64),              # four blocks per row
])
def test_plan_is_plan_counts_with_rows_and_mask_words(n_samples, n_variants, sc, vc, bs):
    rng = np.random.default_rng(n_samples + n_variants)
    vb = bs // 2
    edges = [e + d for e in (vb, 2 * vb, vc, vc + vb) for d in (-1, 0, 1) if 0 <= e + d <= n_variants]
    ranges = [(0, n_variants), (n_variants - 1, n_variants)] + [(a, b) for a in edges for b in edges if a < b][:12]
    ranges += [tuple(sorted(rng.integers(0, n_variants + 1, 2).tolist())) for _ in range(4)]
    subsets = [np.arange(n_samples), np.array([n_samples - 1]), rng.choice(n_samples, 37, replace=False),
               np.array([0, 0, 5, 5, n_samples - 1])]                                          # duplicates count once
    for lo, hi in ranges:
        for samples in subsets:
            plan = check_against_plan_counts(samples, n_samples, sc, vc, n_variants, lo, hi, bs)
            # every selected sample has its own output row: row r of chunk row scol is sample scol * sc + r
            rows = set()
            for p in plan:
                rows |= {int(p["out_row"]) + r for r in range(64) if int(p["row_mask"]) >> r & 1}
            assert rows == set(np.unique(samples).tolist())


def test_plan_empty_requests():
    assert len(plan_sample_counts([], 1000, 64, 8192, 20_000, 0, 20_000)) == 0
    assert len(plan_sample_counts(np.arange(1000), 1000, 64, 8192, 20_000, 500, 500)) == 0
    assert len(plan_sample_counts(np.arange(1000), 1000, 64, 8192, 0, 0, 0)) == 0


@pytest.mark.parametrize("vb", [32, 48, 4096])
def test_mask_word_is_block_index_times_words_per_block(vb):
    bs, vc, sc = 2 * vb, 4 * vb, 16
    wpb = {32: 1, 48: 2, 4096: 128}[vb]
    assert mask_words_per_block(bs) == wpb
    n_variants = 11 * vb + 5
    plan = check_against_plan_counts(np.arange(40), 40, sc, vc, n_variants, 3, n_variants - 1, bs)
    first = plan[plan["scol"] == 0]
    assert np.array_equal(first["mask_word"], np.arange(12) * wpb)         # blocks 0 .. 11 of the group, in order
    assert np.array_equal(first["vcol"] * 4 + first["part"], np.arange(12))


def test_plan_rejects_what_plan_counts_rejects():
    with pytest.raises(IndexError):
        plan_sample_counts([1000], 1000, 64, 8192, 20_000, 0, 10)
    with pytest.raises(ValueError):
        plan_sample_counts([0], 1000, 128, 8192, 20_000, 0, 10)


@pytest.mark.parametrize("n_variants,vc,bs", [(20_000, 8192, 8192), (700, 128, 64), (500, 96, 96)])
def test_pack_variant_mask_bit_by_bit(n_variants, vc, bs):
    rng = np.random.default_rng(n_variants)
    vb = bs // 2
    wpb = -(-vb // 32)
    lo, hi = vb // 2 + 3, n_variants - vb // 3                 # starts and ends inside a block
    assert lo % vb and hi % vb
    mask = rng.random(hi - lo) < 0.3
    words = pack_variant_mask(mask, lo, n_variants, vc, bs)
    n_blocks = -(-n_variants // vc) * (vc // vb)
    assert words.dtype == np.uint32 and words.shape == (n_blocks * wpb,)
    want = [0] * (n_blocks * wpb)
    for v in range(lo, hi):
        if mask[v - lo]:
            block, i = divmod(v, vb)
            want[block * wpb + i // 32] |= 1 << (i % 32)
    assert words.tolist() == want
    t = pack_variant_mask(torch.from_numpy(mask), lo, n_variants, vc, bs)
    assert t.dtype == torch.int32 and np.array_equal(t.numpy().view(np.uint32), words)
    assert not pack_variant_mask(np.zeros(hi - lo, bool), lo, n_variants, vc, bs).any()
    with pytest.raises(IndexError):
        pack_variant_mask(mask, lo + 1 + n_variants - hi, n_variants, vc, bs)


def test_tsv_rows_literal():
    counts = np.zeros((3, 4), np.int64)
    counts[:, AN] = [2000, 0, 1997]
    counts[:, AC] = [31, 0, 1000]
    counts[:, HET] = [29, 0, 2]
    counts[:, HOM_ALT] = [1, 0, 499]
    text = format_rows(["HG00096", "NA12878", "s3"], 1000, counts)
    assert text == ("HG00096\t1000\t2000\t0\t31\t29\t1\n"
                    "NA12878\t1000\t0\t2000\t0\t0\t0\n"
                    "s3\t1000\t1997\t3\t1000\t2\t499\n")
    assert format_rows([], 5, np.zeros((0, 4))) == ""
    assert HEADER == "#IID\tVARIANT_CT\tOBS_CT\tMISSING_CT\tALT_CTS\tHET_CT\tHOM_ALT_CT\n"


def test_library_exports_count_samples():
    from haplohyped_varawareml_amd import build
    assert hasattr(ctypes.CDLL(build.build()), "hhgt_count_samples")


# ---- the code hipcc emits for k_count_samples ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decode_asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "haplohyped_varawareml_amd", "csrc", "decode.hip")
    out = tmp_path_factory.mktemp("isa") / "decode.s"
    r = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.dirname(src), "-S", "--cuda-device-only", "-o", str(out), src],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def kernel_body(asm, name):
    m = re.search(rf"^(_Z\d+{name}\w+):\s*;.*?$", asm, re.M)
    assert m, name
    return re.sub(r";.*", "", asm[m.end():asm.index("s_endpgm", m.end())])


def kernel_meta(asm, name):
    meta = asm[asm.index("amdhsa.kernels"):]
    entries = [e for e in meta.split("  - .agpr_count") if re.search(rf"\.name:\s+_Z\d+{name}\w+", e)]
    assert len(entries) == 1, name
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", entries[0], re.M)}


def test_count_samples_isa(decode_asm):
    body = kernel_body(decode_asm, "k_count_samples")
    mine, theirs = kernel_meta(decode_asm, "k_count_samples"), kernel_meta(decode_asm, "k_count_alleles")
    assert mine["private_segment_fixed_size"] == 0 and mine["vgpr_spill_count"] == 0
    assert "scratch_" not in body
    assert mine["vgpr_count"] <= theirs["vgpr_count"], (mine["vgpr_count"], theirs["vgpr_count"])
    # the row table (and the decoded planes) sit in LDS and are reached as such
    for flat in ("flat_load", "flat_store", "flat_atomic"):
        assert flat not in body, flat
    assert "ds_write_b64" in body and re.search(r"ds_read2?_b(64|32)", body)
    # global atomics: the 32-bit counter adds and the 64-bit n_bad add, nothing else
    atomics = set(re.findall(r"\b((?:global|buffer)_atomic_\w+)", body))
    assert atomics == {"global_atomic_add", "global_atomic_add_x2"}, atomics
    assert len(re.findall(r"\bglobal_atomic_add\b", body)) == 4              # one per counter, issued by the row's thread
    assert "v_bcnt_u32_b32" in body and "row_shr" in body                     # popcounts, DPP reduction
