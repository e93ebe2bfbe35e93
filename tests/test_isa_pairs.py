"""CPU: the gfx950 code of k_pair_counts (csrc/pairs.hip, cross-compiled, no GPU needed): its 80 counters and operands
stay in registers (no scratch, no spill), the register count leaves four waves per SIMD, the inner loop holds
v_bcnt_u32_b32 fed by 16-byte LDS reads, no atomics, and its LDS lets four workgroups share a compute unit (DESIGN.md
§6a f-7: 4 x 32.5 KiB of 160 KiB)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pairs_asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "haplohyped_varawareml_amd", "csrc", "pairs.hip")
    out = tmp_path_factory.mktemp("isa") / "pairs.s"
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


def test_pair_counts_isa(pairs_asm):
    body = kernel_body(pairs_asm, "k_pair_counts")
    meta = kernel_meta(pairs_asm, "k_pair_counts")
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0
    assert "scratch_" not in body
    assert meta["vgpr_count"] <= 128, meta["vgpr_count"]                # 512 / 128: four waves per SIMD, one workgroup each
    assert meta["max_flat_workgroup_size"] == 256
    assert 4 * meta["group_segment_fixed_size"] <= 160 * 1024           # four workgroups per compute unit
    assert "atomic" not in body
    for flat in ("flat_load", "flat_store"):
        assert flat not in body, flat
    # the inner loop: the basic block that holds the popcounts and branches back to its own label
    parts = re.split(r"^(\.LBB\d+_\d+):", body, flags=re.M)
    inner = [text for label, text in zip(parts[1::2], parts[2::2])
             if "v_bcnt_u32_b32" in text and re.search(rf"s_cbranch_\w+ {re.escape(label)}\s*$", text, re.M)]
    assert len(inner) == 1, len(inner)
    n_bcnt, n_read = len(re.findall(r"\bv_bcnt_u32_b32\b", inner[0])), len(re.findall(r"\bds_read_b128\b", inner[0]))
    assert n_bcnt and n_bcnt % 80 == 0 and n_read * 80 == n_bcnt * 8, (n_bcnt, n_read)   # per word: 80 popcounts, 8 reads
    assert not re.search(r"\b(global|buffer)_(load|store)", inner[0])
