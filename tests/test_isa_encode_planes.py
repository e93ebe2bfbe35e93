"""CPU: code-generation properties of k_encode_planes (csrc/encode.hip) that its measured speed depends on — checked on the
gfx950 assembly hipcc emits (cross-compiled, no GPU needed).

* four workgroups of four waves share a CU: at most 128 VGPRs per lane (512 / 4 waves per SIMD), no spills, no scratch;
* the lanes' fields come from aligned window chunks and the neighbour lane's (DPP wave_shl:1), not from 16-byte loads at
  any byte of the line.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "haplohyped_varawareml_amd", "csrc", "encode.hip")
KERNEL = "_Z15k_encode_planes"


@pytest.fixture(scope="module")
def encode_asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "encode.s"
    r = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.dirname(SRC), "-S", "--cuda-device-only", "-o", str(out), SRC],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def _meta(asm, key):
    meta = asm[asm.index("amdhsa.kernels"):]
    i = meta.index(".name:           " + KERNEL)
    # the kernel's keys sit around its .name line, inside its own list entry
    start = meta.rfind("\n  - ", 0, i)
    end = meta.find("\n  - ", i)
    chunk = meta[start:end if end > 0 else len(meta)]
    return int(re.search(r"\." + key + r":\s*(\d+)", chunk).group(1))


def _body(asm):
    m = re.search(r"^(" + KERNEL + r"\w+):\s*;.*?$", asm, re.M)
    assert m, "k_encode_planes not in the assembly"
    return asm[m.end():asm.index("s_endpgm", m.end())]


def test_four_waves_per_simd_no_scratch(encode_asm):
    vgpr = _meta(encode_asm, "vgpr_count")
    assert vgpr <= 128, vgpr
    assert _meta(encode_asm, "vgpr_spill_count") == 0
    assert _meta(encode_asm, "sgpr_spill_count") == 0
    assert _meta(encode_asm, "private_segment_fixed_size") == 0
    assert _meta(encode_asm, "group_segment_fixed_size") == 32768


def test_fields_from_aligned_window_and_neighbour_lane(encode_asm):
    body = _body(encode_asm)
    assert "scratch_" not in body
    assert re.search(r"v_mov_b32_dpp .*wave_shl:1", body), "no neighbour-lane funnel"
    assert "v_alignbyte_b32" in body
    assert "global_load_dwordx4" in body
