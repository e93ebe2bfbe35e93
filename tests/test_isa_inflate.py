"""CPU: the register budget of the device inflater (csrc/inflate.hip), checked on the gfx950 assembly hipcc emits
(cross-compiled, no GPU needed).  k_inflate_members is compiled for seven workgroups per CU (INF_WGS): at most 72
VGPRs per lane, and the measured 198 -> 210 GB/s of text rests on that occupancy.  Scratch (SGPR spills that did not fit
in VGPR lanes) stays at or below the 36 bytes per lane of the kernel this check was written against."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "haplohyped_varawareml_amd", "csrc", "inflate.hip")


@pytest.fixture(scope="module")
def inflate_asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "inflate.s"
    r = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.dirname(SRC), "-S", "--cuda-device-only", "-o", str(out), SRC],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def kernel_meta(asm, name):
    """the metadata entry (amdhsa.kernels) of the kernel whose symbol contains `name` -> {field: int}"""
    meta = asm[asm.index("amdhsa.kernels"):]
    for entry in re.split(r"\n  - ", meta)[1:]:
        m = re.search(r"\.name:\s+(\S+)", entry)
        if m and name in m.group(1):
            return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    raise AssertionError(f"no kernel {name} in the metadata")


def test_inflate_kernel_fits_seven_workgroups_per_cu(inflate_asm):
    m = kernel_meta(inflate_asm, "k_inflate_members")
    assert m["vgpr_count"] <= 72, m
    assert m["private_segment_fixed_size"] <= 36, m
    assert m["max_flat_workgroup_size"] == 256, m


def test_crc_kernel_keeps_out_of_scratch(inflate_asm):
    m = kernel_meta(inflate_asm, "k_crc32_members")
    assert m["private_segment_fixed_size"] == 0, m
