"""CPU: what the eight waves per SIMD of k_lz4_bitplanes_uni rest on (DESIGN.md §3.2 "One plane per workgroup"), read from
the metadata of the cross-compiled kernel: one wave per workgroup, at most 64 VGPRs (512 / 8), no spills, no scratch, and at
most 5120 bytes of static LDS (163 840 / 32 workgroups per CU) — for every instantiation.  tests/test_isa_counts.py holds
the same kernels to the budget of the two-wave form; this is the tighter line the single-wave form runs on."""
import pytest

from tests.test_isa_counts import BP_BUDGET, gfx950_asm, kernel_meta

UNI = sorted((d, lazy) for (kernel, d, lazy) in BP_BUDGET if kernel == "k_lz4_bitplanes_uni")


@pytest.fixture(scope="module")
def lz4bits_asm(tmp_path_factory):
    return gfx950_asm(tmp_path_factory, "lz4bits")


@pytest.mark.parametrize("depth,lazy", UNI)
def test_a_plane_fits_32_times_into_a_cu(lz4bits_asm, depth, lazy):
    meta = kernel_meta(lz4bits_asm, f"k_lz4_bitplanes_uniILi{depth}ELb{int(lazy)}EE")
    print(f"k_lz4_bitplanes_uni<{depth}, {str(lazy).lower()}>: {meta['vgpr_count']} VGPRs, "
          f"{meta['group_segment_fixed_size']} B static LDS, workgroup of {meta['max_flat_workgroup_size']}")
    assert meta["max_flat_workgroup_size"] == 64
    assert meta["vgpr_count"] <= 64, meta["vgpr_count"]
    assert (meta["vgpr_spill_count"], meta["private_segment_fixed_size"]) == (0, 0)
    assert meta["group_segment_fixed_size"] <= 5120, meta["group_segment_fixed_size"]
