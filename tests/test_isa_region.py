"""CPU: the gfx950 code of csrc/region.hip (cross-compiled, no GPU needed), metadata only: k_region_sums is the bit-sum tile
of csrc/plane_tiles.h with one column tile and one word staged at a time, as k_score_sums<1>, and must keep what two
512-thread workgroups per CU need: no spilled register, no scratch, the 12 288 bytes of LDS of that staging, and at most 128
VGPRs (4 waves per SIMD: 512 / 128).  k_region_add, one entry a thread, spills nothing either."""
import pytest

from tests.test_isa_counts import gfx950_asm, kernel_meta, meta_line


@pytest.fixture(scope="module")
def region_asm(tmp_path_factory):
    return gfx950_asm(tmp_path_factory, "region")


@pytest.mark.parametrize("kernel, vgprs, lds", [("k_region_sums", 128, 12288), ("k_region_add", 128, 0)])
def test_region_kernels_budget(region_asm, kernel, vgprs, lds):
    meta = kernel_meta(region_asm, kernel)
    print(meta_line(kernel, meta))
    assert meta["vgpr_count"] <= vgprs, meta["vgpr_count"]
    assert meta["vgpr_spill_count"] == 0, meta["vgpr_spill_count"]
    assert meta["private_segment_fixed_size"] == 0, meta["private_segment_fixed_size"]
    assert meta["group_segment_fixed_size"] <= lds, meta["group_segment_fixed_size"]
