"""CPU: the gfx950 code of csrc/quad.hip (cross-compiled, no GPU needed), metadata only: k_quad_forms holds eight f64
accumulators a wave and two stages of the matrix in LDS, and must keep what two 512-thread workgroups per CU need of the
memory: no spilled register, no scratch, at most 80 KiB of static LDS (a CU has 160 KiB).  Its register counts are
printed, not asserted."""
import pytest

from tests.test_isa_counts import gfx950_asm, kernel_meta, meta_line


@pytest.fixture(scope="module")
def quad_asm(tmp_path_factory):
    return gfx950_asm(tmp_path_factory, "quad")


def test_quad_forms_budget(quad_asm):
    meta = kernel_meta(quad_asm, "k_quad_forms")
    print(meta_line("k_quad_forms", meta))
    assert meta["vgpr_spill_count"] == 0, meta["vgpr_spill_count"]
    assert meta["private_segment_fixed_size"] == 0, meta["private_segment_fixed_size"]
    assert meta["group_segment_fixed_size"] <= 80 * 1024, meta["group_segment_fixed_size"]
