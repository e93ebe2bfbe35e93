"""CPU: the gfx950 code of the kernels of csrc/decode.hip (cross-compiled, no GPU needed) against the register budget of
DESIGN.md §6a "one row walk": the three row-walk kernels (k_count_alleles, k_count_samples, k_genotype_planes) share their
prologue, row loop and call reader as inlined device functions, and sharing them must cost no registers, no spills, no
scratch and no LDS over what the three separate copies took; the two decode kernels, which share none of it, keep their
counts.  SGPR counts and SGPR spills move with the compiler's scalar allocation and are printed, not asserted.

The same for csrc/lz4bits.hip: the plane coder is a chain of inlined phases, and every instantiation of its
two kernels must keep the registers, spills, scratch and LDS it had as one function body: 72 VGPRs is the last count at
seven waves per SIMD (64 the last at eight, which the int8 kernel reaches at depths 0 and 1), and 11 248 bytes of LDS keep
14 workgroups per CU.  That test reads the kernels' metadata only.

The same for the reductions over bit planes (DESIGN.md §6a "plane reductions"): k_pair_counts and k_ld_counts share the
popcount tile of csrc/plane_tiles.h, k_assoc_sums and k_score_sums the bit-sum tile's pieces, and each keeps the registers
and the LDS of its separate copy, without spills or scratch; the kernels of ld.hip that share nothing keep their exact
counts.  Metadata only.

The same for csrc/lz4.hip: the byte-wise coder is a driver over inlined phases, and each of the nine
instantiations of k_lz4_blocks keeps the registers, spills and scratch it had as one function body; three of them sit exactly
on an occupancy line (72 VGPRs at seven waves per SIMD, 64 at eight).  Its LDS is all dynamic.  Metadata only.

The same for csrc/index.hip: k_index_hop is a loop over inlined phases and k_parse_fixed a sequence of steps,
and the four instantiations of the one and the other keep what they had as one function body each — here the scalar side
counts too (the walk's state is wave-uniform and must stay in scalar registers: SGPRs and SGPR spills are part of the budget).
The instruction lines of each body are printed beside profiles/r15_index_isa.txt.

The same for csrc/encode.hip (DESIGN.md §3 "The encode kernels as named phases"): the three encode kernels are drivers over inlined phases, and they and the
padding / expand kernels beside them keep what they had as one function body each, scalar side included (a tile's place and a
line's place are wave-uniform); k_encode_planes sits two registers under the last count at which four workgroups share a CU.  The
static LDS of the encode kernels is held exactly.  k_encode_general must still reach its staged piece through LDS byte reads
and through no flat load (the address-space comments in encode.hip).  Body lines are printed beside profiles/r16_encode_isa.txt."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> (VGPRs, spilled VGPRs, scratch bytes, static LDS bytes, scratch_ instructions) before the row walk was shared
BUDGET = {
    "k_count_alleles": (84, 0, 0, 16, 0),
    "k_count_samples": (64, 0, 0, 1040, 0),
    "k_genotype_planes": (64, 4, 20, 16, 9),
    "k_decode_blocks": (57, 0, 0, 16, 0),
    "k_decode_sel": (22, 0, 0, 16, 0),
}


# (kernel, candidates per one, lazy rule) -> (VGPRs, spilled VGPRs, scratch bytes, static LDS bytes) before the plane coder
# was cut into phases
BP_BUDGET = {}
for _d in (0, 1, 2, 4, 8, 12, 16):
    BP_BUDGET[("k_lz4_bitplanes", _d, False)] = (64 if _d < 2 else 66, 0, 0, 8688 if _d < 2 else 11248)
    BP_BUDGET[("k_lz4_bitplanes_uni", _d, False)] = (64 if _d == 0 else 70, 0, 0, 9072 if _d < 2 else 11248)
for _d in (2, 12):
    BP_BUDGET[("k_lz4_bitplanes", _d, True)] = (64, 0, 0, 11248)
    BP_BUDGET[("k_lz4_bitplanes_uni", _d, True)] = (70, 0, 0, 11248)


# (file, kernel as it stands in the mangled name) -> (VGPRs, static LDS bytes) before the plane tiles were shared; none of
# them spills or uses scratch
PLANE_BUDGET = {("pairs", "k_pair_counts"): (118, 33280), ("ld", "k_ld_counts"): (66, 16896)}
PLANE_BUDGET.update({("assoc", f"k_assoc_sumsILj{_ct}EE"): b
                     for _ct, b in zip((1, 2, 3, 4), ((72, 16384), (114, 32768), (166, 49152), (184, 65536)))})
# (k_score_sums<4> has the smaller STEP_UNROLL: score.hip)
PLANE_BUDGET.update({("score", f"k_score_sumsILj{_ct}EE"): b
                     for _ct, b in zip((1, 2, 3, 4), ((62, 12288), (86, 24576), (114, 36864), (100, 49152)))})
# the kernels of ld.hip outside the shared tile -> VGPRs, exactly
LD_UNTOUCHED = {"k_variant_planes": 25, "k_ld_exceeds": 26}
LD_UNTOUCHED.update({f"k_ld_walkILi{_nq}EE": v for _nq, v in zip((1, 2, 4, 8, 16), (16, 16, 20, 28, 44))})


# k_lz4_blocks<minimum waves per SIMD, effort (5 run only, 6 hash, 7 long run), from bit planes> -> (VGPRs, spilled VGPRs,
# scratch bytes) before the stream coder was cut into phases
LZ4_BUDGET = {(0, 5, False): (76, 0, 0), (8, 5, False): (64, 12, 48), (0, 6, False): (80, 0, 0), (7, 6, False): (72, 3, 12),
              (0, 7, False): (80, 0, 0), (7, 7, False): (72, 3, 12), (8, 5, True): (64, 19, 76), (7, 6, True): (72, 17, 68),
              (7, 7, True): (72, 18, 72)}


# kernel of index.hip as it stands in the mangled name -> (VGPRs, SGPRs, SGPR spills, spilled VGPRs, scratch bytes, static LDS
# bytes) before k_index_hop and k_parse_fixed were cut into phases
INDEX_BUDGET = {"k_index_hopILi5ELb1EE": (94, 106, 8, 0, 0, 0), "k_index_hopILi3ELb1EE": (57, 106, 2, 0, 0, 0),
                "k_index_hopILi5ELb0EE": (52, 101, 0, 0, 0, 0), "k_index_hopILi3ELb0EE": (42, 89, 0, 0, 0, 0),
                "k_parse_fixed": (83, 82, 0, 0, 0, 17432)}


# kernel of encode.hip as it stands in the mangled name -> (VGPRs, SGPRs, SGPR spills, spilled VGPRs, scratch bytes, static LDS
# bytes, non-empty body lines) before the encode kernels were cut into phases; the body lines are printed, not asserted
ENCODE_BUDGET = {"k_encode_tiles": (78, 81, 0, 0, 0, 32768, 8902), "k_encode_planes": (127, 95, 0, 0, 0, 32768, 16434),
                 "k_encode_generalILb1EE": (111, 106, 12, 0, 0, 12544, 2138), "k_encode_generalILb0EE": (108, 106, 0, 0, 0, 12544, 1959),
                 "k_zero_rect": (28, 32, 0, 0, 0, 0, 233), "k_zero_tail_cursor": (28, 35, 0, 0, 0, 0, 539),
                 "k_zero_planes_rect": (12, 22, 0, 0, 0, 0, 163), "k_zero_planes_cursor": (14, 33, 0, 0, 0, 0, 457),
                 "k_planes_expand": (40, 40, 0, 0, 0, 0, 905)}
ENCODE_GENERAL_FLAT_LOADS = 0    # flat_load instructions in either instantiation of k_encode_general before the pass


def gfx950_asm(tmp_path_factory, stem):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "haplohyped_varawareml_amd", "csrc", stem + ".hip")
    out = tmp_path_factory.mktemp("isa") / (stem + ".s")
    r = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.dirname(src), "-S", "--cuda-device-only", "-o", str(out), src],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


@pytest.fixture(scope="module")
def decode_asm(tmp_path_factory):
    return gfx950_asm(tmp_path_factory, "decode")


@pytest.fixture(scope="module")
def lz4bits_asm(tmp_path_factory):
    return gfx950_asm(tmp_path_factory, "lz4bits")


@pytest.fixture(scope="module")
def lz4_asm(tmp_path_factory):
    return gfx950_asm(tmp_path_factory, "lz4")


@pytest.fixture(scope="module")
def plane_asm(tmp_path_factory):
    return {stem: gfx950_asm(tmp_path_factory, stem) for stem in ("pairs", "ld", "assoc", "score")}


def kernel_body(asm, name):
    """the instructions of a kernel, comments stripped, up to the end of the function (a kernel may end in several places)"""
    m = re.search(rf"^(_Z\d+{name}\w+):\s*;.*?$", asm, re.M)
    assert m, name
    end = re.compile(r"^\.Lfunc_end\d+:", re.M).search(asm, m.end())
    return re.sub(r";.*", "", asm[m.end():end.start()])


def kernel_meta(asm, name):
    meta = asm[asm.index("amdhsa.kernels"):]
    entries = [e for e in meta.split("  - .agpr_count") if re.search(rf"\.name:\s+_Z\d+{name}\w+", e)]
    assert len(entries) == 1, name
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", entries[0], re.M)}


@pytest.mark.parametrize("name", sorted(BUDGET))
def test_register_budget(decode_asm, name):
    meta, body = kernel_meta(decode_asm, name), kernel_body(decode_asm, name)
    vgprs, vgpr_spills, scratch, lds, scratch_ops = BUDGET[name]
    print(f"{name}: {meta['vgpr_count']} VGPRs, {meta['sgpr_count']} SGPRs, {meta['sgpr_spill_count']} SGPR spills, "
          f"{meta['vgpr_spill_count']} VGPR spills, {meta['private_segment_fixed_size']} B scratch, "
          f"{meta['group_segment_fixed_size']} B static LDS")
    assert meta["vgpr_count"] <= vgprs, meta["vgpr_count"]
    assert meta["vgpr_spill_count"] <= vgpr_spills, meta["vgpr_spill_count"]
    assert meta["private_segment_fixed_size"] <= scratch, meta["private_segment_fixed_size"]
    assert meta["group_segment_fixed_size"] <= lds, meta["group_segment_fixed_size"]
    assert len(re.findall(r"\bscratch_\w+", body)) <= scratch_ops
    if name.startswith("k_decode"):      # not touched by the row walk: the same code, the same registers
        assert (meta["vgpr_count"], meta["vgpr_spill_count"], meta["private_segment_fixed_size"]) == (vgprs, vgpr_spills, scratch)


@pytest.mark.parametrize("name", ["k_count_alleles", "k_count_samples", "k_genotype_planes"])
def test_calls_come_from_lds_in_16_byte_loads(decode_asm, name):
    body = kernel_body(decode_asm, name)
    assert len(re.findall(r"\bds_read_b128\b", body)) >= 4, name      # 2 planes x 2 groups of 16 calls per thread
    if name != "k_count_alleles":        # (its chunk pointer is generic on purpose: DESIGN.md §6a)
        assert not re.search(r"\bflat_\w+", body), name


@pytest.mark.parametrize("kernel,depth,lazy", sorted(BP_BUDGET))
def test_plane_coder_budget(lz4bits_asm, kernel, depth, lazy):
    # one instantiation by its template arguments, as they stand in the mangled name
    meta = kernel_meta(lz4bits_asm, f"{kernel}ILi{depth}ELb{int(lazy)}EE")
    vgprs, vgpr_spills, scratch, lds = BP_BUDGET[(kernel, depth, lazy)]
    print(f"{kernel}<{depth}, {str(lazy).lower()}>: {meta['vgpr_count']} VGPRs, {meta['sgpr_count']} SGPRs, "
          f"{meta['sgpr_spill_count']} SGPR spills, {meta['vgpr_spill_count']} VGPR spills, "
          f"{meta['private_segment_fixed_size']} B scratch, {meta['group_segment_fixed_size']} B static LDS")
    assert meta["vgpr_count"] <= vgprs, meta["vgpr_count"]
    assert meta["vgpr_spill_count"] <= vgpr_spills, meta["vgpr_spill_count"]
    assert meta["private_segment_fixed_size"] <= scratch, meta["private_segment_fixed_size"]
    assert meta["group_segment_fixed_size"] <= lds, meta["group_segment_fixed_size"]


def meta_line(name, meta):
    return (f"{name}: {meta['vgpr_count']} VGPRs, {meta['sgpr_count']} SGPRs, {meta['sgpr_spill_count']} SGPR spills, "
            f"{meta['vgpr_spill_count']} VGPR spills, {meta['private_segment_fixed_size']} B scratch, "
            f"{meta['group_segment_fixed_size']} B static LDS")


@pytest.mark.parametrize("stem,kernel", sorted(PLANE_BUDGET))
def test_plane_reduction_budget(plane_asm, stem, kernel):
    meta = kernel_meta(plane_asm[stem], kernel)
    vgprs, lds = PLANE_BUDGET[(stem, kernel)]
    print(meta_line(kernel, meta))
    assert meta["vgpr_count"] <= vgprs, meta["vgpr_count"]
    assert meta["vgpr_spill_count"] == 0, meta["vgpr_spill_count"]
    assert meta["private_segment_fixed_size"] == 0, meta["private_segment_fixed_size"]
    assert meta["group_segment_fixed_size"] <= lds, meta["group_segment_fixed_size"]


@pytest.mark.parametrize("kernel", sorted(LD_UNTOUCHED))
def test_ld_kernels_outside_the_tile_keep_their_registers(plane_asm, kernel):
    meta = kernel_meta(plane_asm["ld"], kernel)
    print(meta_line(kernel, meta))
    assert meta["vgpr_count"] == LD_UNTOUCHED[kernel], meta["vgpr_count"]
    assert (meta["vgpr_spill_count"], meta["private_segment_fixed_size"]) == (0, 0)


@pytest.fixture(scope="module")
def index_asm(tmp_path_factory):
    return gfx950_asm(tmp_path_factory, "index")


@pytest.mark.parametrize("kernel", sorted(INDEX_BUDGET))
def test_line_index_budget(index_asm, kernel):
    meta = kernel_meta(index_asm, kernel)
    body = [ln for ln in kernel_body(index_asm, kernel).splitlines() if ln.strip()]
    print(meta_line(kernel, meta) + f", {len(body)} lines of kernel body (profiles/r15_index_isa.txt)")
    got = (meta["vgpr_count"], meta["sgpr_count"], meta["sgpr_spill_count"], meta["vgpr_spill_count"],
           meta["private_segment_fixed_size"], meta["group_segment_fixed_size"])
    assert all(g <= b for g, b in zip(got, INDEX_BUDGET[kernel])), (got, INDEX_BUDGET[kernel])


@pytest.mark.parametrize("mw,effort,planes", sorted(LZ4_BUDGET))
def test_bytewise_coder_budget(lz4_asm, mw, effort, planes):
    meta = kernel_meta(lz4_asm, f"k_lz4_blocksILi{mw}ELi{effort}ELb{int(planes)}EE")
    vgprs, vgpr_spills, scratch = LZ4_BUDGET[(mw, effort, planes)]
    print(meta_line(f"k_lz4_blocks<{mw}, {effort}, {str(planes).lower()}>", meta))
    assert meta["vgpr_count"] <= vgprs, meta["vgpr_count"]
    assert meta["vgpr_spill_count"] <= vgpr_spills, meta["vgpr_spill_count"]
    assert meta["private_segment_fixed_size"] <= scratch, meta["private_segment_fixed_size"]
    assert meta["group_segment_fixed_size"] == 0, meta["group_segment_fixed_size"]


@pytest.fixture(scope="module")
def encode_asm(tmp_path_factory):
    return gfx950_asm(tmp_path_factory, "encode")


@pytest.mark.parametrize("kernel", sorted(ENCODE_BUDGET))
def test_encode_budget(encode_asm, kernel):
    meta = kernel_meta(encode_asm, kernel)
    body = [ln for ln in kernel_body(encode_asm, kernel).splitlines() if ln.strip()]
    budget, parent_lines = ENCODE_BUDGET[kernel][:6], ENCODE_BUDGET[kernel][6]
    print(meta_line(kernel, meta) + f", {len(body)} lines of kernel body (before the pass: {parent_lines}; profiles/r16_encode_isa.txt)")
    vgprs, sgprs, sgpr_spills, vgpr_spills, scratch, lds = budget
    assert meta["vgpr_count"] <= vgprs, meta["vgpr_count"]
    assert meta["sgpr_count"] <= sgprs, meta["sgpr_count"]
    assert meta["sgpr_spill_count"] <= sgpr_spills, meta["sgpr_spill_count"]
    assert meta["vgpr_spill_count"] <= vgpr_spills, meta["vgpr_spill_count"]
    assert meta["private_segment_fixed_size"] <= scratch, meta["private_segment_fixed_size"]
    assert meta["group_segment_fixed_size"] <= lds, meta["group_segment_fixed_size"]
    if kernel.startswith("k_encode"):
        assert meta["group_segment_fixed_size"] == lds, meta["group_segment_fixed_size"]


@pytest.mark.parametrize("kernel", ["k_encode_generalILb1EE", "k_encode_generalILb0EE"])
def test_general_kernel_reads_its_piece_from_lds(encode_asm, kernel):
    body = kernel_body(encode_asm, kernel)
    assert re.search(r"\bds_read_u8\b", body), kernel
    assert len(re.findall(r"\bflat_load\w*", body)) <= ENCODE_GENERAL_FLAT_LOADS, kernel
