"""ctypes binding of libhhgt.so (include/hhgt.h).  Fails loudly when the library is missing:
there is no Python/CPU implementation of the path behind it."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# HHGT_LIB: load another build of the same library (development: tools/lz4_stats.py uses a -DHHGT_LZ4_STATS build)
LIB_PATH = os.environ.get("HHGT_LIB") or os.path.join(HERE, "libhhgt.so")

OK = 0
BLOSC1 = 1
BLOSC2 = 2
N_STAGES = 16
STAGE_NAMES = ["index", "fixed", "encode", "general", "lz4", "frame", "decode", "onehot", "inflate", "pairs", "ld_transpose",
               "ld", "ld_prune", "ld_walk", "grm", "assoc"]


class HhgtError(RuntimeError):
    """Raised for every non-zero libhhgt return code (the reference raises RuntimeError from
    cpp/parse_vcf.cpp:63-66)."""

    def __init__(self, code, msg):
        super().__init__(f"{msg} (hhgt rc={code})")
        self.code = code


class Layout(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("sc", C.c_int32), ("vc", C.c_int32), ("ring", C.c_int32),
                ("v_capacity", C.c_uint64)]


class Window(C.Structure):     # hhgt_window
    _fields_ = [("ref_ptr", C.c_uint64), ("ref_len", C.c_uint64), ("win_start", C.c_int64),
                ("var_start_ptr", C.c_uint64), ("var_ref_ptr", C.c_uint64), ("var_alt_ptr", C.c_uint64),
                ("geno_ptr", C.c_uint64), ("geno_first", C.c_uint32), ("var_lo", C.c_uint32),
                ("var_hi", C.c_uint32), ("reserved", C.c_uint32)]


class BlockSel(C.Structure):   # hhgt_block_sel
    _fields_ = [("src_ptr", C.c_uint64), ("src_bytes", C.c_uint64), ("dst_off", C.c_uint64), ("block", C.c_uint32),
                ("lo", C.c_uint32), ("hi", C.c_uint32), ("reserved", C.c_uint32)]


class CountSel(C.Structure):   # hhgt_count_sel
    _fields_ = [("src_ptr", C.c_uint64), ("src_bytes", C.c_uint64), ("row_mask", C.c_uint64), ("out_row", C.c_uint64),
                ("part", C.c_uint32), ("lo", C.c_uint32), ("hi", C.c_uint32), ("reserved", C.c_uint32)]


class SampleSel(C.Structure):  # hhgt_sample_sel
    _fields_ = [("src_ptr", C.c_uint64), ("src_bytes", C.c_uint64), ("row_mask", C.c_uint64), ("out_row", C.c_uint64),
                ("mask_word", C.c_uint64), ("part", C.c_uint32), ("lo", C.c_uint32), ("hi", C.c_uint32),
                ("reserved", C.c_uint32)]


class PlaneSel(C.Structure):   # hhgt_plane_sel
    _fields_ = [("src_ptr", C.c_uint64), ("src_bytes", C.c_uint64), ("row_mask", C.c_uint64), ("out_row", C.c_uint64),
                ("mask_word", C.c_uint64), ("out_word", C.c_uint64), ("part", C.c_uint32), ("lo", C.c_uint32),
                ("hi", C.c_uint32), ("reserved", C.c_uint32)]


class GatherSel(C.Structure):  # hhgt_gather_sel
    _fields_ = [("src_ptr", C.c_uint64), ("src_bytes", C.c_uint64), ("row_mask", C.c_uint64), ("out_row", C.c_uint64),
                ("mask_word", C.c_uint64), ("out_col", C.c_uint64), ("part", C.c_uint32), ("lo", C.c_uint32),
                ("hi", C.c_uint32), ("reserved", C.c_uint32)]


class EncodeStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "n_lines", "n_records", "n_kept", "n_drop_region", "n_drop_filter", "n_haploid_padded",
        "n_malformed", "n_general_lines", "n_chrom_runs")]

    def asdict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


RESULT_RUNS = 16


class EncodeResultRec(C.Structure):     # hhgt_encode_result
    _fields_ = [("stats", EncodeStats), ("cursor_before", C.c_uint64), ("cursor_after", C.c_uint64),
                ("n_lines_over", C.c_uint64), ("err_density", C.c_uint64), ("run_first", C.c_uint64 * RESULT_RUNS),
                ("run_names", (C.c_char * 32) * RESULT_RUNS), ("v_capacity", C.c_uint64), ("done", C.c_uint32),
                ("reserved", C.c_uint32)]

    def chrom_runs(self):
        n = min(int(self.stats.n_chrom_runs), RESULT_RUNS)
        return [(int(self.run_first[i]), bytes(self.run_names[i]).split(b"\0")[0].decode()) for i in range(n)]


_vp, _u64, _u32, _i32, _str = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_char_p
_lay, _pu64, _pi32, _pvp = C.POINTER(Layout), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_void_p)
# every function of include/hhgt.h, include/hhgt_synth.h and include/hhgt_reader.h this package or its tests call: name ->
# (restype, argtypes).  load() applies the table; tests/test_abi_binding.py holds it against the headers.  (The ingest engine
# has a header of its own, include/hhgt_ingest.h: ingest.py binds that.)
PROTOTYPES = {
    "hhgt_version": (_str, []),
    "hhgt_last_error": (_str, []),
    "hhgt_device_count": (_i32, []),
    "hhgt_ctx_create": (_i32, [_i32, C.POINTER(_vp)]),
    "hhgt_ctx_destroy": (None, [_vp]),
    "hhgt_layout_bytes": (_u64, [_lay]),
    "hhgt_layout_offset": (_u64, [_lay, _u32, _u64]),
    "hhgt_encode_text": (_i32, [_vp, _vp, _u64, _str, _lay, _u64, _vp, _vp, _vp, _vp, _vp, C.POINTER(EncodeStats), _vp]),
    "hhgt_encode_text_async": (_i32, [_vp, _vp, _u64, _str, _lay, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hhgt_encode_text_planes_async": (_i32, [_vp, _vp, _u64, _str, _lay, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hhgt_encode_result_status": (_i32, [_vp]),
    "hhgt_encode_chrom_runs": (_i32, [_vp, _u32, _vp, _vp, C.POINTER(_u32)]),
    "hhgt_pad_tail": (_i32, [_vp, _lay, _u64, _u64, _u64, _vp, _vp]),
    "hhgt_pad_tail_cursor": (_i32, [_vp, _lay, _vp, _vp, _vp]),
    "hhgt_planes_bytes": (_u64, [_lay]),
    "hhgt_pad_tail_planes": (_i32, [_vp, _lay, _u64, _u64, _u64, _vp, _vp]),
    "hhgt_pad_tail_planes_cursor": (_i32, [_vp, _lay, _vp, _vp, _vp]),
    "hhgt_compress_planes": (_i32, [_vp, _lay, _vp, _vp, _u32, _u32, _i32, _vp, _u64, _vp, _pu64, _vp]),
    "hhgt_planes_expand": (_i32, [_vp, _lay, _vp, _vp, _u32, _u32, _vp, _vp]),
    "hhgt_set_clevel": (_i32, [_vp, _i32]),
    "hhgt_reserve": (_i32, [_vp, _u64, _u32, _u64, _u64, _i32, _i32]),
    "hhgt_set_keep_multiallelic": (_i32, [_vp, _i32]),
    "hhgt_set_index_mode": (_i32, [_vp, _i32]),
    "hhgt_stream_create": (_i32, [_vp, _i32, C.POINTER(_vp)]),
    "hhgt_stream_destroy": (_i32, [_vp, _vp]),
    "hhgt_set_frame_stream": (_i32, [_vp, _vp]),
    "hhgt_compress_bound": (_u64, [_u64, _u64, _i32, _i32]),
    "hhgt_compress_chunks": (_i32, [_vp, _vp, _u64, _u64, _i32, _i32, _i32, _vp, _u64, _vp, _pu64, _vp]),
    "hhgt_decompress_chunks": (_i32, [_vp, _vp, _vp, _u64, _u64, _i32, _i32, _vp, _pu64, _vp]),
    "hhgt_decompress_blocks": (_i32, [_vp, _vp, _u32, _u64, _i32, _i32, _vp, _pu64, _vp]),
    "hhgt_count_alleles": (_i32, [_vp, _vp, _u32, _u32, _u32, _i32, _i32, _vp, _u64, _pu64, _vp]),
    "hhgt_count_samples": (_i32, [_vp, _vp, _u32, _u32, _u32, _i32, _i32, _vp, _u64, _vp, _u64, _pu64, _vp]),
    "hhgt_genotype_planes": (_i32, [_vp, _vp, _u32, _u32, _u32, _i32, _i32, _vp, _u64, _vp, _u64, _u64, _pu64, _vp]),
    "hhgt_gather_calls": (_i32, [_vp, _vp, _u32, _u32, _u32, _i32, _i32, _vp, _u64, _vp, _u64, _vp, _i32, _vp, _u64, _u64, _u64,
                                 _pu64, _vp]),
    "hhgt_pair_counts": (_i32, [_vp, _vp, _u64, _u64, _u64, _u64, _vp, _vp]),
    "hhgt_grm": (_i32, [_vp, _vp, _u64, _u64, _u64, _u64, _vp, _vp, _vp]),
    "hhgt_variant_planes": (_i32, [_vp, _vp, _u64, _u64, _u64, _u64, _vp, _vp]),
    "hhgt_ld_counts": (_i32, [_vp, _vp, _u64, _u64, _u32, _vp, _vp]),
    "hhgt_ld_prune": (_i32, [_vp, _vp, _u64, _u32, C.c_double, _vp, _vp]),
    "hhgt_ld_decisions": (_i32, [_vp, _vp, _u64, _u32, C.c_double, _vp, C.c_int64, _vp, _vp]),
    "hhgt_ld_clump": (_i32, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, C.POINTER(_u32), _vp]),
    "hhgt_assoc_sums": (_i32, [_vp, _vp, _u64, _u64, _vp, _u32, _vp, _vp]),
    "hhgt_quad_forms": (_i32, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "hhgt_logistic_fit": (_i32, [_vp, _vp, _u64, _u64, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "hhgt_score_sums": (_i32, [_vp, _vp, _u64, _u64, _u64, _u64, _vp, _u32, _vp, _vp]),
    "hhgt_region_sums": (_i32, [_vp, _vp, _u64, _u64, _vp, _u32, _vp, _u64, _vp, _u64, _u64, _u64, _vp, _pu64, _vp]),
    "hhgt_bgzf_scan": (_i32, [_vp, _u64, _u64, _vp, _vp, _vp, _vp, _pu64, _pu64]),
    "hhgt_inflate_members": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _pu64, _vp]),
    "hhgt_onehot_windows": (_i32, [_vp, _vp, _u32, _u32, _vp, _i32, _vp, _vp, _vp]),
    "hhgt_onehot_bases_u8": (_i32, [_vp, _vp, _u64, _vp, _i32, _vp, _vp]),
    "hhgt_profile_enable": (_i32, [_vp, _i32]),
    "hhgt_profile_reset": (_i32, [_vp]),
    "hhgt_profile_read": (_i32, [_vp, C.POINTER(C.c_double), _pu64]),
    "hhgt_synth_render_fixed": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _str, _i32, _u64, _vp]),
    "hhgt_synth_render_mixed": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _str, _i32, _u64, _vp]),
    "hhgt_synth_write_bgzf": (_i32, [_str, _vp, _u64, _i32, _i32]),
    "hhgt_reader_open": (_i32, [_str, _u64, _i32, _i32, _pvp]),
    "hhgt_reader_close": (None, [_vp]),
    "hhgt_reader_is_bgzf": (_i32, [_vp]),
    "hhgt_reader_next": (_i32, [_vp, _pvp, _pu64]),
    "hhgt_reader_acquire": (_i32, [_vp, _pvp, _pu64, _pi32, _pi32]),
    "hhgt_reader_release": (_i32, [_vp, _i32]),
    "hhgt_reader_copy_async": (_i32, [_vp, _vp, _u64, _vp, _vp]),
    "hhgt_reader_stats": (_i32, [_vp, _pu64, _pu64]),
    "hhgt_reader_trim_pool": (None, []),
    "hhgt_reader_prewarm": (_i32, [_u64, _i32]),
    "hhgt_effective_cpus": (_i32, []),
    "hhgt_crc32": (_u32, [_vp, _u64]),
    "hhgt_fast_inflate": (_i32, [_vp, _u64, _vp, _u64]),
}

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime: it must be in the process BEFORE libhhgt.so pulls in
    # libamdhip64, or the two runtimes disagree about the visible devices
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing. Build it with `python -m haplohyped_varawareml_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback for this path.")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc):
    if rc != OK:
        raise HhgtError(rc, load().hhgt_last_error().decode(errors="replace"))
