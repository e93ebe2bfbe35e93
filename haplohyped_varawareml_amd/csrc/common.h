// common.h — internal declarations shared by the libhhgt.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>
#include "../../include/hhgt.h"

#define HHGT_WAVE 64
// development (-DHHGT_ENC_PRIO=n): the memory-bound kernels of the encode chain raise their waves' issue priority, so that
// beside the (VALU-bound) LZ4 kernel of the other stream their few instructions go out first
#ifdef HHGT_ENC_PRIO
#define HHGT_WAVE_PRIO() __builtin_amdgcn_s_setprio(HHGT_ENC_PRIO)
#else
#define HHGT_WAVE_PRIO()
#endif

// wave-wide inclusive sum on DPP row shifts (no LDS round trips); *total = the wave's sum (uniform), formed from the
// rows' sums on the scalar unit, beside the lanes' last add
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t wave_scan_sum_dpp(uint32_t x, uint32_t lane, uint32_t *total)
{
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);   // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);
    const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane((int)x, 15);
    const uint32_t t1 = (uint32_t)__builtin_amdgcn_readlane((int)x, 31) + t0;
    const uint32_t t2 = (uint32_t)__builtin_amdgcn_readlane((int)x, 47) + t1;
    *total = (uint32_t)__builtin_amdgcn_readlane((int)x, 63) + t2;
    const uint32_t row = lane >> 4;
    return x + (row == 0u ? 0u : (row == 1u ? t0 : (row == 2u ? t1 : t2)));
}

__device__ __forceinline__ uint32_t wave_scan_sum_dpp(uint32_t x, uint32_t lane)
{
    uint32_t total;
    return wave_scan_sum_dpp(x, lane, &total);
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// exclusive scan of one value per thread across a 256-thread block; returns exclusive prefix,
// *total = block sum (valid in all threads)
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *total, uint32_t *sm /*>=8*/)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = wave_incl_scan(v);
    if (lane == 63) sm[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t x = sm[i];
        if (i < w) base += x;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}
#endif

// ---- error plumbing -------------------------------------------------------------------------
void hhgt_set_error(const char *fmt, ...);
#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            hhgt_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                           __LINE__);                                                      \
            return HHGT_ERR_HIP;                                                           \
        }                                                                                  \
    } while (0)

// ---- per-line flag bits (index/fixed-column stage) --------------------------------------------
enum : uint32_t {
    LF_RECORD = 1u,        // data line (non-empty, not '#')
    LF_KEEP = 2u,          // passed region + isSNP
    LF_FAST = 4u,          // FORMAT == "GT" and sample region is exactly 4*S-1 bytes
    LF_MALFORMED = 8u,
    LF_DROP_REGION = 16u,
    LF_DROP_FILTER = 32u,
    LF_CHROM_NEW = 64u,    // CHROM differs from the previous data line
};

// device-side counters written by the kernels of one hhgt_encode_text call
struct DevCounters {
    unsigned long long n_lines;
    unsigned long long n_records;
    unsigned long long n_kept;
    unsigned long long n_drop_region;
    unsigned long long n_drop_filter;
    unsigned long long n_haploid;
    unsigned long long n_malformed;
    unsigned long long n_general;    // entries in the redo (variable-width) list
    unsigned long long n_chrom_runs;
    unsigned long long err_density;  // newline-slot overflow
    unsigned long long err_lines;    // lines beyond the caller's max_lines (asynchronous form only)
    unsigned long long cursor_after; // *d_cursor after the call
    unsigned long long n_other;      // bit-plane form: calls that are neither 0, 1 nor missing (their bytes went to d_G)
    unsigned long long pad[3];
};

#define MAX_CHROM_RUNS 4096u

struct RegionFilter {
    char contig[64];
    int contig_len;   // 0 = no filter
    int has_range;
    long long beg, end;  // 1-based inclusive
    int keep_multi;      // non-reference mode: multi-allelic SNP sites pass the record filter (hhgt_set_keep_multiallelic)
};

// index stage geometry: one wave scans INDEX_REGION bytes, at most INDEX_CAP newlines in it
#define INDEX_REGION 16384u
#define INDEX_CAP 1024u

// encode tile geometry
#define TILE_V 128
#define TILE_S 256

struct LayoutDev {
    uint32_t S;
    uint32_t sc_log2;    // log2(samples per chunk); 31 = dense (single sample-chunk)
    uint32_t n_sc;       // sample-chunks per chunk column
    uint32_t Sc;         // samples per chunk (dense: S)
    uint64_t Vc;         // variants per chunk (dense: v_capacity)
    uint64_t v_capacity;
    uint32_t ring;       // > 0: G is a ring of `ring` chunk columns (v_capacity = ring * Vc), kept indices unbounded
    uint32_t pad_;
};
// byte offset of (chunk column slot vcol, sample row s, variant vin of the column) in the int8 matrix — chunk-tiled:
// G[column][sample chunk][row in chunk][variant][haplotype]; matrix_row: where the row's Vc variants start
static inline __host__ __device__ uint64_t matrix_at(const LayoutDev &L, uint64_t vcol, uint32_t s, uint64_t vin)
{
    const uint32_t scol = L.sc_log2 >= 31u ? 0u : (s >> L.sc_log2);
    const uint32_t sin = s - scol * L.Sc;
    return ((((vcol * L.n_sc + scol) * L.Sc + sin) * L.Vc) + vin) * 2ull;
}
static inline __host__ __device__ uint64_t matrix_row(const LayoutDev &L, uint64_t vcol, uint32_t s) { return matrix_at(L, vcol, s, 0ull); }

// ---- bit-plane form of the matrix (include/hhgt.h "Bit-plane form"): tile-major ----------------------------------------
// A chunk column (Vc variants x S_pad padded sample rows) is cut into tiles of PL_TILE variants; a tile holds, per kind-plane
// kp (0: ONE hap 0, 1: ONE hap 1, 2: EXC hap 0, 3: EXC hap 1) and sample row r, one 32-byte piece (bit i = variant i of the
// tile): P[column slot][tile][kp][row][32 B].  The encoder's workgroup (252 rows x one tile) therefore writes four
// contiguous 8064-byte runs — the first version of this path wrote row-major planes, 32-byte pieces 2 KiB apart, and spent
// 40 % of its time on those partial-line writes — and a compressor wave gathers the 16 pieces of its 4096-variant plane.
#define PL_TILE 256u
struct PlanesGeom {
    uint32_t S_pad;   // padded sample rows per chunk column (n_sc * Sc)
    uint32_t bpr;     // Blosc blocks (4096 variants) per sample row of a column: Vc / 4096
    uint32_t tpc;     // tiles per column: Vc / PL_TILE = 16 * bpr
    uint32_t col0;    // first column slot a compress / expand call works on
};
static inline __host__ __device__ uint64_t planes_piece(const PlanesGeom &g, uint64_t col, uint32_t tile, uint32_t kp, uint32_t row)
{
    return ((((col * g.tpc + tile) * 4ull + kp) * g.S_pad) + row) * 32ull;
}
static inline __host__ __device__ PlanesGeom planes_geom(const LayoutDev &L, uint32_t col0)
{
    PlanesGeom g;
    g.S_pad = L.n_sc * L.Sc;
    g.bpr = (uint32_t)(L.Vc >> 12);
    g.tpc = (uint32_t)(L.Vc / PL_TILE);
    g.col0 = col0;
    return g;
}
// block `id` of a compress call (G's block order relative to column col0) -> column slot, sample row, block in the row
static inline __host__ __device__ void planes_block(const PlanesGeom &g, uint64_t id, uint64_t *col, uint32_t *row, uint32_t *bi)
{
    const uint64_t per_col = (uint64_t)g.S_pad * g.bpr;
    const uint64_t c = id / per_col;
    const uint32_t rem = (uint32_t)(id - c * per_col);
    *col = g.col0 + c;
    *row = rem / g.bpr;
    *bi = rem - (rem / g.bpr) * g.bpr;
}
// The same on 32 bits without a division, for k_lz4_bitplanes_uni (lz4bits.hip), where the two divisions stood in front of
// the address of every wave's only global load: floor(n / d) = (mul * 2 n) >> (32 + sh) with sh = ceil(log2 d) and
// mul = ceil(2^(31 + sh) / d) < 2^32 (Granlund / Montgomery 1994, N = 31: mul * d = 2^(31 + sh) + e with e < d <= 2^sh, so
// the quotient is off by n e / (d 2^(31 + sh)) < 1 / d).  EXACT FOR every n < 2^31 and every 1 <= d < 2^31;
// launch_lz4_bitplanes makes sure of both (block ids stay below 2^30 there).
struct PlanesDiv {
    uint32_t mul_col, sh_col;   // / (S_pad * bpr): blocks per column
    uint32_t mul_row, sh_row;   // / bpr
};
static inline __host__ __device__ void planes_recip(uint32_t d, uint32_t *mul, uint32_t *sh)
{
    uint32_t l = 0;
    while (l < 31u && (1u << l) < d) ++l;
    *mul = (uint32_t)(((1ull << (31u + l)) + d - 1u) / d);
    *sh = l;
}
static inline __host__ __device__ uint32_t planes_div32(uint32_t n, uint32_t mul, uint32_t sh)
{
    return (uint32_t)(((uint64_t)mul * (n << 1)) >> 32) >> sh;
}
static inline __host__ __device__ PlanesDiv planes_div(const PlanesGeom &g)
{
    PlanesDiv dv;
    planes_recip(g.S_pad * g.bpr, &dv.mul_col, &dv.sh_col);
    planes_recip(g.bpr, &dv.mul_row, &dv.sh_row);
    return dv;
}
static inline __host__ __device__ void planes_block32(const PlanesGeom &g, const PlanesDiv &dv, uint32_t id, uint64_t *col, uint32_t *row, uint32_t *bi)
{
    const uint32_t c = planes_div32(id, dv.mul_col, dv.sh_col);
    const uint32_t rem = id - c * (g.S_pad * g.bpr);
    const uint32_t r = planes_div32(rem, dv.mul_row, dv.sh_row);
    *col = (uint64_t)g.col0 + c;
    *row = r;
    *bi = rem - r * g.bpr;
}
// workgroup wg of k_lz4_bitplanes_uni's grid -> the block and the byte plane (0 / 1) it codes.  XCD-aware: of a group of 128
// workgroups, XCD slot r & 7 takes blocks 8 (r & 7) .. 8 (r & 7) + 7 of the group's 64, both planes
static inline __host__ __device__ void planes_wg_plane(uint32_t wg, uint32_t *bid, uint32_t *h)
{
    const uint32_t r = wg & 127u, k = r >> 3;
    *bid = (wg >> 7) * 64u + (r & 7u) * 8u + (k >> 1);
    *h = k & 1u;
}
// where lane `lane` of the wave that codes byte plane h of block bid takes its 8 bytes of the ONE planes from (bytes into the
// planes buffer): lane l reads quarter l & 3 of the 32-byte piece of tile l / 4.  Its 8 bytes of the EXC planes lie
// planes_exc_step(g) bytes behind
static inline __host__ __device__ uint64_t planes_lane_bytes(const PlanesGeom &g, const PlanesDiv &dv, uint32_t bid, uint32_t h, uint32_t lane)
{
    uint64_t col;
    uint32_t row, bi;
    planes_block32(g, dv, bid, &col, &row, &bi);
    return planes_piece(g, col, bi * 16u + (lane >> 2), h, row) + (lane & 3u) * 8ull;
}
static inline __host__ __device__ uint64_t planes_exc_step(const PlanesGeom &g) { return (uint64_t)g.S_pad * 64ull; }

// workspace buffer that only grows
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes);
    void release();
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// ---- prefix sums of the encode chain without scan launches ----------------------------------------------------------------
// A compaction workgroup owns CHAIN_GROUP entries (index regions for k_compact_newlines, lines for k_compact_kept).  The
// kernel in front of it leaves one total per group behind, and workgroup b sums the totals in front of it itself, the way
// k_scan_down_n sums its tiles' partials.  That fan-in is linear in the number of groups, so it is bounded like
// SCAN_SHORT_MAX: at CHAIN_FANIN_MAX = 2048 groups the last workgroup reads 8 words per thread and array (what a scan tile
// reads per thread, SCAN_ITEMS) and all workgroups together 2048^2 / 2 words per array, 8 MB out of L2.  Four times that
// many groups would be 16 times the reads, beyond what the two scan launches cost.
//  - regions: a text block is below 4 GiB (encode_check_args), i.e. at most 2^18 regions or 1024 groups: always inside.
//  - lines: up to 2048 * 256 = 524 288 (the caller's max_lines); beyond, k_parse_fixed writes its keep / cnew flags and
//    launch_scan_exclusive_u32_pair scans them as before (chain_scanned).
#define CHAIN_GROUP 256u
#define CHAIN_FANIN_MAX 2048u
static_assert(((0xFFFFFFF0ull + 1 + INDEX_REGION - 1) / INDEX_REGION + CHAIN_GROUP - 1) / CHAIN_GROUP <= CHAIN_FANIN_MAX,
              "the region totals of the largest text block must stay inside the fan-in bound");
static inline uint32_t chain_groups(uint32_t n) { return (n + CHAIN_GROUP - 1u) / CHAIN_GROUP; }
static inline bool chain_scanned(uint32_t max_lines) { return chain_groups(max_lines) > CHAIN_FANIN_MAX; }

// the per-line columns of an encode call as the launchers take them: one word per line of the text block.  k_parse_fixed
// writes soff .. flags and the two totals per 256 lines (tot: keep flags of group b at [b], CHROM-run flags at [groups + b]);
// k_compact_kept makes kept index and run index of every line from flags and totals.  More lines than the fan-in bound
// (chain_scanned): keep / cnew are written too and the scan turns them into kidx / crun; the four are NULL otherwise
struct LineCols {
    uint32_t *soff, *lend, *pos, *refalt, *flags, *tot, *keep, *kidx, *cnew, *crun;
};
// what k_compact_kept writes: one word per kept line, the list of lines for the general encoder, the CHROM runs
struct KeptCols {
    uint32_t *soff, *lend, *meta, *redo_list, *redo_flag;
    uint64_t *run_first;   // [MAX_CHROM_RUNS]
    uint8_t *run_names;    // [MAX_CHROM_RUNS][32]
};

// encode workspaces of a context.  They grow inside the calls, or ahead of them in hhgt_reserve: both through ensure_index
// and ensure_lines, so a size is written once
struct EncodeWs {
    DevBuf slots, counts, nl, scan_tmp;
    // region_tot: newlines per CHAIN_GROUP regions, added up by the index kernels.  Zero between calls: k_encode_finish zeroes
    // what its call used, like the DevCounters (hhgt_ctx::counters_clean covers both), and new memory is zeroed where it is made
    DevBuf region_tot;
    DevBuf n_lines;        // one word: the lines the index found (k_compact_newlines)
    DevBuf line_tot;       // LineCols::tot
    enum { L_SOFF, L_LEND, L_POS, L_REFALT, L_FLAGS, K_SOFF, K_LEND, K_META, REDO_LIST, REDO_FLAG, N_LINE };
    enum { S_KEEP, S_KIDX, S_CNEW, S_CRUN, N_SCANNED };
    DevBuf line[N_LINE];         // a word per line each
    DevBuf scanned[N_SCANNED];   // ... and these four for more lines than the fan-in bound only (chain_scanned)
    DevBuf run_first, run_names;
    DevBuf result;         // hhgt_encode_result staging, for a caller's record the device cannot write itself
    int ensure_index(uint32_t n_regions, hipStream_t st);   // what the newline index of n_regions regions writes
    int ensure_lines(uint32_t max_lines);   // what the stages behind the index write for at most max_lines lines
    int ensure_runs();                      // run_first, run_names, result: one size each (a call without text still finishes)
    template <typename F> void each(F f)
    {
        for (DevBuf *b : {&slots, &counts, &nl, &scan_tmp, &region_tot, &n_lines, &line_tot, &run_first, &run_names, &result}) f(*b);
        for (DevBuf &b : line) f(b);
        for (DevBuf &b : scanned) f(b);
    }
    // the launchers' view: every member by name beside its buffer
    uint32_t *col(int i) const { return line[i].as<uint32_t>(); }
    LineCols line_cols(uint32_t max_lines) const
    {
        LineCols l;
        l.soff = col(L_SOFF), l.lend = col(L_LEND), l.pos = col(L_POS), l.refalt = col(L_REFALT), l.flags = col(L_FLAGS);
        l.tot = line_tot.as<uint32_t>();
        const bool sc = chain_scanned(max_lines);
        l.keep = sc ? scanned[S_KEEP].as<uint32_t>() : nullptr, l.kidx = sc ? scanned[S_KIDX].as<uint32_t>() : nullptr;
        l.cnew = sc ? scanned[S_CNEW].as<uint32_t>() : nullptr, l.crun = sc ? scanned[S_CRUN].as<uint32_t>() : nullptr;
        return l;
    }
    KeptCols kept_cols() const
    {
        KeptCols k;
        k.soff = col(K_SOFF), k.lend = col(K_LEND), k.meta = col(K_META), k.redo_list = col(REDO_LIST), k.redo_flag = col(REDO_FLAG);
        k.run_first = run_first.as<uint64_t>(), k.run_names = run_names.as<uint8_t>();
        return k;
    }
};

struct hhgt_ctx {
    int device = 0;
    hipDeviceProp_t prop;
    EncodeWs enc;
    DevBuf counters;       // DevCounters
    DevBuf cursor;         // uint64: v_base of the synchronous hhgt_encode_text (the asynchronous form gets the caller's)
    // compress workspaces
    // two sets: with a frame stream (hhgt_set_frame_stream) the framing of call k reads set k & 1 while the LZ4 kernels of
    // call k + 1 write the other
    struct CodecWs {
        DevBuf lz_scratch, lz_csize, lz_flags, fr_bsize, fr_csize, fr_flags;
        uint32_t lz_tag = 0;       // tag of the last launch_lz4_blocks on lz_flags
        hipEvent_t lz_done = nullptr, fr_done = nullptr;
        bool fr_pending = false;   // fr_done was recorded behind a framing that read this set
        // all but lz_flags (one word, made and zeroed by the first launch on the set) for n_chunks chunks of nblocks blocks
        // of nwaves streams, `slot` scratch bytes per stream
        int ensure(uint64_t n_chunks, uint32_t nblocks, uint32_t nwaves, size_t slot);
    } cw[2];
    uint64_t cmp_seq = 0;
    hipStream_t frame_stream = nullptr;   // hhgt_set_frame_stream; nullptr: the framing follows the LZ4 kernels on their stream
    DevBuf dec_bad, oh_ovl, oh_lut, crc_x2n;
    DevBuf ld_bits;        // hhgt_ld_prune: the per-pair decisions between its two kernels
    DevBuf score_part;     // hhgt_score_sums: the spans' partial sums between its two kernels
    DevBuf region_part;    // hhgt_region_sums: the partial sums of the regions of several pieces, by slot
    DevBuf clump_ws;       // hhgt_ld_clump: forward links, blockers, the two states and the rounds' counters (ClumpWs)
    bool crc_x2n_ready = false;
    // pinned host mirror for counters
    DevCounters *h_counters = nullptr;
    hhgt_encode_result *h_result_pinned = nullptr;
    hhgt_encode_result h_result;
    // last encode's chrom runs (host)
    std::vector<uint64_t> run_first_kept;
    std::vector<std::string> run_names_host;
    int clevel = 5;        // Blosc clevel analogue (reference: compression_opts[4] = 5)
    int keep_multi = 0;    // hhgt_set_keep_multiallelic
    int index_mode = -1;   // hhgt_set_index_mode (< 0: HHGT_INDEX_MODE, default: the walk)
    bool counters_clean = false;   // k_encode_finish of the last call left the DevCounters zeroed
    // profiling
    int profiling = 0;
    double stage_ms[HHGT_N_STAGES] = {0};
    uint64_t stage_launches[HHGT_N_STAGES] = {0};
    struct Pending { int stage; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> event_pool;
};

// RAII-ish stage timer: records events around a stage when profiling is on
struct StageTimer {
    hhgt_ctx *ctx;
    hipStream_t st;
    int stage;
    hipEvent_t a = nullptr, b = nullptr;
    StageTimer(hhgt_ctx *c, hipStream_t s, int stage_);
    void stop();
};
int hhgt_profile_collect(hhgt_ctx *ctx);

// ---- launchers (defined in the .hip files) ------------------------------------------------------
// scan.hip
int launch_scan_exclusive_u32(const uint32_t *d_in, uint32_t *d_out, uint64_t n, uint32_t *d_tmp,
                              size_t tmp_elems, hipStream_t st);
int launch_scan_exclusive_u32_pair(const uint32_t *in_a, uint32_t *out_a, const uint32_t *in_b, uint32_t *out_b, uint64_t n,
                                   uint32_t *d_tmp, size_t tmp_elems, hipStream_t st);
size_t scan_tmp_elems(uint64_t n);

// index.hip
// d_region_tot: chain_groups(n_regions) words, zero on entry; the kernels add every region's count to its group's word
int launch_index_newlines(const uint8_t *d_text, uint64_t n, uint32_t *d_slots, uint32_t *d_counts, uint32_t *d_region_tot,
                          uint32_t n_regions, uint32_t min_line, uint32_t S, int mode, DevCounters *d_cnt, hipStream_t st);
int index_mode_default();
// Everything after the newline index is sized by a host-side BOUND on the line count (max_lines) and reads the
// actual count (d_nlines, written by k_compact_newlines) and the append position (d_cursor) from device memory, so the
// chain can be queued without a host round trip (hhgt_encode_text_async).
int launch_compact_newlines(const uint32_t *d_slots, const uint32_t *d_counts, const uint32_t *d_region_tot,
                            uint32_t n_regions, uint32_t *d_nl, uint32_t max_lines, uint32_t *d_nlines, hipStream_t st);
int launch_parse_fixed(const uint8_t *d_text, uint64_t n, const uint32_t *d_nl, const uint32_t *d_nlines,
                       uint32_t max_lines, const RegionFilter &region, uint32_t S, const LineCols &l, int mode,
                       DevCounters *d_cnt, hipStream_t st);
int launch_compact_kept(const uint8_t *d_text, uint64_t n, const uint32_t *d_nl, const uint32_t *d_nlines, uint32_t max_lines,
                        const LineCols &l, const KeptCols &k, uint32_t max_runs, const uint64_t *d_cursor, uint64_t v_capacity,
                        uint32_t ring, uint32_t *d_start, uint32_t *d_stop, uint8_t *d_ref, uint8_t *d_alt, DevCounters *d_cnt,
                        bool strided, hipStream_t st);

// encode.hip
int launch_encode_tiles(const uint8_t *d_text, uint64_t n, const uint32_t *k_soff, const uint32_t *k_meta,
                        uint32_t n_lines_bound, const uint64_t *d_cursor, LayoutDev lay, int8_t *d_G,
                        uint32_t *redo_list, uint32_t *redo_flag, DevCounters *d_cnt, hipStream_t st);
int launch_encode_general(const uint8_t *d_text, uint64_t n, const uint32_t *k_soff, const uint32_t *k_lend,
                          const uint32_t *k_meta, const uint32_t *redo_list, const uint64_t *d_cursor, LayoutDev lay,
                          int8_t *d_G, uint8_t *d_P, DevCounters *d_cnt, int n_cu, hipStream_t st);
// bit-plane form of the matrix (include/hhgt.h): 2048 plane bytes per 8 KiB block of G
int launch_encode_planes(const uint8_t *d_text, uint64_t n, const uint32_t *k_soff, const uint32_t *k_meta,
                         uint32_t n_lines_bound, const uint64_t *d_cursor, LayoutDev lay, uint8_t *d_P, int8_t *d_G,
                         uint32_t *redo_list, uint32_t *redo_flag, DevCounters *d_cnt, hipStream_t st);
int launch_pad_tail_planes(LayoutDev lay, uint64_t v_end, uint64_t vcol_begin, uint64_t vcol_end, uint8_t *d_P, hipStream_t st);
int launch_pad_tail_planes_cursor(LayoutDev lay, const uint64_t *d_cursor, uint8_t *d_P, hipStream_t st);
int launch_planes_expand(LayoutDev lay, const uint8_t *d_P, const uint8_t *d_G, uint32_t col0, uint32_t n_cols, uint8_t *d_out, hipStream_t st);
int launch_pad_tail(LayoutDev lay, uint64_t v_end, uint64_t vcol_begin, uint64_t vcol_end, int8_t *d_G,
                    hipStream_t st);
// zero [*d_cursor, round_up(*d_cursor, Vc)) of the cursor's chunk column and the sample padding rows of that column
int launch_pad_tail_cursor(LayoutDev lay, const uint64_t *d_cursor, int8_t *d_G, hipStream_t st);

// lz4.hip
size_t lz4_slot_bytes(int neblock);
// d_planes != NULL: the chunks exist as bit planes (hhgt.h "Bit-plane form"); d_src then only supplies the bytes of calls
// beyond 0 / 1 / missing and may be NULL
int launch_lz4_blocks(const uint8_t *d_src, const uint8_t *d_planes, PlanesGeom pg, uint64_t n_chunks, uint64_t chunk_nbytes, int typesize,
                      int blocksize, uint8_t *d_scratch, size_t slot_bytes, uint32_t *d_csize, int clevel, uint32_t *d_flags, uint32_t tag,
                      hipStream_t st);
// d_flags (one word, zero once; may be NULL) + tag (a value no earlier call on this word used, not 0): the bit-plane coder
// notes in it whether it left streams marked, and the scanning launch behind returns at once when it did not
// lz4bits.hip: typesize 2, 8 KiB blocks; streams it cannot code get csize = 0xFFFFFFFF
int launch_lz4_bitplanes(const uint8_t *d_src, bool planes, PlanesGeom pg, uint64_t n_blocks, uint8_t *d_scratch, size_t slot_bytes, uint32_t *d_csize,
                         int depth, uint32_t *d_flags, uint32_t tag, hipStream_t st);
// frame.hip
int launch_frame(const uint8_t *d_scratch, size_t slot_bytes, const uint32_t *d_csize, const uint8_t *d_src, const uint8_t *d_planes,
                 PlanesGeom pg, uint64_t n_chunks, uint64_t chunk_nbytes, int typesize, int blocksize, int format,
                 uint32_t *d_bstart, uint64_t *d_chunk_csize, uint8_t *d_dst, uint64_t dst_cap,
                 uint64_t *d_chunk_off, uint32_t *d_chunk_flags, hipStream_t st);
int launch_decode(const uint8_t *d_src, const uint64_t *d_chunk_off, uint64_t n_chunks, uint64_t chunk_nbytes,
                  int typesize, int blocksize, uint8_t *d_dst, unsigned long long *d_bad, hipStream_t st);
int launch_decode_sel(const hhgt_block_sel *d_sel, uint32_t n_sel, uint64_t chunk_nbytes, int typesize, int blocksize,
                      uint8_t *d_dst, unsigned long long *d_bad, hipStream_t st);
int launch_count_alleles(const hhgt_count_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc, int blocksize,
                         uint32_t *d_counts, uint64_t n_out, unsigned long long *d_bad, hipStream_t st);
int launch_count_samples(const hhgt_sample_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc, int blocksize,
                         const uint32_t *d_vmask, uint64_t vmask_words, uint32_t *d_counts, uint64_t n_out,
                         unsigned long long *d_bad, hipStream_t st);
int launch_genotype_planes(const hhgt_plane_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc, int blocksize,
                           const uint32_t *d_vmask, uint64_t vmask_words, uint32_t *d_planes, uint64_t n_rows,
                           uint64_t row_words, unsigned long long *d_bad, hipStream_t st);
int launch_gather_calls(const hhgt_gather_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc, int blocksize,
                        const uint32_t *d_vmask, uint64_t vmask_words, const uint32_t *d_row_map, uint64_t n_map,
                        const void *d_values, int elem_bytes, void *d_out, uint64_t n_rows, uint64_t n_cols,
                        uint64_t row_stride, unsigned long long *d_bad, hipStream_t st);
// pairs.hip
int launch_pair_counts(const uint32_t *d_planes, uint32_t n_rows, uint64_t row_words, uint64_t w_lo, uint64_t w_hi,
                       uint32_t *d_table, hipStream_t st);
// grm.hip
int launch_grm(const uint32_t *d_planes, uint32_t n_rows, uint64_t row_words, uint64_t w_lo, uint64_t w_hi, const float *d_z,
               double *d_table, hipStream_t st);
// ld.hip
int launch_variant_planes(const uint32_t *d_planes, uint32_t n_rows, uint64_t row_words, uint64_t w_lo, uint64_t w_hi,
                          uint32_t *d_vplanes, hipStream_t st);
int launch_ld_counts(const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, uint32_t window, uint32_t *d_table,
                     hipStream_t st);
uint32_t ld_walk_words(uint32_t window);
int launch_ld_exceeds(const uint32_t *d_table, uint64_t n_var, uint32_t window, double r2, uint64_t *d_bits, hipStream_t st);
int launch_ld_walk(const uint64_t *d_bits, uint64_t n_var, uint32_t window, uint8_t *d_keep, hipStream_t st);
int launch_ld_decisions(const uint32_t *d_table, uint64_t n_var, uint32_t window, double r2, const int64_t *d_pos, int64_t max_dist,
                        uint64_t *d_bits, hipStream_t st);
// clump.hip
#define CLUMP_BATCH 8u      // rounds between two reads of the counters
// hhgt_ld_clump's workspace, carved out of one buffer: uint64 fwd [n][nq] (bit d: linked with variant k + 1 + d), uint64
// blk [n][2 nq] (the blockers: nq words back, nq words forward), uint8 state [2][n], uint32 counters [CLUMP_BATCH]
struct ClumpWs {
    uint64_t *fwd, *blk;
    uint32_t *counters;
    uint8_t *state[2];
    static size_t bytes(uint64_t n, uint32_t nq) { return (size_t)n * nq * 24u + CLUMP_BATCH * 4u + 2u * (size_t)n; }
    ClumpWs(void *p, uint64_t n, uint32_t nq)
    {
        fwd = reinterpret_cast<uint64_t *>(p), blk = fwd + n * nq;
        counters = reinterpret_cast<uint32_t *>(blk + 2u * n * nq);
        state[0] = reinterpret_cast<uint8_t *>(counters + CLUMP_BATCH), state[1] = state[0] + n;
    }
};
int launch_clump_blockers(const uint64_t *d_bits, uint64_t n_var, uint32_t window, const uint32_t *d_rank, const uint8_t *d_eligible,
                          const ClumpWs &ws, hipStream_t st);
int launch_clump_round(uint64_t n_var, uint32_t window, const ClumpWs &ws, uint32_t from, uint32_t *d_counter, hipStream_t st);
int launch_clump_owners(const uint64_t *d_bits, uint64_t n_var, uint32_t window, const uint32_t *d_rank, const ClumpWs &ws,
                        uint32_t from, int32_t *d_owner, hipStream_t st);
// assoc.hip
int launch_assoc_sums(const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, const double *d_w, uint32_t n_cols,
                      double *d_sums, hipStream_t st);
// quad.hip
int launch_quad_forms(const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, const double *d_coef, const double *d_a, double *d_q,
                      hipStream_t st);
// logistic.hip
int launch_logistic_fit(const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, const uint32_t *d_valid, const double *d_x,
                        uint32_t q, const double *d_y, const double *d_beta0, double *d_out, hipStream_t st);
// score.hip
uint64_t score_spans(uint64_t n_words);   // spans of a range of n_words words: rows of d_part
int launch_score_sums(const uint32_t *d_planes, uint32_t n_rows, uint64_t row_words, uint64_t w_lo, uint64_t w_hi, const double *d_w,
                      uint32_t n_cols, double *d_part, double *d_sums, hipStream_t st);
// region.hip
int launch_region_sums(const uint32_t *d_planes, uint32_t n_rows, uint64_t row_words, const double *d_w, uint32_t n_cols,
                       const int64_t *d_pieces, uint64_t n_pieces, const int64_t *d_runs, uint64_t n_runs, uint64_t n_slots,
                       uint64_t n_regions, double *d_part, double *d_sums, unsigned long long *d_bad, hipStream_t st);
int launch_inflate(const uint8_t *d_src, uint64_t src_bytes, const uint64_t *d_comp_off, const uint32_t *d_comp_len,
                   const uint64_t *d_out_off, const uint32_t *d_isize, uint64_t n_members, uint8_t *d_dst,
                   uint64_t dst_bytes, uint32_t *d_status, const uint32_t *d_crc32, const uint32_t *d_x2n, hipStream_t st);
void crc32_x2n_table(uint32_t *t /*[32]*/);

// layout helper shared by host and device
static inline __host__ __device__ uint64_t layout_offset(const LayoutDev &L, uint32_t s, uint64_t v)
{
    uint64_t vcol = v / L.Vc, vin = v - vcol * L.Vc;
    if (L.ring) vcol %= L.ring;
    uint32_t scol = (L.sc_log2 >= 31) ? 0u : (s >> L.sc_log2);
    uint32_t sin = s - scol * L.Sc;
    return (((vcol * L.n_sc + scol) * L.Sc + sin) * L.Vc + vin) * 2ull;
}
