// encode.hip — GT text -> int8 genotype tiles on gfx950 (CDNA4).
//
// Replaces the reference's per-record, per-sample loop
//   var.getGenotypes(gt); phase1 = (int8)gt[0]; phase2 = (int8)gt[1]   /root/reference/cpp/parse_vcf.cpp:45-52
//   '.' -> -9, else allele index                                        /root/reference/cpp/vcfpp.h:546-588
// (and htslib's vcf_parse_format GT tokeniser behind it) by ONE pass over the sample columns of all
// kept lines that emits every sample at once as G[s, v', 2].
//
// k_encode_tiles (fixed-width lines "a|b\t" x S — the 1000G shape): a 256-thread workgroup owns a
//   TL_V-variant x 256-sample tile (TL_V = 64: 32 KiB of LDS, four workgroups per CU).  Wave w reads
//   TL_V/4 lines; lane l reads 16 contiguous bytes (4 samples) of each line, so every wave-load is a coalesced
//   1 KiB run of raw GT bytes.  Each lane packs its 4 samples x TL_V/4 variants in registers, the tile is
//   transposed through an XOR-swizzled LDS image (conflict-free ds_write_b128 / ds_read_b128) and leaves as
//   2*TL_V-byte sample-row segments.
//   HBM roofline: algorithmic bytes per variant = 4*S read + 2*S written; no MFMA (byte work).
// k_encode_general (anything else: GT:DP columns, multi-digit alleles, haploid calls ...): one wave
//   per line, tab-rank by ballot/prefix over 1 KiB pieces, htslib GT rule per field.
#include "common.h"

// -------------------------------------------------------------------------------------------------
// what the three encode kernels share
typedef uint32_t u32x4_unaligned __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t u32x4_al __attribute__((ext_vector_type(4)));
constexpr uint32_t FILL_FIELD = 0x09307C30u;  // "0|0\t"
// Text near its end, the one careful load behind the kernels' hot ones.  room16: how many of the 16 bytes at `at` lie inside the
// text; tail4_or: the dword at p of which `room` bytes exist, every byte past them reads `fill`; load16_or: 16 bytes read so.
__device__ __forceinline__ uint32_t room16(uint64_t n, uint64_t at) { return at >= n ? 0u : (n - at >= 16ull ? 16u : (uint32_t)(n - at)); }
__device__ __forceinline__ uint32_t tail4_or(const uint8_t *p, uint32_t room, uint32_t fill)
{
    uint32_t x = 0;
#pragma unroll
    for (uint32_t bb = 0; bb < 4u; ++bb) x |= (bb < room ? (uint32_t)p[bb] : fill) << (bb * 8u);
    return x;
}

__device__ __forceinline__ uint4 load16_or(const uint8_t *__restrict__ text, uint64_t n, uint64_t at, uint32_t fill)
{
    const uint32_t room = room16(n, at);
    if (room == 16u) {
        const u32x4_unaligned t = *reinterpret_cast<const u32x4_unaligned *>(text + at);
        return make_uint4(t.x, t.y, t.z, t.w);
    }
    uint32_t w[4];
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) w[q] = tail4_or(text + at + 4u * q, room > 4u * q ? room - 4u * q : 0u, fill);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// Where a tile (or, for the variable-width kernel, one line) stands: gv0 = its first global column, k0 = the batch-local
// kept index of that column (negative: the tile straddles the append position), (vcol, vin) = the chunk column slot — ring
// wrap applied — and the variant inside it; live = there is a kept line at or behind k0 and the column is inside the matrix.
struct TilePlace {
    uint64_t gv0, vcol, vin;
    long long k0;
    bool live;
};
// global column v -> its chunk column slot (ring wrap applied) and the variant inside it
__device__ __forceinline__ void column_of(const LayoutDev &lay, uint64_t v, uint64_t *vcol, uint64_t *vin)
{
    *vcol = v / lay.Vc;
    *vin = v - *vcol * lay.Vc;
    if (lay.ring) *vcol %= lay.ring;
}
// the tile of `width` columns that is `tile` tiles behind the one that holds the append position v_base
__device__ __forceinline__ TilePlace tile_place(const LayoutDev &lay, uint64_t v_base, uint32_t n_kept, uint32_t width, uint64_t tile)
{
    TilePlace t;
    t.gv0 = (v_base / width + tile) * (uint64_t)width;
    t.k0 = (long long)t.gv0 - (long long)v_base;
    t.live = t.k0 < (long long)n_kept && (lay.ring || t.gv0 < lay.v_capacity);
    column_of(lay, t.gv0, &t.vcol, &t.vin);
    return t;
}

// a line of the fixed-width kernels that holds a field they cannot decode goes to the variable-width kernel, once
__device__ __forceinline__ void send_to_general(uint32_t k, uint32_t *__restrict__ redo_list, uint32_t *__restrict__ redo_flag, DevCounters *cnt)
{
    if (atomicExch(&redo_flag[k], 1u) == 0u) {
        unsigned long long slot = atomicAdd(&cnt->n_general, 1ull);
        redo_list[slot] = k;
    }
}

// One field "a|b" + terminator in a dword (little endian: a, sep, b, terminator) over the alphabet {0, 1, .} x {|, /} —
// branch-free SWAR on x ^ "0|0\t": an allele byte must be 0x00, 0x01 or 0x1E ('.'), bit 4 of it is the EXC bit and
// bit 0 | bit 4 the ONE bit; the separator byte 0x00 or 0x53 ('/').  one / exc: bit 0 = haplotype 0, bit 16 = haplotype 1;
// off != 0: a field outside the alphabet.  The terminator rule is the caller's: EXACT_TAB folds "it is a tab" into `off` (the
// tile kernel); without it the byte is not looked at (the variable-width kernel accepts a tab, a newline or ':').
struct FieldBits { uint32_t one, exc, off; };
template <bool EXACT_TAB>
__device__ __forceinline__ FieldBits classify_field(uint32_t x)
{
    FieldBits f;
    const uint32_t y = x ^ FILL_FIELD;
    const uint32_t t4 = y >> 4;
    f.exc = t4 & 0x00010001u;                                              // '.' in either allele
    f.one = (y | t4) & 0x00010001u;                                        // '1' or '.'
    const uint32_t want = __umul24(f.exc, 30u) | (y & 0x00010001u & ~f.exc);   // what the allele bytes must then be
    const uint32_t z = y & (EXACT_TAB ? 0xFF00FF00u : 0x0000FF00u), zz = z ^ 0x00005300u;   // separator (/ terminator) bytes
    f.off = ((y & 0x00FF00FFu) ^ want) | (z < zz ? z : zz);
    return f;
}

// -------------------------------------------------------------------------------------------------
// one "a|b\t" field in a dword -> h0 | h1 << 8 ; bit 31 = not a fixed-width field this path may decode
__device__ __forceinline__ uint32_t parse_field_exact(uint32_t x)
{
    uint32_t a = x & 0xFFu, sep = (x >> 8) & 0xFFu, b = (x >> 16) & 0xFFu, t = x >> 24;
    uint32_t da = a - '0', db = b - '0';
    bool ok = (sep == '|' || sep == '/') && t == '\t' && (da < 10u || a == '.') && (db < 10u || b == '.');
    uint32_t h0 = a == '.' ? 0xF7u : da;  // -9 as int8
    uint32_t h1 = b == '.' ? 0xF7u : db;
    return (h0 & 0xFFu) | ((h1 & 0xFFu) << 8) | (ok ? 0u : 0x80000000u);
}

__device__ __forceinline__ uint32_t parse_field(uint32_t x)
{
    // common case: both alleles are '0' or '1', separator '|', terminator '\t'
    if ((x & 0xFFFEFFFEu) == 0x09307C30u) return (x & 1u) | ((x >> 8) & 0x100u);
    return parse_field_exact(x);
}

// TL_V = variants per tile.  LDS = 256 rows x 2*TL_V bytes = 32 KiB: four workgroups share a CU, so the load, transpose and
// store phases of different tiles overlap (TL_V = 128, 64 KiB and two workgroups per CU, was the other width built).
constexpr int TL_V = 64;
constexpr int TL_LW = TL_V / 4;        // lines per wave: their 16-byte loads are all in flight together (1 KiB each)
constexpr int TL_SLOTS = TL_V / 8;     // 16-byte slots per LDS row
constexpr int TL_WSL = TL_SLOTS / 4;   // slots per row owned by one wave
// The lane's 4 fields of each of the wave's lines kw .. kw + TL_LW - 1 as they were read; returns which of them are kept
// fixed-width lines (bit j, wave-uniform).  Any other line, and every field past the last sample, reads "0|0\t".
__device__ __forceinline__ uint32_t load_lines(uint4 (&raw)[TL_LW], const uint8_t *__restrict__ text, uint64_t n, const uint32_t *__restrict__ k_soff,
                                           const uint32_t *__restrict__ k_meta, long long kw, uint32_t n_kept, uint32_t ls, uint32_t nval)
{
    uint32_t lvalid = 0u;
#pragma unroll
    for (int j = 0; j < TL_LW; ++j) {
        const long long k = kw + j;
        bool valid = k >= 0 && k < (long long)n_kept;
        uint32_t meta = 0, soff = 0;
        if (valid) {
            meta = k_meta[k];
            soff = k_soff[k];
        }
        valid = valid && (meta & LF_FAST);
        lvalid |= valid ? 1u << j : 0u;
        uint4 v = make_uint4(FILL_FIELD, FILL_FIELD, FILL_FIELD, FILL_FIELD);
        if (valid && nval) {
            const uint64_t off = (uint64_t)soff + 4ull * ls;
            if (nval == 4u && off + 16ull <= n) {
                u32x4_unaligned t = __builtin_nontemporal_load(reinterpret_cast<const u32x4_unaligned *>(text + off));
                v = make_uint4(t.x, t.y, t.z, t.w);
            } else {
                // (field by field, each behind its own branch: the 16 bytes in one go cost the kernel 4 VGPRs and 6 SGPRs.  No
                // field of an LF_FAST line starts past the end of the text: parse_record, index.hip, sets the flag only where
                // the 4 S - 1 bytes of sample columns end inside it; reading such a field as tabs cost 2 SGPRs over the budget)
                const uint32_t room = room16(n, off);
                uint32_t d[4];
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q)
                    d[q] = q < nval && 4u * q < room ? tail4_or(text + off + 4u * q, room - 4u * q, (uint32_t)'\t') : FILL_FIELD;
                v = make_uint4(d[0], d[1], d[2], d[3]);
            }
        }
        raw[j] = v;
    }
    return lvalid;
}

// every field to its two int8 calls: acc[q][c] holds sample q's calls of lines 2 c (low half) and 2 c + 1
__device__ __forceinline__ void pack_lines(const uint4 (&raw)[TL_LW], uint32_t lvalid, uint32_t (&acc)[4][TL_LW / 2], uint32_t last_q, long long kw, uint32_t lane,
                                           uint32_t *__restrict__ redo_list, uint32_t *__restrict__ redo_flag, DevCounters *cnt)
{
#pragma unroll
    for (int j = 0; j < TL_LW; ++j) {
        uint32_t x[4] = {raw[j].x, raw[j].y, raw[j].z, raw[j].w};
        uint32_t bad = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t xx = x[q];
            // the last sample of a line is terminated by the line end, not by a tab (LF_FAST already pinned where it ends)
            if ((uint32_t)q == last_q) xx = (xx & 0x00FFFFFFu) | 0x09000000u;
            uint32_t r = parse_field(xx);
            bad |= r;
            acc[q][j >> 1] |= (r & 0xFFFFu) << ((j & 1) * 16);
        }
        if ((lvalid >> j) & 1u) {
            unsigned long long bm = __ballot((bad & 0x80000000u) != 0u);
            if (bm != 0ull && lane == 0) send_to_general((uint32_t)(kw + j), redo_list, redo_flag, cnt);
        }
    }
}

// registers -> LDS (sample-major rows; wave w owns byte columns [w * TL_V/2, (w+1) * TL_V/2) of every row), one barrier,
// LDS -> HBM: each row leaves as one contiguous 2*TL_V-byte run (TL_SLOTS lanes x 16 B)
__device__ __forceinline__ void transpose_out(uint4 *tile, const uint32_t (&acc)[4][TL_LW / 2], const TilePlace &at, const LayoutDev &lay,
                                              int8_t *__restrict__ G, uint32_t s0, uint32_t w, uint32_t lane)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t row = 4u * lane + q;
        const uint32_t swz = (row >> 2) & 7u;
#pragma unroll
        for (int c = 0; c < TL_WSL; ++c) {
            const uint32_t slot = (w * TL_WSL + c) ^ (swz & (TL_SLOTS - 1));
            tile[row * TL_SLOTS + slot] = make_uint4(acc[q][c * 4 + 0], acc[q][c * 4 + 1], acc[q][c * 4 + 2], acc[q][c * 4 + 3]);
        }
    }
    __syncthreads();
    const uint32_t c16 = threadIdx.x & (TL_SLOTS - 1);
    const long long kfirst = at.k0 + (long long)c16 * 8;  // batch-local kept index of this lane's 8 columns
    constexpr int ROWS_PER_IT = 256 / TL_SLOTS;
#pragma unroll 4
    for (int it = 0; it < TILE_S / ROWS_PER_IT; ++it) {
        const uint32_t row = it * ROWS_PER_IT + (threadIdx.x / TL_SLOTS);
        const uint32_t s = s0 + row;
        if (s >= lay.S) continue;
        const uint32_t swz = (row >> 2) & 7u;
        uint4 v = tile[row * TL_SLOTS + (c16 ^ (swz & (TL_SLOTS - 1)))];
        int8_t *dst = G + matrix_at(lay, at.vcol, s, at.vin) + c16 * 16u;
        if (kfirst >= 0) {
            __builtin_nontemporal_store(u32x4_al{v.x, v.y, v.z, v.w}, reinterpret_cast<u32x4_al *>(dst));
        } else if (kfirst + 8 > 0) {  // tile straddles v_base: keep the columns the previous batch wrote
            uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (kfirst + e >= 0)
                    reinterpret_cast<uint16_t *>(dst)[e] = (uint16_t)(d[e >> 1] >> ((e & 1) * 16));
        }
    }
}

__global__ __launch_bounds__(256, 4) void k_encode_tiles(
    const uint8_t *__restrict__ text, uint64_t n, const uint32_t *__restrict__ k_soff,
    const uint32_t *__restrict__ k_meta, const uint64_t *__restrict__ d_cursor, LayoutDev lay, int8_t *__restrict__ G,
    uint32_t *__restrict__ redo_list, uint32_t *__restrict__ redo_flag, DevCounters *cnt)
{
    __shared__ uint4 tile[TILE_S * TL_SLOTS];  // 256 rows x 2*TL_V B, 16-byte slots XOR-swizzled by (row >> 2) & 7
    // (*d_cursor) append position: device-resident, so a chain of calls needs no host round trip
    const uint32_t n_kept = (uint32_t)cnt->n_kept;
    const TilePlace at = tile_place(lay, *d_cursor, n_kept, TL_V, blockIdx.x);
    if (!at.live) return;
    const uint32_t s0 = blockIdx.y * TILE_S;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t S = lay.S;
    const uint32_t ls = s0 + 4u * lane;                                 // first sample of this lane
    const uint32_t nval = ls >= S ? 0u : (S - ls >= 4u ? 4u : S - ls);  // samples this lane owns
    const uint32_t last_q = (S - 1u >= ls && S - 1u < ls + 4u) ? S - 1u - ls : 4u;  // which dword is sample S-1
    const long long kw = at.k0 + (long long)(w * TL_LW);                // the wave's first line
    uint4 raw[TL_LW];
    uint32_t acc[4][TL_LW / 2] = {};
    const uint32_t lvalid = load_lines(raw, text, n, k_soff, k_meta, kw, n_kept, ls, nval);
    pack_lines(raw, lvalid, acc, last_q, kw, lane, redo_list, redo_flag, cnt);
    transpose_out(tile, acc, at, lay, G, s0, w, lane);
}

// -------------------------------------------------------------------------------------------------
// k_encode_planes: the same pass as k_encode_tiles for callers whose only consumer of the matrix is the compressor —
// two BITS per allele instead of a byte (include/hhgt.h "Bit-plane form"): ONE (allele 1, or missing) and EXC (anything
// but 0 / 1), so what crosses HBM between the two halves of the path is S/2 bytes per variant each way instead of 2 S.
//
// A 256-thread workgroup owns one plane tile (PL_TILE = 256 variants) of a band of PT_S = 252 samples; wave w reads lines
// [64 w, 64 w + 64) of the tile in groups of lines whose loads are in flight together (one 16-byte-aligned 1 KiB window per
// line: pl_load_window; lanes 0..62 own 4 samples each, lane 63 loads but owns nothing); where a group's line starts come
// from: pl_load_step.  Each lane's four fields are rebuilt from its chunk and its neighbour's just before packing
// (pl_funnel).  Packing is SWAR on the field dword "a|b\t": (x & 0x00010001) holds the
// two allele bits, shifted by the line number they accumulate into a register whose low half is haplotype 0 and whose
// high half is haplotype 1 over 16 lines; one xor/or chain per line tells whether all four fields of the lane were
// "[01]|[01]\t" (pl_pack_group: what happens otherwise).  Per 32 lines a lane holds one dword per (sample, plane, kind):
// 16 ds_write_b32 into a 32 KiB image [kind][plane][sample][32 B] (rows 0..251 are the band's); after one barrier the
// image leaves as four contiguous 8064-byte runs — the planes are TILE-MAJOR in HBM (common.h) for exactly that.  The tile
// that straddles the append position merges with the bits the previous call wrote.
// HBM roofline: algorithmic bytes per variant = 4 S read + S/2 written.  Why 252 samples and not 256: a band's fields are
// 1008 bytes, so with any start phase they fit one 16-byte-aligned 1 KiB window, one load instruction per line and wave
// with every lane aligned.  Lanes that load at the (arbitrary) byte where the sample columns start run ~20 % slower
// (tools/micro/strided_read.hip: 6.4 -> 5.1 TB/s), and a 256-sample band needs a 65th aligned chunk per line.
constexpr int PT_S = 252;             // samples per band: 63 owner lanes x 4 (TILE_S stays k_encode_tiles')
constexpr int PT_V = 256;             // = PL_TILE
constexpr int PT_ROWDW = PT_V / 32;   // dwords per image row
constexpr int PT_NW = 4;              // waves per workgroup
constexpr int PT_LW = PT_V / PT_NW;   // lines per wave
constexpr int PT_G = 8;               // lines per load group; the next group's loads are issued before a group is packed
constexpr int PT_NG = 32 / PT_G;      // load groups per step of 32 lines
constexpr int PT_WGS = 4;             // waves per SIMD the register allocation leaves room for (= workgroups per CU)
struct PlGroup {
    uint4 raw[PT_G];
    uint32_t lvalid;   // bit j: line j of the group is a kept fixed-width line (wave-uniform)
    uint32_t lstride;  // bit j: line j is a kept record whose columns are all of one width of 5 .. 8 bytes, GT first (k_meta bits 20-23)
};
// the line table of 32 lines at once: lane j holds soff / meta of line kb + j (meta = 0 beyond the batch), so that a
// load group needs no scalar loads (the first version paid two dependent s_load round trips in front of every line)
struct PlStep { uint32_t soff, meta; };
// What a wave keeps for its tile, and `stp` for a step of 32 lines (index.hip's HopState is the model): s0 = the band's first
// sample, ls / nval = the lane's first sample and how many it owns (lane 63 none), rel = (S - 1) - ls for pl_edge_fields
struct PlWave {
    const uint8_t *__restrict__ text;
    uint64_t n;
    PlStep stp;
    uint32_t s0, ls, nval, lane, S;
    int rel;
    uint32_t *__restrict__ redo_list, *__restrict__ redo_flag;
    DevCounters *cnt;
    __device__ __forceinline__ uint32_t soff(int j) const { return (uint32_t)__builtin_amdgcn_readlane((int)stp.soff, j); }
    __device__ __forceinline__ uint32_t meta(int j) const { return (uint32_t)__builtin_amdgcn_readlane((int)stp.meta, j); }
};
__device__ __forceinline__ PlStep pl_load_step(const uint32_t *__restrict__ k_soff, const uint32_t *__restrict__ k_meta, long long kb,
                                               uint32_t n_kept, uint32_t lane)
{
    PlStep t;
    const long long k = kb + (long long)(lane & 31u);
    const bool valid = k >= 0 && k < (long long)n_kept;
    t.soff = valid ? k_soff[k] : 0u;
    t.meta = valid ? k_meta[k] : 0u;
    return t;
}

// Lane `lane`'s 16-byte chunk of the aligned 1 KiB window that covers the band's fields of one line: the band's fields
// start at F = soff + 4 s0 (s0 = 252 b, so F = soff + 1008 b and F's phase against 16 bytes is the line's, whatever the
// band), the window at F minus that phase (the text itself starts on a 16-byte boundary: api.hip checks).  The window may
// reach up to 12 bytes past the line's end (the band behind it has fewer than 4 samples) or into the bytes in front of F
// (band 0): none of those bytes is a field this lane owns, and the window has to stay inside the text only.  EDGE (k_encode_planes: the
// last band, and any band of a tile whose last line's window could end past the text) reads a window that would end past
// the text's end with care, and what lies past the end reads as a tab; every other tile reads flat.
template <bool EDGE>
__device__ __forceinline__ uint4 pl_load_window(const PlWave &w, uint32_t soff)
{
    const uint64_t F = (uint64_t)soff + 4ull * w.s0;
    const uint64_t A = F & ~15ull;
    const uint64_t off = A + 16ull * w.lane;
    if (!EDGE || A + 1024ull <= w.n) {   // (wave-uniform)
        const u32x4_al t = __builtin_nontemporal_load(reinterpret_cast<const u32x4_al *>(w.text + off));
        return make_uint4(t.x, t.y, t.z, t.w);
    }
    return load16_or(w.text, w.n, off, (uint32_t)'\t');
}

// The lane's four fields from its window chunk c and lane + 1's: bytes [d, d + 16) of the 32 (d = the line's phase,
// wave-uniform).  Four DPP moves (wave_shl:1; lane 63 gets zeros — it owns nothing), dwords d >> 2 .. (d >> 2) + 4 of the
// eight by two v_cndmask stages on the bits of d >> 2 (as lane masks: a uniform select of an array element becomes a
// scratch round trip), v_alignbyte by d & 3.
__device__ __forceinline__ uint4 pl_funnel(const uint4 c, const uint32_t d)
{
    const uint32_t w[8] = {c.x, c.y, c.z, c.w,
                           (uint32_t)__builtin_amdgcn_mov_dpp((int)c.x, 0x130, 0xf, 0xf, true),
                           (uint32_t)__builtin_amdgcn_mov_dpp((int)c.y, 0x130, 0xf, 0xf, true),
                           (uint32_t)__builtin_amdgcn_mov_dpp((int)c.z, 0x130, 0xf, 0xf, true),
                           (uint32_t)__builtin_amdgcn_mov_dpp((int)c.w, 0x130, 0xf, 0xf, true)};
    const bool k2 = __builtin_amdgcn_inverse_ballot_w64((d & 8u) ? ~0ull : 0ull);
    const bool k1 = __builtin_amdgcn_inverse_ballot_w64((d & 4u) ? ~0ull : 0ull);
    uint32_t t[6], u[5];
#pragma unroll
    for (int i = 0; i < 6; ++i) t[i] = k2 ? w[i + 2] : w[i];
#pragma unroll
    for (int i = 0; i < 5; ++i) u[i] = k1 ? t[i + 1] : t[i];
    const uint32_t r = d & 3u;
    return make_uint4(__builtin_amdgcn_alignbyte(u[1], u[0], r), __builtin_amdgcn_alignbyte(u[2], u[1], r),
                      __builtin_amdgcn_alignbyte(u[3], u[2], r), __builtin_amdgcn_alignbyte(u[4], u[3], r));
}

// the band that holds the last sample: fields the lane does not own read "0|0\t", and the last sample of the line is
// terminated by the line end (LF_FAST pinned where it ends).  rel = (S - 1) - (the lane's first sample): field q is
// owned if q < rel, the last sample's if q == rel.
template <bool EDGE>
__device__ __forceinline__ uint4 pl_edge_fields(uint4 v, int rel)
{
    if (EDGE) {
        uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t keep = rel > q ? 0xFFFFFFFFu : (rel == q ? 0x00FFFFFFu : 0u);
            x[q] = (x[q] & keep) | (FILL_FIELD & ~keep);
        }
        v = make_uint4(x[0], x[1], x[2], x[3]);
    }
    return v;
}

struct __attribute__((packed)) PlU32 { uint32_t v; };
// the raw window chunks of the PT_G lines of group g of the step (the funnel waits for pl_pack_group: the chunks in flight
// stay 4 registers per line)
template <bool EDGE>
__device__ __forceinline__ void pl_load_group(const PlWave &w, PlGroup &gr, const int g)
{
    uint32_t lv = 0, lst = 0;
#pragma unroll
    for (int j = 0; j < PT_G; ++j) {
        const uint32_t meta = w.meta(g * PT_G + j);
        const uint32_t soff = w.soff(g * PT_G + j);
        uint4 v = make_uint4(FILL_FIELD, FILL_FIELD, FILL_FIELD, FILL_FIELD);
        if (meta & LF_FAST) {   // (wave-uniform)
            lv |= 1u << j;
            v = pl_load_window<EDGE>(w, soff);
        } else if ((meta >> 20) & 15u)
            lst |= 1u << j;   // decoded by the second level (pack_careful), at its stride
        gr.raw[j] = v;
    }
    gr.lvalid = lv;
    gr.lstride = lst;
}

// Level (1) of pl_pack_group: true, and the group's ONE bits in one[q], when every field of every lane is "[01]|[01]\t"
// (~14 vector instructions per line, unrolled); false, and nothing added, when some lane saw something else.
template <bool EDGE>
__device__ __forceinline__ bool pack_fast(const PlWave &w, const PlGroup &gr, const int j0, const int sh, uint32_t (&one)[4])
{
    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, bad = 0;
#pragma unroll
    for (int j = 0; j < PT_G; ++j) {
        // the line's phase (a line that was not loaded holds "0|0\t" in every dword: phase 0 keeps it so)
        const uint32_t soff = w.soff(j0 + j);   // (read outside the select: a lane read is not speculated, it would become a branch per line)
        const uint32_t d = ((gr.lvalid >> j) & 1u) ? soff & 15u : 0u;
        const uint4 x = pl_edge_fields<EDGE>(pl_funnel(gr.raw[j], d), w.rel);
        a0 |= (x.x & 0x00010001u) << (sh + j);
        a1 |= (x.y & 0x00010001u) << (sh + j);
        a2 |= (x.z & 0x00010001u) << (sh + j);
        a3 |= (x.w & 0x00010001u) << (sh + j);
        bad |= ((x.x ^ FILL_FIELD) | (x.y ^ FILL_FIELD)) | ((x.z ^ FILL_FIELD) | (x.w ^ FILL_FIELD));
    }
    bad |= gr.lstride ? 2u : 0u;   // a record decoded at its stride is the second level's (as data, not as a branch: the branch cost 86 spilled registers)
    // (lane 63 owns nothing: what it holds is the next band's, or past the line)
    if ((__builtin_amdgcn_ballot_w64((bad & 0xFFFEFFFEu) != 0u) & 0x7FFFFFFFFFFFFFFFull) != 0ull) return false;
    one[0] |= a0, one[1] |= a1, one[2] |= a2, one[3] |= a3;
    return true;
}

// Sample s's column of a record whose columns are all `wd` (5 .. 8) bytes wide with the GT sub-field first — "a|b:dd\t" — as
// the field dword "a|b\t", or all ones (a field no alphabet accepts) for a column of any other shape.  The column is checked
// where it stands: byte 3 is the ':' that ends the GT, bytes 4 .. wd - 2 hold neither a tab nor a newline (the bytes above
// read 0), byte wd - 1 is the tab (the newline behind the last sample).  lbase: wave-uniform, 32-bit lane offsets behind it
__device__ __forceinline__ uint32_t strided_field(const uint8_t *lbase, uint32_t room, uint32_t wd, uint32_t s, bool last_sample)
{
    const uint32_t shb = 8u * (wd - 5u);   // where the column's last byte sits in its second dword
    const uint32_t lowm = shb ? (1u << shb) - 1u : 0u;
    const uint32_t vo = wd * s;
    if (vo + 8u > room) return 0xFFFFFFFFu;
    const uint32_t d1 = reinterpret_cast<const PlU32 *>(lbase + vo + 4u)->v;
    const uint32_t low = d1 & lowm;
    const uint32_t t9 = low ^ 0x09090909u, tA = low ^ 0x0A0A0A0Au;
    uint32_t bad = (((t9 - 0x01010101u) & ~t9) | ((tA - 0x01010101u) & ~tA)) & 0x80808080u;
    bad |= ((d1 >> shb) & 0xFFu) ^ (last_sample ? 0x0Au : 0x09u);
    const uint32_t d0 = reinterpret_cast<const PlU32 *>(lbase + vo)->v;
    bad |= (d0 >> 24) ^ (uint32_t)':';
    return bad ? 0xFFFFFFFFu : ((d0 & 0x00FFFFFFu) | 0x09000000u);
}

// Levels (2) and (3) of pl_pack_group: the group again, line by line in a ROLLED loop that reads the (cache-hot) line once
// more and classifies every field (classify_field, exact tab).  k = the batch-local kept index of the group's first line.
template <bool EDGE>
__device__ __forceinline__ void pack_careful(const PlWave &w, const int j0, const int sh, uint32_t (&one)[4], uint32_t (&exc)[4], long long k)
{
#pragma unroll 1
    for (int j = 0; j < PT_G; ++j) {
        const uint32_t meta = w.meta(j0 + j);
        const uint32_t wd = (meta >> 20) & 15u;
        if (!(meta & LF_FAST) && wd == 0u) continue;
        const uint32_t soff = w.soff(j0 + j);
        uint32_t hard = 0;
        auto add_field = [&](uint32_t x, int q) {   // bits into one[q] / exc[q], anything outside the alphabet -> hard
            const FieldBits f = classify_field<true>(x);
            const uint32_t keep = f.off ? 0u : 0xFFFFFFFFu;
            one[q] |= (f.one & keep) << (sh + j);
            exc[q] |= (f.exc & keep) << (sh + j);
            hard |= f.off;
        };
        if (meta & LF_FAST) {   // (wave-uniform)
            const uint4 v = pl_edge_fields<EDGE>(pl_funnel(pl_load_window<EDGE>(w, soff), soff & 15u), w.rel);
            add_field(v.x, 0), add_field(v.y, 1), add_field(v.z, 2), add_field(v.w, 3);
        } else {
            // config 4's GT:DP records (round 3 sent them all to the variable-width kernel: 3.5 of config 4's 16 ms, tab
            // ranking and one atomic per nonzero call); a column of any other shape sends the line there like any other
            // surprise.  One field at a time: the first level's registers stay what they were.
            const uint64_t room64 = w.n - (uint64_t)soff;
            const uint32_t room = room64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)room64;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                add_field((uint32_t)q < w.nval ? strided_field(w.text + soff, room, wd, w.ls + (uint32_t)q, w.ls + (uint32_t)q == w.S - 1u) : FILL_FIELD, q);
        }
        const unsigned long long bm = __builtin_amdgcn_ballot_w64(hard != 0u) & 0x7FFFFFFFFFFFFFFFull;
        if (bm != 0ull && w.lane == 0) send_to_general((uint32_t)(k + j), w.redo_list, w.redo_flag, w.cnt);
    }
}

// Group g of a step (kb = the kept index of the step's first line) -> per sample q: o / e[half][q], bit sh + j (haplotype 0)
// and bit 16 + sh + j (haplotype 1) for line j of the group.  Three levels.  (1) pack_fast.  (2) some lane saw something
// else: pack_careful classifies every field over the alphabet {0, 1, .} x {|, /}.  (3) a field outside that
// alphabet (a third allele, a multi-digit index, anything malformed) contributes zero bits and sends its line to the
// variable-width kernel, which sets the bits of the whole line (idempotent for the fields that were fine here).  Keeping (2)
// rolled and out of the registers of (1) is what lets four workgroups share a CU.
template <bool EDGE>
__device__ __forceinline__ void pl_pack_group(const PlWave &w, const PlGroup &gr, const int g, uint32_t (&o)[2][4], uint32_t (&e)[2][4], long long kb)
{
    const int j0 = g * PT_G, half = j0 >> 4, sh = j0 & 15;
    if (!pack_fast<EDGE>(w, gr, j0, sh, o[half])) pack_careful<EDGE>(w, j0, sh, o[half], e[half], kb + j0);
}

// a step (32 lines; step = which of the tile's) -> image row (kind * 2 + plane) * 256 + sample, dword step ^ ((lane >> 1) & 7)
__device__ __forceinline__ void write_image(uint32_t *img, const uint32_t (&o)[2][4], const uint32_t (&e)[2][4], uint32_t step, uint32_t lane)
{
    const uint32_t c = step ^ ((lane >> 1) & 7u);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t r = (4u * lane + (uint32_t)q) * PT_ROWDW + c;
        img[r] = __builtin_amdgcn_perm(o[1][q], o[0][q], 0x05040100u);                   // ONE, haplotype 0
        img[256u * PT_ROWDW + r] = __builtin_amdgcn_perm(o[1][q], o[0][q], 0x07060302u);   // ONE, haplotype 1
        img[512u * PT_ROWDW + r] = __builtin_amdgcn_perm(e[1][q], e[0][q], 0x05040100u);   // EXC, haplotype 0
        img[768u * PT_ROWDW + r] = __builtin_amdgcn_perm(e[1][q], e[0][q], 0x07060302u);   // EXC, haplotype 1
    }
}

// image -> HBM: per kind-plane the band's 252 rows are one contiguous 8064-byte run of the tile (tile-major planes,
// common.h); rows 252..255 (lane 63's) are not the band's.  Un-swizzle in registers, then the append-position merge.
__device__ __forceinline__ void store_image(const uint32_t *img, const TilePlace &at, const LayoutDev &lay, uint8_t *__restrict__ P, uint32_t s0)
{
    const PlanesGeom pg = planes_geom(lay, 0u);
    const uint32_t tile = (uint32_t)(at.vin / PL_TILE);
    const uint32_t nkeep = at.k0 < 0 ? (uint32_t)(-at.k0) : 0u;     // leading columns that belong to the previous call
#pragma unroll 4
    for (int it = 0; it < 2048 / (64 * PT_NW); ++it) {
        const uint32_t pi = (uint32_t)it * (64u * PT_NW) + threadIdx.x;   // 16-byte piece: kp * 512 + row * 2 + half
        const uint32_t kp = pi >> 9, row = (pi >> 1) & 255u, half = pi & 1u;
        const uint32_t s = s0 + row;
        if (row >= PT_S || s >= lay.S) continue;
        const uint32_t sw = (row >> 3) & 7u;   // the writer's (lane >> 1) & 7: row = 4 lane + q
        const uint4 t = reinterpret_cast<const uint4 *>(img)[(kp * 256u + row) * 2u + (half ^ (sw >> 2))];
        const bool s1 = sw & 1u, s2 = sw & 2u;   // dword c of the piece sits at c ^ (sw & 3)
        const uint32_t a0 = s1 ? t.y : t.x, a1 = s1 ? t.x : t.y, a2 = s1 ? t.w : t.z, a3 = s1 ? t.z : t.w;
        uint32_t d0 = s2 ? a2 : a0, d1 = s2 ? a3 : a1, d2 = s2 ? a0 : a2, d3 = s2 ? a1 : a3;
        uint8_t *dst = P + planes_piece(pg, at.vcol, tile, kp, s) + half * 16u;
        if (nkeep) {   // (workgroup-uniform) the tile straddles the append position
            const uint32_t b0 = half * 128u;
            if (b0 + 128u <= nkeep) continue;
            if (b0 < nkeep) {
                const uint4 old = *reinterpret_cast<const uint4 *>(dst);
                const uint32_t nb = nkeep - b0;   // 1..127 low bits stay
                const uint32_t ov[4] = {old.x, old.y, old.z, old.w};
                uint32_t d[4] = {d0, d1, d2, d3};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t km = nb >= 32u * (i + 1) ? 0xFFFFFFFFu : (nb <= 32u * i ? 0u : ((1u << (nb - 32u * i)) - 1u));
                    d[i] = (ov[i] & km) | (d[i] & ~km);
                }
                d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
            }
        }
        __builtin_nontemporal_store(u32x4_al{d0, d1, d2, d3}, reinterpret_cast<u32x4_al *>(dst));
    }
}

template <bool EDGE>
__device__ __forceinline__ void encode_planes_tile(PlWave &w, const uint32_t *__restrict__ k_soff, const uint32_t *__restrict__ k_meta,
                                                   uint32_t n_kept, const TilePlace &at, const LayoutDev &lay, uint8_t *__restrict__ P, uint32_t *img)
{
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long kw = at.k0 + (long long)(wv * PT_LW);
    PlStep nxt = pl_load_step(k_soff, k_meta, kw, n_kept, w.lane);
#pragma unroll 1
    for (int gp = 0; gp < PT_LW / 32; ++gp) {   // 32 lines -> one dword per (kind, plane, sample)
        const long long kb = kw + (long long)(gp * 32);
        w.stp = nxt;
        if (gp + 1 < PT_LW / 32) nxt = pl_load_step(k_soff, k_meta, kb + 32, n_kept, w.lane);
        uint32_t o[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, e[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        // sched_barrier(0): the instruction scheduler may not move anything across — it would otherwise hoist the loads of
        // all four groups of a step to its top (128 registers of text in flight per lane, and spills)
        if (!EDGE) {
            // two groups in flight: load B, pack A, load A, pack B
            PlGroup A, B;
            pl_load_group<EDGE>(w, A, 0);
#pragma unroll
            for (int g = 0; g < PT_NG; g += 2) {
                pl_load_group<EDGE>(w, B, g + 1);
                __builtin_amdgcn_sched_barrier(0);
                pl_pack_group<EDGE>(w, A, g, o, e, kb);
                __builtin_amdgcn_sched_barrier(0);
                if (g + 2 < PT_NG) pl_load_group<EDGE>(w, A, g + 2);
                __builtin_amdgcn_sched_barrier(0);
                pl_pack_group<EDGE>(w, B, g + 1, o, e, kb);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            // (EDGE tiles' careful path does not fit the registers next to a second group in flight: one group at a time)
#pragma unroll
            for (int g = 0; g < PT_NG; ++g) {
                PlGroup A;
                pl_load_group<EDGE>(w, A, g);
                __builtin_amdgcn_sched_barrier(0);
                pl_pack_group<EDGE>(w, A, g, o, e, kb);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        write_image(img, o, e, wv * (uint32_t)(PT_LW / 32) + (uint32_t)gp, w.lane);
    }
    __syncthreads();
    store_image(img, at, lay, P, w.s0);
}

// The band of sample columns that holds the last sample (and lanes past it) reads with care (EDGE), and so does every band
// of a tile whose last line's window could end past the text (the text's last lines, in front of a last band of 1..3
// samples): kept lines are in text order, so no line of the tile starts behind its last one.  Every other tile reads flat.
// One launch, a workgroup-uniform branch: since the medium path is a rolled loop both bodies fit the same registers, and
// the last band's tiles fill the tail of the grid instead of being an under-filled launch of their own (round 3 first split
// them: 1.2 of 7.8 ms per step).
__global__ __launch_bounds__(64 * PT_NW, PT_WGS) void k_encode_planes(
    const uint8_t *__restrict__ text, uint64_t n, const uint32_t *__restrict__ k_soff, const uint32_t *__restrict__ k_meta,
    const uint64_t *__restrict__ d_cursor, LayoutDev lay, uint8_t *__restrict__ P, int8_t *__restrict__ G,
    uint32_t *__restrict__ redo_list, uint32_t *__restrict__ redo_flag, DevCounters *cnt, uint32_t tiles_v, uint32_t tiles_s)
{
    HHGT_WAVE_PRIO();
    __shared__ __attribute__((aligned(16))) uint32_t img[1024 * PT_ROWDW];   // 32 KiB
    const uint32_t n_kept = (uint32_t)cnt->n_kept;
    // which tile: (variant tile, sample band) from the linear workgroup id.  Sample band fastest, so workgroups that run
    // together read neighbouring KiB of the same lines, and the bands of one variant tile stay on one XCD (workgroup id
    // mod 8), so the cache lines two neighbouring bands share are fetched by one L2
    const uint32_t x = blockIdx.x & 7u, q = blockIdx.x >> 3;
    const uint32_t band = q % tiles_s;
    const uint32_t tile_v = (q / tiles_s) * 8u + x;
    if (tile_v >= tiles_v) return;
    const TilePlace at = tile_place(lay, *d_cursor, n_kept, PT_V, tile_v);
    if (!at.live) return;
    bool edge = band + 1u == tiles_s;
    if (!edge) {
        const long long kl = at.k0 + (PT_V - 1) < (long long)n_kept - 1 ? at.k0 + (PT_V - 1) : (long long)n_kept - 1;
        if (kl >= 0) edge = (uint64_t)k_soff[kl] + 4ull * PT_S * band + 1024ull > n;
    }
    const uint32_t lane = threadIdx.x & 63u, S = lay.S, s0 = band * PT_S, ls = s0 + 4u * lane;
    const uint32_t nval = (lane == 63u || ls >= S) ? 0u : (S - ls >= 4u ? 4u : S - ls);
    PlWave w = {text, n, {0u, 0u}, s0, ls, nval, lane, S, lane == 63u ? -1 : (int)(S - 1u) - (int)ls, redo_list, redo_flag, cnt};
    if (edge)
        encode_planes_tile<true>(w, k_soff, k_meta, n_kept, at, lay, P, img);
    else
        encode_planes_tile<false>(w, k_soff, k_meta, n_kept, at, lay, P, img);
}

// -------------------------------------------------------------------------------------------------
// htslib vcf_parse_format GT rule (see oracle/vcf_oracle.c parse_gt for the restatement it mirrors)
template <typename RD>
__device__ __forceinline__ uint32_t parse_gt_bytes(RD rd, uint32_t p, uint32_t lim, uint32_t *n_alleles)
{
    int l = 0;
    int vals[2] = {-9, -9};
    for (;;) {
        uint32_t c = p < lim ? rd(p) : 0u;
        if (c == '.') {
            ++p;
            if (l < 2) vals[l] = -9;
            ++l;
        } else if (c - '0' < 10u) {
            long long v = 0;
            while (p < lim) {
                uint32_t d = rd(p) - '0';
                if (d >= 10u) break;
                v = v * 10 + d;
                if (v > 0x7fffffffLL) v &= 0x7fffffffLL;
                ++p;
            }
            if (l < 2) vals[l] = (int)v;
            ++l;
        } else
            break;
        c = p < lim ? rd(p) : 0u;
        if (c != '|' && c != '/') break;
        ++p;
    }
    if (l == 0) {
        vals[0] = -9;
        l = 1;
    }
    *n_alleles = (uint32_t)l;
    return ((uint32_t)vals[0] & 0xFFu) | (((uint32_t)vals[1] & 0xFFu) << 8);
}

// -------------------------------------------------------------------------------------------------
constexpr uint32_t GEN_HALO = 64u;  // bytes staged past each 1 KiB piece: a GT sub-field that starts in the piece ends inside it

// The staged piece and the column list are reached through pointers that CARRY the LDS address space.  Through a generic
// pointer variable (or as one arm of a select against the global text) the reader below lost the address space and every
// character it fetches became a flat_load — 915 global-load instructions per line, 520 us per line.
typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3))) uint16_t lds_u16;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) u32x4_al lds_u128;
// the lanes hand the staged piece and the column list to each other through LDS, which executes a wave's accesses in order: this
// keeps the COMPILER from moving a lane's read of another lane's slot across the stores (no instruction; lz4bits.hip's BP_FENCE)
__device__ __forceinline__ void gen_fence()
{
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

__device__ __forceinline__ void stage_piece(lds_u8 *piece, const uint4 cur, const uint4 hal, uint32_t lane)
{
    *reinterpret_cast<lds_u128 *>(piece + 16u * lane) = u32x4_al{cur.x, cur.y, cur.z, cur.w};
    if (lane < GEN_HALO / 16u) *reinterpret_cast<lds_u128 *>(piece + 1024u + 16u * lane) = u32x4_al{hal.x, hal.y, hal.z, hal.w};
}

// exact per-byte "== c" mask of 16 bytes (SWAR), 4 bits per dword
__device__ __forceinline__ uint32_t eq_mask16(const uint4 v, uint32_t c)
{
    const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t t = wv[q] ^ (c * 0x01010101u);
        const uint32_t z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
        m |= ((((z >> 7) * 0x01020408u) >> 24) & 0xFu) << (4 * q);
    }
    return m;
}

// the tabs of the lane's 16 bytes at b0 (one bit per byte, none at or behind the line's end); *nl_inside collects newlines
__device__ __forceinline__ uint32_t tab_and_newline_masks(const uint4 cur, uint32_t b0, uint32_t lend, uint32_t *nl_inside)
{
    const uint32_t inl = b0 >= lend ? 0u : (lend - b0 >= 16u ? 0xFFFFu : ((1u << (lend - b0)) - 1u));
    *nl_inside |= eq_mask16(cur, '\n') & inl;
    return eq_mask16(cur, '\t') & inl;
}

// the columns that start in this piece, in order: list[i] = offset of the byte behind the i-th tab; returns how many
__device__ __forceinline__ uint32_t list_columns(lds_u16 *list, uint32_t m, uint32_t lane)
{
    const uint32_t c = __popc(m);
    uint32_t nf;
    uint32_t at = wave_scan_sum_dpp(c, lane, &nf) - c, mm = m;
    while (__builtin_amdgcn_ballot_w64(mm != 0u) != 0ull) {
        const bool on = mm != 0u;
        const uint32_t j = (uint32_t)__builtin_ctz(mm | 0x10000u);
        list[on ? at : 1023u] = (uint16_t)(16u * lane + j + 1u);   // (slot 1023 is never a column's: a piece with 1024 tabs has its last one at offset 1023, written by an `on` lane)
        at += on ? 1u : 0u;
        mm &= mm - 1u;
    }
    return nf;
}

// byte p of the text: from the staged piece (and its halo), or from the text itself beyond the halo (rare long sub-fields)
struct PieceReader {
    const lds_u8 *piece;
    const uint8_t *text;
    uint32_t base, avail;
    __device__ __forceinline__ uint32_t operator()(uint32_t p) const
    {
        const uint32_t o = p - base;
        if (o < avail) return (uint32_t)piece[o];
        return (uint32_t)text[p];
    }
};

// skip gtidx sub-fields: p to the start of the GT sub-field; false when the column has none
__device__ __forceinline__ bool skip_to_gt(const PieceReader &rd, uint32_t &p, uint32_t lend, uint32_t gtidx)
{
    for (uint32_t gsk = 0; gsk < gtidx; ++gsk) {
        while (p < lend && rd(p) != ':' && rd(p) != '\t') ++p;
        if (p < lend && rd(p) == ':') ++p;
        else return false;
    }
    return true;
}

// the common column: GT reads "a|b" / "a/b" with a, b in {0, 1, .}, closed by ':', a tab or the line end.  Four bytes from
// the staged piece (two aligned dwords, one funnel shift) through classify_field; the terminator is judged here
__device__ __forceinline__ bool common_column(const PieceReader &rd, uint32_t p, uint32_t lend, uint32_t *hv)
{
    const bool inb = p - rd.base + 8u <= rd.avail;
    const uint32_t o = inb ? p - rd.base : 0u;
    const lds_u32 *w32 = reinterpret_cast<const lds_u32 *>(rd.piece);
    uint32_t x = __builtin_amdgcn_alignbyte(w32[(o >> 2) + 1u], w32[o >> 2], o & 3u);
    if (p + 3u >= lend) x = (x & 0x00FFFFFFu) | 0x09000000u;   // the line (and the text) ends behind the call
    const FieldBits f = classify_field<false>(x);
    const uint32_t yt = (x ^ FILL_FIELD) >> 24;                     // terminator: '\t', '\n' or ':'
    const bool done = inb & (f.off == 0u) & ((yt == 0u) | (yt == 0x03u) | (yt == 0x33u)) & (p + 3u <= lend);
    const uint32_t h0 = (f.exc & 1u) ? 0xF7u : (f.one & 1u), h1 = (f.exc >> 16) ? 0xF7u : (f.one >> 16);
    *hv = h0 | (h1 << 8);
    return done;
}

// Where a line's calls go in the bit-plane form (wave-uniform: the line's tile and bit are the same for every sample):
// word = sample 0's dword of kind-plane 0, kstride = dwords between the kind-planes of a tile
struct PlaneLine { uint8_t *word; uint64_t kstride; uint32_t pmask; };
__device__ __forceinline__ PlaneLine plane_line(const PlanesGeom &pg, const TilePlace &at, uint8_t *P)
{
    const uint32_t tile = (uint32_t)(at.vin / PL_TILE), bit = (uint32_t)(at.vin % PL_TILE);
    return {P + planes_piece(pg, at.vcol, tile, 0u, 0u) + ((bit >> 5) << 2), (uint64_t)pg.S_pad * 8ull, 1u << (bit & 31u)};
}

// (the bytes of calls beyond 0 / 1 / missing go to their place in G — 64-bit multiplies: only where needed)
__device__ __forceinline__ void emit_planes(const PlaneLine &pl, const LayoutDev &lay, const TilePlace &at, bool act, uint32_t s, uint32_t hv,
                                            int8_t *__restrict__ G, uint32_t *n_other)
{
    const uint32_t h0 = hv & 0xFFu, h1 = (hv >> 8) & 0xFFu;
    // kind-planes of a tile: ONE of haplotype 0, ONE of haplotype 1, EXC of haplotype 0, EXC of haplotype 1
    const bool bk[4] = {act && (h0 == 1u || h0 == 0xF7u), act && (h1 == 1u || h1 == 0xF7u), act && h0 > 1u, act && h1 > 1u};
    uint32_t *pw = reinterpret_cast<uint32_t *>(pl.word + (uint64_t)s * 32ull);
    if (bk[0]) atomicOr(pw, pl.pmask);
    if (bk[1]) atomicOr(pw + pl.kstride, pl.pmask);
    if (bk[2]) atomicOr(pw + 2ull * pl.kstride, pl.pmask);
    if (bk[3]) atomicOr(pw + 3ull * pl.kstride, pl.pmask);
    if (bk[2] && h0 != 0xF7u) {
        ++*n_other;
        if (G) G[matrix_at(lay, at.vcol, s, at.vin)] = (int8_t)h0;
    }
    if (bk[3] && h1 != 0xF7u) {
        ++*n_other;
        if (G) G[matrix_at(lay, at.vcol, s, at.vin) + 1ull] = (int8_t)h1;
    }
}

__device__ __forceinline__ void wave_totals(DevCounters *cnt, uint32_t haploid, uint32_t malformed, uint32_t n_other, uint32_t lane)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        haploid += __shfl_down(haploid, d, 64);
        n_other += __shfl_down(n_other, d, 64);
    }
    if (lane == 0) {
        if (haploid) atomicAdd(&cnt->n_haploid, (unsigned long long)haploid);
        if (malformed) atomicAdd(&cnt->n_malformed, (unsigned long long)malformed);
        if (n_other) atomicAdd(&cnt->n_other, (unsigned long long)n_other);
    }
}

// PLANES: the bit-plane form (k_encode_planes wrote zeros for every call of the lines this kernel owns; the bits are set
// by atomic or, the bytes of calls beyond 0 / 1 / missing go to their place in G).
// One wave per line, 1 KiB pieces.  Lane l holds bytes [16 l, 16 l + 16) of the piece and finds its tabs (one bit per
// byte); a wave scan numbers them, and every lane writes where the columns behind its tabs start into a list in LDS.
// Then the COLUMNS are dealt to the lanes, 64 consecutive samples per round: four bytes at the column's start from the
// staged piece, the branch-free {0, 1, .} x {|, /} classification of the tile kernel's second level (anything else:
// the byte walk of the GT rule, lane by lane), and the round's ONE / EXC bits of both haplotypes are four ballots —
// the nonzero calls go to the planes as global atomic ors (other lines of the same 32-variant group set their bits in the
// same dwords).
// Round 3, after config 4 spent 3.8 of 16 ms here (88 k `GT:DP` lines at 115 GB/s): the first version dealt the BYTES
// to the lanes and let every lane loop over the columns that start in its 16 (two or three half-empty iterations per
// piece); this one runs 3.6 ms, of which 2.8 without any global atomic (~500 instructions per KiB and wave).  Collecting a
// line's calls in an LDS image (four ballots per round, merged by three lanes) and sending them to the planes at the end of
// the line was built and measured: 4.3 ms — a burst of sparse device-scope atomics hides worse than a trickle (in git
// history: round 3).
template <bool PLANES>
__global__ __launch_bounds__(256) void k_encode_general(const uint8_t *__restrict__ text, uint64_t n, const uint32_t *__restrict__ k_soff,
                                                        const uint32_t *__restrict__ k_lend, const uint32_t *__restrict__ k_meta,
                                                        const uint32_t *__restrict__ redo_list, const uint64_t *__restrict__ d_cursor,
                                                        LayoutDev lay, int8_t *__restrict__ G, uint8_t *__restrict__ P, DevCounters *cnt)
{
    const uint64_t v_base = *d_cursor;
    const PlanesGeom pgeom = planes_geom(lay, 0u);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * 4u;
    const uint32_t n_redo = (uint32_t)cnt->n_general;
    const uint32_t S = lay.S;
    __shared__ __attribute__((aligned(16))) uint8_t sbuf[4][1024 + GEN_HALO];   // the piece (plus a halo), per wave
    __shared__ uint16_t slist[4][1024];                                          // where its columns start
    const uint32_t wq = threadIdx.x >> 6;
    lds_u8 *piece = (lds_u8 *)sbuf[wq];
    lds_u16 *list = (lds_u16 *)slist[wq];
    uint32_t haploid = 0, malformed = 0, n_other = 0;
    for (uint32_t idx = wave; idx < n_redo; idx += n_waves) {
        const uint32_t k = redo_list[idx];
        const uint32_t soff = k_soff[k], lend = k_lend[k], gtidx = (k_meta[k] >> 8) & 0xFFFu;
        const TilePlace at = tile_place(lay, v_base, 0xFFFFFFFFu, 1u, k);   // the line's column: v_base + k
        if (!at.live) continue;
        const PlaneLine pline = PLANES ? plane_line(pgeom, at, P) : PlaneLine{nullptr, 0ull, 0u};
        const uint32_t rs = soff - 1u;  // the 9th tab: every sample field is preceded by a tab in [rs, lend)
        uint32_t tabs_before = 0, nl_inside = 0;
        // software pipeline: the piece in `cur` / `hal` was loaded one iteration ago
        uint4 cur = load16_or(text, n, (uint64_t)rs + 16u * lane, 0u);
        uint4 hal = lane < GEN_HALO / 16u ? load16_or(text, n, (uint64_t)rs + 1024u + 16u * lane, 0u) : make_uint4(0u, 0u, 0u, 0u);
        for (uint32_t base = rs; base < lend; base += 1024u) {
            const uint32_t b0 = base + 16u * lane;
            const bool more = base + 1024u < lend;   // (wave-uniform)
            uint4 nx = make_uint4(0u, 0u, 0u, 0u), nh = nx;
            if (more) {
                nx = load16_or(text, n, (uint64_t)b0 + 1024u, 0u);
                if (lane < GEN_HALO / 16u) nh = load16_or(text, n, (uint64_t)base + 2048u + 16u * lane, 0u);
            }
            stage_piece(piece, cur, hal, lane);
            const uint32_t m = tab_and_newline_masks(cur, b0, lend, &nl_inside);
            const PieceReader rd = {piece, text, base, lend - base < 1024u + GEN_HALO ? lend - base : 1024u + GEN_HALO};
            const uint32_t nf = list_columns(list, m, lane);
            gen_fence();
            for (uint32_t r0 = 0; r0 < nf; r0 += 64u) {   // (wave-uniform trip count)
                const uint32_t i = r0 + lane;
                const uint32_t s = tabs_before + i;
                const bool act = i < nf && s < S;   // surplus columns are not decoded (the oracle ignores them too)
                const uint32_t o0 = (uint32_t)list[i < 1024u ? i : 1023u];
                uint32_t p = base + (act ? o0 : 1u);
                const bool missing = gtidx != 0u && act && !skip_to_gt(rd, p, lend, gtidx);
                uint32_t na = 2u, hv;
                const bool done = common_column(rd, p, lend, &hv) & !missing;
                if (!done) hv = 0xF7F7u;
                if (__builtin_amdgcn_ballot_w64(act && !done && !missing) != 0ull) {   // (wave-uniform: some lane needs the byte walk)
                    if (act && !done && !missing) {
                        na = 1u;
                        // the sub-field ends at ':' or at the column's tab; both stop the GT rule
                        hv = parse_gt_bytes(rd, p, lend, &na);
                    }
                }
                if (act && missing) na = 1u;   // a column without the GT sub-field counts as one missing allele (parse_gt_bytes of nothing)
                if (act && na == 1u) ++haploid;
                if (!PLANES) {
                    if (act) *reinterpret_cast<uint16_t *>(G + matrix_at(lay, at.vcol, s, at.vin)) = (uint16_t)hv;
                } else
                    emit_planes(pline, lay, at, act, s, hv, G, &n_other);
            }
            tabs_before += nf;
            cur = nx;
            hal = nh;
            gen_fence();
        }
        // fewer sample columns than the header declares; or a line end inside the line: a line shorter than any record
        // with S samples can be (its newline lay in the part the hopping index does not look at, index.hip)
        const bool broken = __builtin_amdgcn_ballot_w64(nl_inside != 0u) != 0ull;
        if ((tabs_before < S || broken) && lane == 0) ++malformed;
    }
    wave_totals(cnt, haploid, malformed, n_other, lane);
}

// -------------------------------------------------------------------------------------------------
// zero bytes [b0, b1) of a sample row of the int8 matrix in 16-byte segments, the workgroups of grid.x side by side
__device__ __forceinline__ void zero_row_bytes(int8_t *row, uint64_t b0, uint64_t b1)
{
    const uint64_t seg0 = b0 / 16ull, seg1 = (b1 + 15ull) / 16ull;
    for (uint64_t sgm = seg0 + blockIdx.x * blockDim.x + threadIdx.x; sgm < seg1; sgm += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t lo = sgm * 16ull, hi = lo + 16ull;
        if (lo >= b0 && hi <= b1)
            *reinterpret_cast<uint4 *>(row + lo) = make_uint4(0, 0, 0, 0);
        else
            for (uint64_t b = lo < b0 ? b0 : lo; b < (hi > b1 ? b1 : hi); ++b) row[b] = 0;
    }
}

// zero columns [c0, c1) (variant index inside the chunk column) of rows [r0, r1) (sample index inside
// the padded sample axis) of chunk column vcol
__global__ __launch_bounds__(256) void k_zero_rect(LayoutDev lay, uint64_t vcol0, uint32_t r0, uint32_t r1, uint64_t c0, uint64_t c1, int8_t *__restrict__ G)
{
    const uint64_t vcol = vcol0 + blockIdx.z;   // one launch covers a range of chunk columns
    const uint32_t r = r0 + blockIdx.y;
    if (r >= r1) return;
    zero_row_bytes(G + matrix_row(lay, vcol, r), c0 * 2ull, c1 * 2ull);
}

// cursor form of the tail padding: the kept count lives in device memory (asynchronous chains)
__global__ __launch_bounds__(256) void k_zero_tail_cursor(LayoutDev lay, const uint64_t *__restrict__ d_cursor, int8_t *__restrict__ G)
{
    uint64_t vcol, c0;
    column_of(lay, *d_cursor, &vcol, &c0);
    if (c0 == 0) return;                       // the cursor sits on a column boundary: nothing is open
    const uint32_t r = blockIdx.y;             // padded sample row
    zero_row_bytes(G + matrix_row(lay, vcol, r), r < lay.S ? c0 * 2ull : 0ull, lay.Vc * 2ull);   // sample padding rows: the whole row
}

int launch_pad_tail_cursor(LayoutDev lay, const uint64_t *d_cursor, int8_t *d_G, hipStream_t st)
{
    const uint32_t S_pad = lay.n_sc * lay.Sc;
    if (S_pad == 0) return HHGT_OK;
    uint64_t segs = (lay.Vc * 2 + 15) / 16 + 1;
    uint32_t gx = (uint32_t)((segs + 255) / 256);
    if (gx > 8) gx = 8;
    hipLaunchKernelGGL(k_zero_tail_cursor, dim3(gx, S_pad), dim3(256), 0, st, lay, d_cursor, d_G);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

// -------------------------------------------------------------------------------------------------
int launch_encode_tiles(const uint8_t *d_text, uint64_t n, const uint32_t *k_soff, const uint32_t *k_meta,
                        uint32_t n_lines_bound, const uint64_t *d_cursor, LayoutDev lay, int8_t *d_G,
                        uint32_t *redo_list, uint32_t *redo_flag, DevCounters *d_cnt, hipStream_t st)
{
    if (n_lines_bound == 0 || lay.S == 0) return HHGT_OK;
    const uint32_t tiles_s = (lay.S + TILE_S - 1) / TILE_S;
    // the append position is only known on the device: one tile more than the lines need covers any phase
    const uint64_t tiles_v = (63 + (uint64_t)n_lines_bound + 63) / 64;
    hipLaunchKernelGGL(k_encode_tiles, dim3((uint32_t)tiles_v, tiles_s), dim3(256), 0, st, d_text, n, k_soff, k_meta, d_cursor, lay,
                       d_G, redo_list, redo_flag, d_cnt);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

int launch_encode_general(const uint8_t *d_text, uint64_t n, const uint32_t *k_soff, const uint32_t *k_lend,
                          const uint32_t *k_meta, const uint32_t *redo_list, const uint64_t *d_cursor, LayoutDev lay,
                          int8_t *d_G, uint8_t *d_P, DevCounters *d_cnt, int n_cu, hipStream_t st)
{
    if (lay.S == 0) return HHGT_OK;
    if (d_P)
        hipLaunchKernelGGL(k_encode_general<true>, dim3((uint32_t)n_cu * 8u), dim3(256), 0, st, d_text, n, k_soff, k_lend,
                           k_meta, redo_list, d_cursor, lay, d_G, d_P, d_cnt);
    else
        hipLaunchKernelGGL(k_encode_general<false>, dim3((uint32_t)n_cu * 8u), dim3(256), 0, st, d_text, n, k_soff, k_lend,
                           k_meta, redo_list, d_cursor, lay, d_G, d_P, d_cnt);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

int launch_encode_planes(const uint8_t *d_text, uint64_t n, const uint32_t *k_soff, const uint32_t *k_meta,
                         uint32_t n_lines_bound, const uint64_t *d_cursor, LayoutDev lay, uint8_t *d_P, int8_t *d_G,
                         uint32_t *redo_list, uint32_t *redo_flag, DevCounters *d_cnt, hipStream_t st)
{
    if (n_lines_bound == 0 || lay.S == 0) return HHGT_OK;
    const uint32_t tiles_s = (lay.S + PT_S - 1) / PT_S;
    // the append position is only known on the device: one tile more than the lines need covers any phase
    const uint64_t tiles_v = ((uint64_t)(PT_V - 1) + (uint64_t)n_lines_bound + (PT_V - 1)) / PT_V;
    // (measured, encode stage of the bench: 7.6 ms variant tile fastest, 7.4 ms band fastest / XCD-aware)
    // the XCD-aware order deals variant tiles out in groups of 8: the grid is rounded up to whole groups
    const uint64_t n_wg = (tiles_v + 7ull) / 8ull * 8ull * tiles_s;
    hipLaunchKernelGGL(k_encode_planes, dim3((uint32_t)n_wg), dim3(64 * PT_NW), 0, st, d_text, n, k_soff, k_meta, d_cursor, lay,
                       d_P, d_G, redo_list, redo_flag, d_cnt, (uint32_t)tiles_v, tiles_s);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

// -------------------------------------------------------------------------------------------------
// planes: zero the bits of variants [c0, Vc) of padded sample rows [r0, r1) of chunk columns vcol0 + blockIdx.z
// (tile-major planes: per tile and kind-plane the rows' 32-byte pieces are contiguous).  grid.x walks the tiles of the
// column, grid.y groups of 32 rows; a thread owns one dword of one row's piece, for the four kind-planes.
__device__ __forceinline__ void zero_planes_rows(const LayoutDev &lay, uint64_t vcol, uint32_t r0, uint32_t r1, uint64_t c0, uint32_t S,
                                                 uint8_t *__restrict__ P)
{
    const PlanesGeom pg = planes_geom(lay, 0u);
    const uint32_t r = r0 + blockIdx.y * 32u + (threadIdx.x >> 3), dw = threadIdx.x & 7u;
    if (r >= r1) return;
    const uint64_t from = r < S ? c0 : 0ull;   // sample padding rows: the whole row
    for (uint32_t t = blockIdx.x; t < pg.tpc; t += gridDim.x) {
        const uint64_t lo = (uint64_t)t * PL_TILE + 32ull * dw;   // first variant of this thread's dword
        if (lo + 32ull <= from) continue;
        const uint32_t keep = lo >= from ? 0u : ((1u << (uint32_t)(from - lo)) - 1u);
#pragma unroll
        for (uint32_t kp = 0; kp < 4u; ++kp) {
            uint32_t *p = reinterpret_cast<uint32_t *>(P + planes_piece(pg, vcol, t, kp, r)) + dw;
            *p = keep ? (*p & keep) : 0u;
        }
    }
}

__global__ __launch_bounds__(256) void k_zero_planes_rect(LayoutDev lay, uint64_t vcol0, uint32_t r0, uint32_t r1, uint64_t c0,
                                                          uint8_t *__restrict__ P)
{
    zero_planes_rows(lay, vcol0 + blockIdx.z, r0, r1, c0, 0xFFFFFFFFu, P);
}

__global__ __launch_bounds__(256) void k_zero_planes_cursor(LayoutDev lay, const uint64_t *__restrict__ d_cursor, uint8_t *__restrict__ P)
{
    uint64_t vcol, c0;
    column_of(lay, *d_cursor, &vcol, &c0);
    if (c0 == 0) return;                       // the cursor sits on a column boundary: nothing is open
    zero_planes_rows(lay, vcol, 0u, lay.n_sc * lay.Sc, c0, lay.S, P);
}

int launch_pad_tail_planes_cursor(LayoutDev lay, const uint64_t *d_cursor, uint8_t *d_P, hipStream_t st)
{
    const uint32_t S_pad = lay.n_sc * lay.Sc;
    if (S_pad == 0) return HHGT_OK;
    const uint32_t tpc = (uint32_t)(lay.Vc / PL_TILE);
    hipLaunchKernelGGL(k_zero_planes_cursor, dim3(tpc < 32 ? tpc : 32, (S_pad + 31) / 32), dim3(256), 0, st, lay, d_cursor, d_P);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

int launch_pad_tail_planes(LayoutDev lay, uint64_t v_end, uint64_t vcol_begin, uint64_t vcol_end, uint8_t *d_P, hipStream_t st)
{
    const uint32_t S_pad = lay.n_sc * lay.Sc;
    const uint32_t tpc = (uint32_t)(lay.Vc / PL_TILE);
    const uint32_t gx = tpc < 32 ? tpc : 32;
    if (v_end % lay.Vc) {   // (a) variant padding of the last touched chunk column
        const uint64_t vcol = v_end / lay.Vc;
        if (vcol < vcol_end && vcol >= vcol_begin && S_pad)
            hipLaunchKernelGGL(k_zero_planes_rect, dim3(gx, (S_pad + 31) / 32), dim3(256), 0, st, lay, vcol, 0u, S_pad, v_end - vcol * lay.Vc, d_P);
    }
    if (S_pad > lay.S) {    // (b) sample padding rows of every touched chunk column
        for (uint64_t v0 = vcol_begin; v0 < vcol_end; v0 += 65535) {
            const uint32_t nz = (uint32_t)(vcol_end - v0 < 65535 ? vcol_end - v0 : 65535);
            hipLaunchKernelGGL(k_zero_planes_rect, dim3(gx, (S_pad - lay.S + 31) / 32, nz), dim3(256), 0, st, lay, v0, lay.S, S_pad, 0ull, d_P);
        }
    }
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

// -------------------------------------------------------------------------------------------------
// planes -> int8 bytes (the inverse of the packing; for consumers that want the matrix after all and for the parity
// tests).  One workgroup per Blosc block (one sample row x 4096 variants = 16 tiles), thread t owns variants
// [16 t, 16 t + 16): 2 bytes of each kind-plane piece of tile t / 16.
__global__ __launch_bounds__(256) void k_planes_expand(LayoutDev lay, PlanesGeom pg, const uint8_t *__restrict__ P, const uint8_t *G,
                                                       uint8_t *out, uint64_t id0)   // out may be G
{
    uint64_t col;
    uint32_t row, bi;
    planes_block(pg, id0 + blockIdx.x, &col, &row, &bi);
    const uint32_t t = threadIdx.x;
    const uint32_t tile = bi * 16u + (t >> 4), sub = t & 15u;   // 16-bit word `sub` of the tile's 32-byte piece
    const uint64_t kstride = (uint64_t)pg.S_pad * 16ull;        // 16-bit words between kind-planes
    const uint16_t *pl = reinterpret_cast<const uint16_t *>(P + planes_piece(pg, col, tile, 0u, row)) + sub;
    const uint32_t o0 = pl[0], o1 = pl[kstride], e0 = pl[2ull * kstride], e1 = pl[3ull * kstride];
    const uint64_t base = matrix_at(lay, col, row, (uint64_t)bi * 4096ull + 16ull * t);   // this thread's 16 variants of the block
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint32_t x = 0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int j = 2 * i + k;
            uint32_t h0 = (o0 >> j) & 1u, h1 = (o1 >> j) & 1u;
            if ((e0 >> j) & 1u) h0 = h0 ? 0xF7u : (G ? (uint32_t)G[base + 2u * j] : 0u);
            if ((e1 >> j) & 1u) h1 = h1 ? 0xF7u : (G ? (uint32_t)G[base + 2u * j + 1u] : 0u);
            x |= (h0 | (h1 << 8)) << (16 * k);
        }
        w[i] = x;
    }
    uint4 *dst = reinterpret_cast<uint4 *>(out + base);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

int launch_planes_expand(LayoutDev lay, const uint8_t *d_P, const uint8_t *d_G, uint32_t col0, uint32_t n_cols, uint8_t *d_out, hipStream_t st)
{
    const PlanesGeom pg = planes_geom(lay, col0);
    const uint64_t n_blocks = (uint64_t)n_cols * pg.S_pad * pg.bpr;
    for (uint64_t b0 = 0; b0 < n_blocks; b0 += 0x40000000ull) {
        const uint64_t nb = n_blocks - b0 < 0x40000000ull ? n_blocks - b0 : 0x40000000ull;
        hipLaunchKernelGGL(k_planes_expand, dim3((uint32_t)nb), dim3(256), 0, st, lay, pg, d_P, d_G, d_out, b0);
    }
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
int launch_pad_tail(LayoutDev lay, uint64_t v_end, uint64_t vcol_begin, uint64_t vcol_end, int8_t *d_G,
                    hipStream_t st)
{
    const uint32_t S_pad = lay.n_sc * lay.Sc;
    // (a) variant padding of the last touched chunk column
    if (v_end % lay.Vc) {
        uint64_t vcol = v_end / lay.Vc;
        uint64_t c0 = v_end - vcol * lay.Vc, c1 = lay.Vc;
        if (vcol < vcol_end && vcol >= vcol_begin && S_pad) {
            uint64_t segs = ((c1 - c0) * 2 + 15) / 16 + 1;
            uint32_t gx = (uint32_t)((segs + 255) / 256);
            if (gx > 1024) gx = 1024;
            hipLaunchKernelGGL(k_zero_rect, dim3(gx, S_pad), dim3(256), 0, st, lay, vcol, 0u, S_pad, c0, c1, d_G);
        }
    }
    // (b) sample padding rows of every touched chunk column
    if (S_pad > lay.S) {
        uint64_t segs = (lay.Vc * 2 + 15) / 16 + 1;
        uint32_t gx = (uint32_t)((segs + 255) / 256);
        if (gx > 64) gx = 64;
        for (uint64_t v0 = vcol_begin; v0 < vcol_end; v0 += 65535) {
            uint32_t nz = (uint32_t)(vcol_end - v0 < 65535 ? vcol_end - v0 : 65535);
            hipLaunchKernelGGL(k_zero_rect, dim3(gx, S_pad - lay.S, nz), dim3(256), 0, st, lay, v0, lay.S, S_pad, 0ull,
                               lay.Vc, d_G);
        }
    }
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
