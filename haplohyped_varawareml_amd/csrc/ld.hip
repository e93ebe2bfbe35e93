// Linkage disequilibrium between nearby variants from genotype bit planes: hhgt_variant_planes turns hhgt_genotype_planes'
// sample-major rows (32 variants per word) into variant-major rows (32 samples per word), hhgt_ld_counts reduces every pair
// of rows at most `window` apart to eight popcounts, hhgt_ld_prune decides r^2 > t per pair from those integers and walks the
// variants greedily; hhgt_ld_decisions makes the same decisions, with a distance cut, for the clumping of clump.hip.
// include/hhgt.h has the contract.
#include "common.h"
#include "plane_tiles.h"

// ---- hhgt_variant_planes: the bit transposition ------------------------------------------------------------------------

static constexpr uint32_t TR_ROWS = 256;    // plane rows per workgroup: 64 per wave, 8 output words per bit position
static constexpr uint32_t TR_WORDS = 8;     // plane words per row and workgroup: 32-byte pieces of a row, 256 bit positions

// grid = (ceil(words / 8), ceil(n_rows / 256)), 256 threads.  The tile's 256 rows x 8 words of the three planes go to LDS with
// consecutive lanes on consecutive words of a row (row stride 9 words: the column reads below touch 32 banks); then lane =
// row: per word and plane a wave holds 64 rows' words, bit c of all of them is one v_cmp (a 64-bit row mask in an SGPR
// pair), lane c keeps mask c, and after the 32 bits lanes 0..31 store their mask as words 2 rb, 2 rb + 1 of output row
// 32 word + c (rb: the wave's block of 64 rows).  Rows >= n_rows are staged as zeros, words >= sw are not stored: every
// output word [3][32 (w_hi - w_lo)][sw] is written once, by plain stores.
__global__ __launch_bounds__(256) void k_variant_planes(const uint32_t *__restrict__ planes, uint32_t n_rows,
                                                        uint32_t row_words, uint32_t w_lo, uint32_t w_hi, uint32_t sw,
                                                        uint32_t *__restrict__ vplanes)
{
    __shared__ uint32_t s_in[3u * TR_ROWS * (TR_WORDS + 1u)];   // 27 KiB
    const uint32_t w0 = w_lo + blockIdx.x * TR_WORDS, row0 = blockIdx.y * TR_ROWS;
    const uint64_t plane_words = (uint64_t)n_rows * row_words;
    const uint64_t out_plane = (uint64_t)(w_hi - w_lo) * 32u * sw;
#pragma unroll
    for (uint32_t q = 0; q < TR_ROWS * TR_WORDS / 256u; ++q) {
        const uint32_t item = threadIdx.x + 256u * q, k = item & (TR_WORDS - 1u), r = item / TR_WORDS;
        uint32_t h = 0u, ref = 0u, alt = 0u;
        if (row0 + r < n_rows && w0 + k < w_hi) {
            const uint32_t *p = planes + (uint64_t)(row0 + r) * row_words + w0 + k;
            h = p[0];
            ref = p[plane_words];
            alt = p[2u * plane_words];
        }
        const uint32_t at = r * (TR_WORDS + 1u) + k;
        s_in[at] = h;
        s_in[TR_ROWS * (TR_WORDS + 1u) + at] = h | ref | alt;
        s_in[2u * TR_ROWS * (TR_WORDS + 1u) + at] = alt;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t s0 = (row0 + wave * 64u) / 32u;              // first output word of this wave's 64 rows
    if (s0 >= sw) return;
    for (uint32_t k = 0; k < TR_WORDS && w0 + k < w_hi; ++k) {
#pragma unroll
        for (uint32_t pl = 0; pl < 3u; ++pl) {
            const uint32_t x = s_in[pl * TR_ROWS * (TR_WORDS + 1u) + (wave * 64u + lane) * (TR_WORDS + 1u) + k];
            uint64_t mine = 0ull;
#pragma unroll 8
            for (uint32_t c = 0; c < 32u; ++c) {
                const uint64_t m = __ballot((x >> c) & 1u);
                if (lane == c) mine = m;
            }
            if (lane < 32u) {
                uint32_t *o = vplanes + pl * out_plane + ((uint64_t)(w0 + k - w_lo) * 32u + lane) * sw + s0;
                o[0] = (uint32_t)mine;
                if (s0 + 1u < sw) o[1] = (uint32_t)(mine >> 32);
            }
        }
    }
}

int launch_variant_planes(const uint32_t *d_planes, uint32_t n_rows, uint64_t row_words, uint64_t w_lo, uint64_t w_hi,
                          uint32_t *d_vplanes, hipStream_t st)
{
    if (n_rows == 0 || w_lo >= w_hi) return HHGT_OK;
    const uint64_t gx = (w_hi - w_lo + TR_WORDS - 1u) / TR_WORDS;
    const uint32_t gy = (n_rows + TR_ROWS - 1u) / TR_ROWS;
    if (gx > 0x7fffffffull || gy > 65535u || row_words > 0xfffffff0ull) {
        hhgt_set_error("variant_planes: %u rows, words [%llu, %llu) of %llu (at most %u rows, 2^31 - 1 tiles of %u words)",
                       n_rows, (unsigned long long)w_lo, (unsigned long long)w_hi, (unsigned long long)row_words,
                       65535u * TR_ROWS, TR_WORDS);
        return HHGT_ERR_ARG;
    }
    hipLaunchKernelGGL(k_variant_planes, dim3((uint32_t)gx, gy), dim3(256), 0, st, d_planes, n_rows, (uint32_t)row_words,
                       (uint32_t)w_lo, (uint32_t)w_hi, (n_rows + 31u) / 32u, d_vplanes);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

// ---- hhgt_ld_counts: the band of pairs -----------------------------------------------------------------------------------

static constexpr uint32_t TILE = 32;     // variants per tile side: a workgroup owns the pairs (i, j) of 32 i-rows x 32 j-rows
static constexpr uint32_t SLICE = 16;    // sample words per row staged at a time: 64 bytes of each row and plane

// grid = (T, 1 + ceil(window / 32)) for T = ceil(n_var / 32): workgroup (ti, b) holds the i-rows of tile ti and the j-rows of
// tile ti + b, and owns the entries (k, d) = (i, j - i - 1) with 1 <= j - i <= window of them: a pair lies in one i-tile and
// one j-tile, at most ceil(window / 32) tiles on, so every entry of the table has exactly one owner.  256 threads as 16 x 16: thread
// (ty, tx) keeps the pairs (32 ti + ty + 16 a, 32 (ti + b) + tx + 16 c), a, c = 0, 1, eight counters each: 32 counters,
// 4 workgroups of 4 waves per compute unit on 17 KiB of LDS each.  The tile is 32 and not pairs.hip's 64 because the band
// is narrow: at window 50 a 32-tile computes 96 pairs per variant for 50 wanted, a 64-tile 128, and a 64-tile's 128
// counters per thread would leave two waves per SIMD.  Per slice of 16 sample words the 32 + 32 rows go to LDS as one uint4
// (HET, COMPLETE, HOM_ALT, 0) per row and word; per word a thread reads its 2 i-rows and 2 j-rows (4 ds_read_b128: 16
// consecutive slots on the j side, one slot per 16 lanes on the i side) and does 17 VALU operations per pair.  Rows >= n_var
// and words >= sw are staged as zeros.  At the end each thread adds its counters to its entries: plain read-modify-write.
__global__ __launch_bounds__(256, 4) void k_ld_counts(const uint32_t *__restrict__ vplanes, uint32_t n_var, uint32_t sw,
                                                      uint32_t window, uint4 *__restrict__ table)
{
    __shared__ u32x4 s_slice[2u * SLICE * (TILE + 1u)];   // 16.5 KiB
    const uint32_t i0 = blockIdx.x * TILE;
    const uint64_t j0 = (uint64_t)i0 + (uint64_t)blockIdx.y * TILE;
    if (j0 >= n_var) return;
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint64_t plane_words = (uint64_t)n_var * sw;
    uint32_t cnt[2][2][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) cnt[a][c][e] = 0u;
    for (uint32_t w0 = 0; w0 < sw; w0 += SLICE) {
        stage_slice<TILE, SLICE, 2u * TILE * SLICE / 256u>(s_slice, vplanes, sw, plane_words, (uint64_t)i0, j0, n_var, w0, sw - w0,
                                                           [](uint32_t het, uint32_t m, uint32_t alt) { return u32x4{het, m, alt, 0u}; });
#pragma unroll 4
        for (uint32_t w = 0; w < SLICE; ++w) {
            u32x4 I[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) I[a] = s_slice[tile_slot<TILE, SLICE>(0u, w, ty + 16u * (uint32_t)a)];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const u32x4 J = s_slice[tile_slot<TILE, SLICE>(1u, w, tx + 16u * (uint32_t)c)];
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    uint32_t *t = cnt[a][c];
                    bcnt_acc(t[0], I[a].y & J.y);                              // N:  Mu Mv
                    bcnt_acc(t[1], I[a].x & J.y);                              // HM: Hu Mv
                    bcnt_acc(t[2], I[a].z & J.y);                              // AM: Au Mv
                    bcnt_acc(t[3], I[a].y & J.x);                              // MH: Mu Hv
                    bcnt_acc(t[4], I[a].y & J.z);                              // MA: Mu Av
                    bcnt_acc(t[5], I[a].x & J.x);                              // HH: Hu Hv
                    bcnt_acc(t[6], (I[a].x & J.z) | (I[a].z & J.x));           // HA: Hu Av or Au Hv
                    bcnt_acc(t[7], I[a].z & J.z);                              // AA: Au Av
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const uint64_t i = (uint64_t)i0 + ty + 16u * (uint32_t)a;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint64_t j = j0 + tx + 16u * (uint32_t)c;
            if (j >= n_var || j <= i || j - i > window) continue;
            uint4 *e = table + (i * window + (j - i - 1u)) * 2u;
            const uint32_t *t = cnt[a][c];
            uint4 lo = e[0], hi = e[1];
            lo.x += t[0], lo.y += t[1], lo.z += t[2], lo.w += t[3];
            hi.x += t[4], hi.y += t[5], hi.z += t[6], hi.w += t[7];
            e[0] = lo;
            e[1] = hi;
        }
    }
}

int launch_ld_counts(const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, uint32_t window, uint32_t *d_table,
                     hipStream_t st)
{
    if (n_var < 2 || sw == 0) return HHGT_OK;
    const uint64_t tiles = (n_var + TILE - 1u) / TILE;
    if (n_var > 0xffffff00ull || sw > 0xfffffff0ull) {
        hhgt_set_error("ld_counts: %llu variants of %llu words (at most 2^32 - 256 variants, 2^32 - 16 words)",
                       (unsigned long long)n_var, (unsigned long long)sw);
        return HHGT_ERR_ARG;
    }
    hipLaunchKernelGGL(k_ld_counts, dim3((uint32_t)tiles, 1u + (window + TILE - 1u) / TILE), dim3(256), 0, st, d_vplanes,
                       (uint32_t)n_var, (uint32_t)sw, window, reinterpret_cast<uint4 *>(d_table));
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

// ---- hhgt_ld_prune: the decisions, then the walk -------------------------------------------------------------------------

// exceeds(u, v, t) of one table entry, as include/hhgt.h states it: int64 sums, three float64 products, each rounded once
// (there is no addition, so nothing contracts into an fma).  A pair with dx dy = 0 has num = 0 (Cauchy-Schwarz): 0 > 0.
__device__ __forceinline__ bool ld_exceeds(uint4 lo, uint4 hi, double t)
{
    const int64_t n = lo.x, hm = lo.y, am = lo.z, mh = lo.w, ma = hi.x, hh = hi.y, ha = hi.z, aa = hi.w;
    const int64_t sx = hm + 2 * am, sxx = hm + 4 * am, sy = mh + 2 * ma, syy = mh + 4 * ma, sxy = hh + 2 * ha + 4 * aa;
    const double num = (double)(n * sxy - sx * sy), dx = (double)(n * sxx - sx * sx), dy = (double)(n * syy - sy * sy);
    const double nn = num * num, den = dx * dy;
    return nn > t * den;
}

// one wave per (variant v of the tile, 64 window slots): lane l decides the pair (u, v) = (v - 1 - d, v), d = 64 q + l, from
// table row window + u, entry d (row r of the table is the variant window places before variant r of the tile: the first
// `window` rows are the carried ones), and the wave's ballot is word q of bits[v]: bit d set = u prunes v if u is kept
__global__ __launch_bounds__(256) void k_ld_exceeds(const uint4 *__restrict__ table, uint32_t n_var, uint32_t window,
                                                    uint32_t nq, double t, uint64_t *__restrict__ bits)
{
    const uint64_t unit = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (unit >= (uint64_t)n_var * nq) return;
    const uint32_t v = (uint32_t)(unit / nq), q = (uint32_t)(unit % nq), d = q * 64u + (threadIdx.x & 63u);
    bool x = false;
    if (d < window) {
        const uint4 *e = table + (((uint64_t)window + v - 1u - d) * window + d) * 2u;
        x = ld_exceeds(e[0], e[1], t);
    }
    const uint64_t m = __ballot(x);
    if ((threadIdx.x & 63u) == 0u) bits[unit] = m;
}

// hhgt_ld_decisions: k_ld_exceeds with a distance cut and the public layout of include/hhgt.h — nq = ceil(window / 64) words
// per variant, not the walk's power of two.  pos (NULL: no limit) is laid out like the table's rows: pos[window + v] is
// variant v of the tile.  The difference of two int64 is taken in uint64, where it cannot overflow.
__global__ __launch_bounds__(256) void k_ld_decisions(const uint4 *__restrict__ table, uint32_t n_var, uint32_t window,
                                                      uint32_t nq, double t, const int64_t *__restrict__ pos,
                                                      uint64_t max_dist, uint64_t *__restrict__ bits)
{
    const uint64_t unit = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (unit >= (uint64_t)n_var * nq) return;
    const uint32_t v = (uint32_t)(unit / nq), q = (uint32_t)(unit % nq), d = q * 64u + (threadIdx.x & 63u);
    bool x = false;
    if (d < window) {
        const uint64_t u = (uint64_t)window + v - 1u - d;
        const uint4 *e = table + (u * window + d) * 2u;
        x = ld_exceeds(e[0], e[1], t);
        if (x && pos) {
            const int64_t a = pos[(uint64_t)window + v], b = pos[u];
            x = (a >= b ? (uint64_t)a - (uint64_t)b : (uint64_t)b - (uint64_t)a) <= max_dist;
        }
    }
    const uint64_t m = __ballot(x);
    if ((threadIdx.x & 63u) == 0u) bits[unit] = m;
}

int launch_ld_decisions(const uint32_t *d_table, uint64_t n_var, uint32_t window, double r2, const int64_t *d_pos, int64_t max_dist,
                        uint64_t *d_bits, hipStream_t st)
{
    if (n_var == 0) return HHGT_OK;
    const uint32_t nq = (window + 63u) / 64u;
    const uint64_t blocks = (n_var * nq + 3u) / 4u;
    if (n_var > 0x7fffffffull || blocks > 0x7fffffffull) {
        hhgt_set_error("ld_decisions: %llu variants at window %u (at most 2^31 - 1 variants, 2^33 decision words)",
                       (unsigned long long)n_var, window);
        return HHGT_ERR_ARG;
    }
    hipLaunchKernelGGL(k_ld_decisions, dim3((uint32_t)blocks), dim3(256), 0, st, reinterpret_cast<const uint4 *>(d_table),
                       (uint32_t)n_var, window, nq, r2, d_pos, (uint64_t)max_dist, d_bits);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

// one wave.  K[q] bit l = the keep flag of the variant 64 q + l + 1 places before the current one: a shift register of
// `window` bits in NQ 64-bit words that every lane holds alike (wave-uniform, so scalar registers).  Per round of 64 variants
// lane l loads the NQ decision words of variant v0 + l; then the variants go one by one: the words of variant v0 + j are read
// from lane j, it is kept iff none of its set bits meets a set bit of K, and K shifts its flag in.  The round's flags leave as
// one byte per lane.
template <int NQ>
__global__ __launch_bounds__(64) void k_ld_walk(const uint64_t *__restrict__ bits, uint32_t n_var, uint32_t window,
                                                uint8_t *__restrict__ keep)
{
    const uint32_t lane = threadIdx.x;
    uint64_t K[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const uint32_t d = (uint32_t)q * 64u + lane;
        K[q] = __ballot(d < window && keep[window - 1u - d] != 0);
    }
    for (uint32_t v0 = 0; v0 < n_var; v0 += 64u) {
        uint64_t E[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) E[q] = v0 + lane < n_var ? bits[(uint64_t)(v0 + lane) * NQ + q] : 0ull;
        uint64_t kept = 0ull;
        const uint32_t n = min(64u, n_var - v0);
        for (uint32_t j = 0; j < n; ++j) {
            uint64_t hit = 0ull;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)E[q], (int)j);
                const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(E[q] >> 32), (int)j);
                hit |= (((uint64_t)hi << 32) | lo) & K[q];
            }
            const uint64_t k = hit == 0ull ? 1ull : 0ull;
            kept |= k << j;
#pragma unroll
            for (int q = NQ - 1; q > 0; --q) K[q] = (K[q] << 1) | (K[q - 1] >> 63);
            K[0] = (K[0] << 1) | k;
        }
        if (lane < n) keep[(uint64_t)window + v0 + lane] = (uint8_t)((kept >> lane) & 1ull);
    }
}

// 64-bit words of the walk's shift register, and of a variant's decision bits: a power of two with 64 nq >= window, 1 .. 16.
// The one place that says so: the scratch size, the decisions' layout and the walk's instantiation all take it from here.
uint32_t ld_walk_words(uint32_t window)
{
    uint32_t nq = 1;
    while (nq * 64u < window) nq *= 2u;
    return nq;
}

int launch_ld_exceeds(const uint32_t *d_table, uint64_t n_var, uint32_t window, double r2, uint64_t *d_bits, hipStream_t st)
{
    if (n_var == 0) return HHGT_OK;
    const uint32_t nq = ld_walk_words(window);
    const uint64_t blocks = (n_var * nq + 3u) / 4u;
    if (n_var > 0x7fffffffull || blocks > 0x7fffffffull) {
        hhgt_set_error("ld_prune: %llu variants at window %u (at most 2^31 - 1 variants, 2^33 decision words)",
                       (unsigned long long)n_var, window);
        return HHGT_ERR_ARG;
    }
    hipLaunchKernelGGL(k_ld_exceeds, dim3((uint32_t)blocks), dim3(256), 0, st, reinterpret_cast<const uint4 *>(d_table),
                       (uint32_t)n_var, window, nq, r2, d_bits);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

// (the register is indexed by constants only, so each width is its own instantiation: a runtime width would index it
// dynamically, out of registers)
int launch_ld_walk(const uint64_t *d_bits, uint64_t n_var, uint32_t window, uint8_t *d_keep, hipStream_t st)
{
    if (n_var == 0) return HHGT_OK;
    void (*walk)(const uint64_t *, uint32_t, uint32_t, uint8_t *) = nullptr;
    switch (ld_walk_words(window)) {
    case 1: walk = k_ld_walk<1>; break;
    case 2: walk = k_ld_walk<2>; break;
    case 4: walk = k_ld_walk<4>; break;
    case 8: walk = k_ld_walk<8>; break;
    default: walk = k_ld_walk<16>; break;
    }
    hipLaunchKernelGGL(walk, dim3(1), dim3(64), 0, st, d_bits, (uint32_t)n_var, window, d_keep);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
