// Quadratic forms of per-variant vectors in one dense symmetric matrix (hhgt_quad_forms): q[v] = x_v^T A x_v, the reduction
// behind the mixed-model association scan (x^T M x of every variant).  The planes are hhgt_variant_planes' — uint32
// [3][n_var][sw], 32 samples per word —, x_v(s) is a combination of the variant's three bits at s with three coefficients of
// its own, and A is double [32 sw][32 sw].  A (samples x samples) . (samples x variants) product on the f64 MFMA whose right
// factor is built in registers from bits, with the second factor applied in the epilogue: no samples x variants matrix is
// ever written.  include/hhgt.h has the contract.
#include "common.h"
#include "plane_tiles.h"

static constexpr uint32_t WAVES = 8;                     // waves per workgroup: 16 variants each
static constexpr uint32_t VARS = 16u * WAVES;            // variants per workgroup
static constexpr uint32_t BLOCK = 128;                   // plane rows of a row block: 8 accumulators a wave
static constexpr uint32_t TILES = BLOCK / 16u;
static constexpr uint32_t POS = 32;                      // positions staged at a time: one plane word
// doubles between two positions of a stage in LDS: 16 past the block, so that the two positions one ds_read_b64 pass reads
// (lanes 0..15 and 16..31: 128 bytes each) lie 1152 bytes apart — the two halves of the 64 banks
static constexpr uint32_t PITCH = BLOCK + 16u;
static constexpr uint32_t HALF = POS / 2u / WAVES;        // positions of half a stage that a wave fetches
static constexpr uint32_t STAGE = POS * PITCH;           // doubles of a stage: 36 KiB, two of them 72 KiB: two workgroups a CU

typedef double f64x2 __attribute__((ext_vector_type(2)));

// x at bit `bit` of the three words: (c0 HET + c1 COMPLETE) + c2 HOM_ALT, every product exact (a bit is 0.0 or 1.0), the two
// sums rounded once each, in that order
__device__ __forceinline__ double x_at(const double (&c)[3], uint32_t het, uint32_t complete, uint32_t alt, uint32_t bit)
{
    return __fma_rn(c[2], bit_as_f64(alt, bit), __fma_rn(c[1], bit_as_f64(complete, bit), c[0] * bit_as_f64(het, bit)));
}

// grid = ceil(n_var / 128); wave u owns the variants 128 g + 16 u + (0..15).  The rows of A go by in blocks of 128; for row
// block b the wave holds (A x)[128 b + (0..127)][its 16 variants] in eight accumulators: MFMA A side = a 16 x 4 piece of A
// from LDS, B side = x of (position 4 t + (l >> 4), variant l & 15) made from the lane's words.  A is symmetric, so block b
// takes only the positions below 128 (b + 1): those left of the diagonal block first, in ascending order, then the
// accumulators are doubled (exact), then the diagonal block's.  What is staged for (b, word w) is A[32 w + (0..31)][128 b +
// (0..127)] — rows of 1 KiB, the upper triangle and the diagonal blocks in full — which the MFMA reads as
// A[128 b + row][32 w + position].  Two stages in LDS: the next one travels from L2 through registers into the other buffer
// while this one is multiplied — in two halves of 16 positions, which keeps the kernel at 128 VGPRs: two workgroups a CU —,
// and one barrier a stage orders both (a wave that writes stage i + 1 has passed barrier i, which every wave reaches only
// after it has read stage i - 1 in the same buffer).  Epilogue of a row block: register r of tile j of lane l is
// row 16 j + (l >> 4) + 4 r (tile_row), variant l & 15: times x at that row, into one double a lane, j then r ascending.
// At the end lanes 0..15 add the four lane groups of their variant, ascending, and store.
__global__ __launch_bounds__(64 * WAVES, 4) void k_quad_forms(const uint32_t *__restrict__ vplanes, uint64_t n_var, uint32_t sw,
                                                           const double *__restrict__ coef, const double *__restrict__ a,
                                                           double *__restrict__ q)
{
    __shared__ f64x2 s_a[2][STAGE / 2u];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t var = (uint64_t)blockIdx.x * VARS + wave * 16u + (lane & 15u);
    const bool valid = var < n_var;
    const uint64_t plane_words = n_var * sw;
    const uint32_t *src = vplanes + (valid ? var : 0ull) * sw;
    const uint32_t k = lane >> 4;
    const uint32_t n = 32u * sw, n_blocks = (sw + 3u) / 4u;
    double c[3];
#pragma unroll
    for (uint32_t p = 0; p < 3u; ++p) c[p] = valid ? coef[var * 3u + p] : 0.0;

    // a stage by 512 threads, in two halves of 16 positions: of half h wave u fetches the positions 16 h + u, 16 h + u + 8,
    // lane l the doubles 2 l, 2 l + 1 of the 128 — columns >= n (the ragged last block) are staged as zeros
    f64x2 half[HALF];
    auto fetch = [&](uint32_t b, uint32_t w, uint32_t h) {
        const uint32_t col = BLOCK * b + 2u * lane;
#pragma unroll
        for (uint32_t i = 0; i < HALF; ++i) {
            const uint64_t row = 32u * w + 16u * h + wave + WAVES * i;
            half[i] = col < n ? *reinterpret_cast<const f64x2 *>(a + row * n + col) : f64x2{0.0, 0.0};
        }
    };
    auto put = [&](uint32_t to, uint32_t h) {
#pragma unroll
        for (uint32_t i = 0; i < HALF; ++i) s_a[to][((16u * h + wave + WAVES * i) * PITCH) / 2u + lane] = half[i];
    };
    auto words = [&](uint32_t w, uint32_t (&out)[3]) {
#pragma unroll
        for (uint32_t p = 0; p < 3u; ++p) out[p] = valid ? src[p * plane_words + w] >> k : 0u;
    };
    uint32_t next_bits[3] = {0u, 0u, 0u};
    if (sw) {
        words(0u, next_bits);
        fetch(0u, 0u, 0u), put(0u, 0u);
        fetch(0u, 0u, 1u), put(0u, 1u);
    }

    double sum = 0.0;
    uint32_t buf = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint32_t last = min(4u * b + 4u, sw);
        f64x4 acc[TILES];
#pragma unroll
        for (uint32_t j = 0; j < TILES; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};

        for (uint32_t w = 0; w < last; ++w, buf ^= 1u) {
            if (w == 4u * b) {                           // the diagonal block begins: what lies left of it counts twice
#pragma unroll
                for (uint32_t j = 0; j < TILES; ++j) acc[j] = acc[j] * 2.0;
            }
            uint32_t bits[3];
#pragma unroll
            for (uint32_t p = 0; p < 3u; ++p) bits[p] = next_bits[p];
            __syncthreads();
            // the stage after this one goes into the other buffer while this one is multiplied, a half at a time
            const bool ends = w + 1u == last;
            const uint32_t nb = ends ? b + 1u : b, nw = ends ? 0u : w + 1u;
            const bool more = nb < n_blocks;
            if (more) words(nw, next_bits), fetch(nb, nw, 0u);
            const double *a_src = reinterpret_cast<const double *>(s_a[buf]) + k * PITCH + (lane & 15u);
#pragma unroll
            for (uint32_t h = 0; h < 2u; ++h) {
#pragma unroll
                for (uint32_t t = 4u * h; t < 4u * h + 4u; ++t) {
                    const double x = x_at(c, bits[0], bits[1], bits[2], 4u * t);
#pragma unroll
                    for (uint32_t j = 0; j < TILES; ++j)
                        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_src[4u * t * PITCH + 16u * j], x, acc[j], 0, 0, 0);
                }
                if (more) {
                    put(buf ^ 1u, h);
                    if (h == 0u) fetch(nb, nw, 1u);
                }
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < BLOCK / 32u; ++i) {     // the block's own words, one at a time: x at the accumulators' rows
            uint32_t rows[3];
#pragma unroll
            for (uint32_t p = 0; p < 3u; ++p) rows[p] = (valid && 4u * b + i < sw) ? src[p * plane_words + 4u * b + i] >> k : 0u;
#pragma unroll
            for (uint32_t jj = 0; jj < 2u; ++jj)
#pragma unroll
                for (uint32_t r = 0; r < 4u; ++r)        // bit 16 jj + 4 r (+ k) of word i: tile_row(lane, r) of tile 2 i + jj
                    sum = __fma_rn(acc[2u * i + jj][r], x_at(c, rows[0], rows[1], rows[2], 16u * jj + 4u * r), sum);
        }
    }
    const double g1 = __shfl(sum, (int)(lane & 15u) + 16, 64), g2 = __shfl(sum, (int)(lane & 15u) + 32, 64),
                 g3 = __shfl(sum, (int)(lane & 15u) + 48, 64);
    if (k == 0u && valid) q[var] = ((sum + g1) + g2) + g3;
}

int launch_quad_forms(const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, const double *d_coef, const double *d_a, double *d_q,
                      hipStream_t st)
{
    if (n_var == 0) return HHGT_OK;
    if (n_var >= 0x7fffffffull * VARS || sw > HHGT_QUAD_MAX_WORDS) {
        hhgt_set_error("quad_forms: %llu variants of %llu words (fewer than %llu variants, at most %u words)",
                       (unsigned long long)n_var, (unsigned long long)sw, 0x7fffffffull * VARS, HHGT_QUAD_MAX_WORDS);
        return HHGT_ERR_ARG;
    }
    hipLaunchKernelGGL(k_quad_forms, dim3((uint32_t)((n_var + VARS - 1u) / VARS)), dim3(64 * WAVES), 0, st, d_vplanes, n_var,
                       (uint32_t)sw, d_coef, d_a, d_q);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
