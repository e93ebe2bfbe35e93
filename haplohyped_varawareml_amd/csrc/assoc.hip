// Sums of per-sample weights under the bits of variant-major planes (hhgt_assoc_sums): the reduction over samples behind a
// single-variant association scan.  The planes are hhgt_variant_planes' — uint32 [3][n_var][sw], 32 samples per word — and
// every bit position (sample) carries a row of n_cols doubles; an entry of the result is the sum of one column over the
// positions at which one row of one plane has a 1: a (variants x samples) . (samples x columns) product whose left factor is
// bits, done on the f64 MFMA.  include/hhgt.h has the contract.
#include "common.h"
#include "plane_tiles.h"

static constexpr uint32_t WAVES = 8;                     // waves per workgroup: 16 variants each
static constexpr uint32_t VARS = 16u * WAVES;            // variants per workgroup
static constexpr uint32_t SLICE = 4;                     // sample words per row staged at a time: 128 rows of the weights

// The bit-sum tile of plane_tiles.h with a variant for a row and a sample for a position.  grid = ceil(n_var / 128); wave u
// owns the variants 128 b + 16 u + (0..15) x the three planes x all column tiles: 3 CT accumulators (4 doubles a lane each: 96
// registers at CT = 4), one class of weights that all three planes read.  A variant's words are sw apart, 16 distinct
// addresses a wave — a row's words stay in cache for the next slices.  Samples of words >= sw are staged as zeros.
// The weights do not fit LDS whole (2560 x 16 doubles = 320 KiB): every workgroup reads all of them once, slice by slice,
// from L2; 128 variants a workgroup keep that traffic near the planes' own.
template <uint32_t CT>
__global__ __launch_bounds__(64 * WAVES) void k_assoc_sums(const uint32_t *__restrict__ vplanes, uint64_t n_var, uint32_t sw,
                                                           const double *__restrict__ w, uint32_t n_cols,
                                                           double *__restrict__ sums)
{
    __shared__ double s_w[CT * 32u * SLICE * 16u];      // 16 KiB a column tile
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t var = (uint64_t)blockIdx.x * VARS + wave * 16u + (lane & 15u);
    const uint64_t plane_words = n_var * sw;
    const uint32_t *src = vplanes + (var < n_var ? var : 0ull) * sw;
    const uint32_t k = lane >> 4;
    const double *b_src = s_w + k * 16u + (lane & 15u);

    f64x4 acc[3][CT];
#pragma unroll
    for (uint32_t p = 0; p < 3u; ++p)
#pragma unroll
        for (uint32_t ct = 0; ct < CT; ++ct) acc[p][ct] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (uint32_t w0 = 0; w0 < sw; w0 += SLICE) {
        uint32_t bits[3][SLICE];
#pragma unroll
        for (uint32_t p = 0; p < 3u; ++p)
#pragma unroll
            for (uint32_t i = 0; i < SLICE; ++i)
                bits[p][i] = (var < n_var && i < sw - w0) ? src[p * plane_words + w0 + i] : 0u;
        __syncthreads();   // the previous slice has been read
#pragma unroll
        for (uint32_t q = 0; q < CT * 32u * SLICE * 16u / (64u * WAVES); ++q) {
            const uint32_t item = threadIdx.x + 64u * WAVES * q;
            const uint32_t c = item % (CT * 16u), s = item / (CT * 16u);       // (constants: shifts, or a multiply for 48)
            const uint64_t row = 32ull * w0 + s;
            const double x = (c < n_cols && row < 32ull * sw) ? w[row * n_cols + c] : 0.0;
            s_w[weight_at<CT, SLICE>(0u, c >> 4, s, c & 15u)] = x;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < SLICE; ++i) {
#pragma unroll
            for (uint32_t t = 0; t < 8u; ++t) {
                double a[3];
#pragma unroll
                for (uint32_t p = 0; p < 3u; ++p) a[p] = bit_as_f64(bits[p][i], 4u * t + k);
#pragma unroll
                for (uint32_t ct = 0; ct < CT; ++ct) {
                    const double b = b_src[weight_at<CT, SLICE>(0u, ct, 32u * i + 4u * t, 0u)];
#pragma unroll
                    for (uint32_t p = 0; p < 3u; ++p)
                        acc[p][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p], b, acc[p][ct], 0, 0, 0);
                }
            }
        }
    }
    const uint32_t col = lane & 15u;
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint64_t v = (uint64_t)blockIdx.x * VARS + wave * 16u + tile_row(lane, r);
        if (v >= n_var) continue;
#pragma unroll
        for (uint32_t p = 0; p < 3u; ++p)
#pragma unroll
            for (uint32_t ct = 0; ct < CT; ++ct) {
                const uint32_t c = ct * 16u + col;
                if (c < n_cols) sums[(v * 3u + p) * n_cols + c] = acc[p][ct][r];
            }
    }
}

int launch_assoc_sums(const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, const double *d_w, uint32_t n_cols,
                      double *d_sums, hipStream_t st)
{
    if (n_var == 0) return HHGT_OK;
    const uint64_t blocks = (n_var + VARS - 1u) / VARS;
    if (blocks > 0x7fffffffull || sw >= (1ull << 27)) {
        hhgt_set_error("assoc_sums: %llu variants of %llu words (at most %llu variants, 2^27 - 1 words)",
                       (unsigned long long)n_var, (unsigned long long)sw, 0x7fffffffull * VARS);
        return HHGT_ERR_ARG;
    }
    by_column_tiles(n_cols, [&](auto ct) {
        hipLaunchKernelGGL(k_assoc_sums<decltype(ct)::value>, dim3((uint32_t)blocks), dim3(64 * WAVES), 0, st, d_vplanes, n_var,
                           (uint32_t)sw, d_w, n_cols, d_sums);
    });
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
