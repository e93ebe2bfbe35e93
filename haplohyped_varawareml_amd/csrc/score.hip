// Sums of per-variant weights under the bits of genotype planes (hhgt_score_sums): the reduction over variants behind a
// polygenic score and behind the projection of a sample onto principal components.  The planes are hhgt_genotype_planes' —
// uint32 [3][n_rows][row_words], 32 variants per word — and every bit position (variant) carries, per dosage class, a row of
// n_cols doubles; an entry of the result is the sum of one column over the positions at which a plane row has a 1, the three
// planes together: a (samples x variants) . (variants x columns) product whose left factor is bits, done on the f64 MFMA —
// the transpose of assoc.hip's.  include/hhgt.h has the contract.
#include "common.h"
#include "plane_tiles.h"

static constexpr uint32_t WAVES = 8;                     // waves per workgroup: 16 plane rows each
static constexpr uint32_t ROWS = 16u * WAVES;            // plane rows per workgroup
static constexpr uint32_t SLICE = HHGT_SCORE_SLICE;      // words per row staged at a time: 32 positions x 3 classes each
static constexpr uint32_t ADD_THREADS = 256;             // k_score_add: one entry a thread

// the class of weights plane k reads: the planes are HET, HOM_REF, HOM_ALT, the weights HOM_REF, HET, HOM_ALT
__device__ static constexpr uint32_t class_of_plane(uint32_t p) { return p == 0u ? 1u : p == 1u ? 0u : 2u; }

// The bit-sum tile of plane_tiles.h with a plane row (a sample's row) for a row and a variant for a position.  grid =
// (ceil(n_rows / 128), spans): workgroup (b, y) owns the plane rows 128 b + (0..127) over the words [w_lo + y span,
// min(w_lo + (y + 1) span, w_hi)); wave u its rows 16 u + (0..15) x all column tiles: CT accumulators (4 doubles a lane each:
// 32 registers at CT = 4), into which the three planes' MFMAs chain, each plane against its class of weights: at a position
// the planes in their order.  Positions of words past the span's end are staged as zeros, and nothing outside [w_lo, w_hi) is
// loaded.  The accumulators go to part[y][row][column] with a plain store: every entry of the span's partial table that
// belongs to a row and a column is written, by exactly one lane.
// The weights do not fit LDS: every row tile streams its spans' weights once from L2 / MALL.  128 rows a tile, not 256: a
// 256-row tile would halve that stream (an estimate: at 2560 rows, 230 k positions and 16 columns, 10 x 88 MB in place of
// 20 x 88 MB), but needs 16 waves a workgroup or two accumulator sets a wave, and the stream is served by the caches, not
// by HBM (the weights of a span, 48 KiB x columns / 16 x 64 words, are read by all row tiles at about the same time) —
// neither alternative has been measured.
template <uint32_t CT>
__global__ __launch_bounds__(64 * WAVES) void k_score_sums(const uint32_t *__restrict__ planes, uint32_t n_rows, uint64_t row_words,
                                                           uint64_t w_lo, uint64_t w_hi, uint64_t span,
                                                           const double *__restrict__ w, uint32_t n_cols,
                                                           double *__restrict__ part)
{
    __shared__ double s_w[3u * CT * 32u * SLICE * 16u];  // 12 KiB a column tile and word
    constexpr uint32_t STEP_UNROLL = CT >= 3u ? 4u : 8u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t row = (uint64_t)blockIdx.x * ROWS + wave * 16u + (lane & 15u);
    const uint64_t plane_words = (uint64_t)n_rows * row_words;
    const uint32_t *src = planes + (row < n_rows ? row : 0ull) * row_words;
    const uint32_t k = lane >> 4;
    const double *b_src = s_w + k * 16u + (lane & 15u);
    const uint64_t w_begin = w_lo + (uint64_t)blockIdx.y * span;
    const uint64_t w_end = w_begin + span < w_hi ? w_begin + span : w_hi;
    const uint64_t class_stride = 32ull * row_words;     // positions of one class of the weights

    f64x4 acc[CT];
#pragma unroll
    for (uint32_t ct = 0; ct < CT; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (uint64_t w0 = w_begin; w0 < w_end; w0 += SLICE) {
        uint32_t bits[3][SLICE];
#pragma unroll
        for (uint32_t p = 0; p < 3u; ++p)
#pragma unroll
            for (uint32_t i = 0; i < SLICE; ++i)
                bits[p][i] = (row < n_rows && w0 + i < w_end) ? src[p * plane_words + w0 + i] : 0u;
        __syncthreads();   // the previous slice has been read
#pragma unroll
        for (uint32_t q = 0; q < 3u * CT * 32u * SLICE * 16u / (64u * WAVES); ++q) {
            const uint32_t item = threadIdx.x + 64u * WAVES * q;
            const uint32_t c = item % (CT * 16u), rest = item / (CT * 16u);    // (constants: shifts, or a multiply for 48)
            const uint32_t s = rest % (32u * SLICE), cls = rest / (32u * SLICE);
            const uint64_t pos = 32ull * w0 + s;
            const double x = (c < n_cols && pos < 32ull * w_end) ? w[(cls * class_stride + pos) * n_cols + c] : 0.0;
            s_w[weight_at<CT, SLICE>(cls, c >> 4, s, c & 15u)] = x;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < SLICE; ++i) {
            // the eight steps of a word unrolled whole up to two column tiles, by four beyond: whole, the compiler reads all
            // of a word's B ahead of the chain, and at CT = 4 that costs the second resident workgroup (148 registers against
            // 100); measured, alternating: 6.42 -> 4.61 ms at 64 columns, while by four is 3 % slower at CT = 1.  CT = 2 and 3
            // were not measured apart: 3 goes with 4 because whole costs it the second workgroup too (132 against 114)
#pragma unroll STEP_UNROLL
            for (uint32_t t = 0; t < 8u; ++t) {
                double a[3];
#pragma unroll
                for (uint32_t p = 0; p < 3u; ++p) a[p] = bit_as_f64(bits[p][i], 4u * t + k);
#pragma unroll
                for (uint32_t ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (uint32_t p = 0; p < 3u; ++p) {
                        const double b = b_src[weight_at<CT, SLICE>(class_of_plane(p), ct, 32u * i + 4u * t, 0u)];
                        acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p], b, acc[ct], 0, 0, 0);
                    }
            }
        }
    }
    const uint32_t col = lane & 15u;
    double *dst = part + (uint64_t)blockIdx.y * n_rows * n_cols;
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint64_t out_row = (uint64_t)blockIdx.x * ROWS + wave * 16u + tile_row(lane, r);
        if (out_row >= n_rows) continue;
#pragma unroll
        for (uint32_t ct = 0; ct < CT; ++ct) {
            const uint32_t c = ct * 16u + col;
            if (c < n_cols) dst[out_row * n_cols + c] = acc[ct][r];
        }
    }
}

// one thread an entry of sums [n_rows][n_cols]: the spans' partial sums added in ascending order of the span, the total
// then added to the entry — its only owner in the launch: a plain read-modify-write
__global__ __launch_bounds__(ADD_THREADS) void k_score_add(const double *__restrict__ part, uint32_t n_spans, uint64_t n_entries,
                                                           double *__restrict__ sums)
{
    const uint64_t i = (uint64_t)blockIdx.x * ADD_THREADS + threadIdx.x;
    if (i >= n_entries) return;
    double total = 0.0;
    for (uint32_t s = 0; s < n_spans; ++s) total += part[(uint64_t)s * n_entries + i];
    sums[i] += total;
}

// the span of a range of n_words words, as include/hhgt.h states it: HHGT_SCORE_SPAN, or the multiple of it that keeps the
// spans within grid.y; a function of the range's length alone
uint64_t score_span_words(uint64_t n_words)
{
    const uint64_t units = (n_words + HHGT_SCORE_SPAN - 1u) / HHGT_SCORE_SPAN;
    const uint64_t per = (units + HHGT_SCORE_MAX_SPANS - 1u) / HHGT_SCORE_MAX_SPANS;
    return HHGT_SCORE_SPAN * (per ? per : 1u);
}

uint64_t score_spans(uint64_t n_words)
{
    const uint64_t span = score_span_words(n_words);
    return (n_words + span - 1u) / span;
}

// d_part: double [score_spans(w_hi - w_lo)][n_rows][n_cols], every entry of which the first launch writes.  The caller has
// checked the ranges (n_rows below 2^32, row_words below 2^27, w_lo < w_hi <= row_words, 1 <= n_cols <= 64)
int launch_score_sums(const uint32_t *d_planes, uint32_t n_rows, uint64_t row_words, uint64_t w_lo, uint64_t w_hi, const double *d_w,
                      uint32_t n_cols, double *d_part, double *d_sums, hipStream_t st)
{
    const uint64_t span = score_span_words(w_hi - w_lo), spans = score_spans(w_hi - w_lo);
    const uint64_t tiles = ((uint64_t)n_rows + ROWS - 1u) / ROWS;
    by_column_tiles(n_cols, [&](auto ct) {
        hipLaunchKernelGGL(k_score_sums<decltype(ct)::value>, dim3((uint32_t)tiles, (uint32_t)spans), dim3(64 * WAVES), 0, st, d_planes,
                           n_rows, row_words, w_lo, w_hi, span, d_w, n_cols, d_part);
    });
    HIP_TRY(hipGetLastError());
    const uint64_t n_entries = (uint64_t)n_rows * n_cols;
    hipLaunchKernelGGL(k_score_add, dim3((uint32_t)((n_entries + ADD_THREADS - 1u) / ADD_THREADS)), dim3(ADD_THREADS), 0, st, d_part,
                       (uint32_t)spans, n_entries, d_sums);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
