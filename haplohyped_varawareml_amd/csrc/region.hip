// Segmented sums of per-variant weights under the bits of genotype planes (hhgt_region_sums): score.hip's product — (plane
// rows x positions) . (positions x columns), bits on the left, on the f64 MFMA — with the cuts at the boundaries of regions
// instead of every HHGT_SCORE_SPAN words, so that one pass over the planes gives every region its columns: the reduction
// behind a burden score (one number per sample and gene).  The caller brings the cuts as a table of pieces (store_plan.
// plan_regions makes it); include/hhgt.h has the contract.
#include "common.h"
#include "plane_tiles.h"

static constexpr uint32_t WAVES = 8;                     // waves per workgroup: 16 plane rows each
static constexpr uint32_t ROWS = 16u * WAVES;            // plane rows per workgroup
static constexpr uint32_t ADD_THREADS = 256;             // k_region_add: one entry a thread

// the class of weights plane k reads: the planes are HET, HOM_REF, HOM_ALT, the weights HOM_REF, HET, HOM_ALT
__device__ static constexpr uint32_t class_of_plane(uint32_t p) { return p == 0u ? 1u : p == 1u ? 0u : 2u; }

// a piece the kernel may work on: inside the rows, at most HHGT_REGION_SPAN words, its region and its slot inside their
// tables.  Everything a workgroup reads or writes lies inside what this admits
__device__ static bool piece_ok(const int64_t *piece, uint64_t row_words, uint64_t n_regions, uint64_t n_slots)
{
    const int64_t p_lo = piece[HHGT_PIECE_LO], p_hi = piece[HHGT_PIECE_HI], out = piece[HHGT_PIECE_OUT], slot = piece[HHGT_PIECE_SLOT];
    if (p_lo < 0 || p_hi < p_lo || (uint64_t)p_hi > 32ull * row_words) return false;
    if (((uint64_t)p_hi + 31u) / 32u - (uint64_t)p_lo / 32u > HHGT_REGION_SPAN) return false;
    if (out < 0 || (uint64_t)out >= n_regions) return false;
    return slot == HHGT_PIECE_DIRECT || (slot >= 0 && (uint64_t)slot < n_slots);
}

// The bit-sum tile of plane_tiles.h with one column tile and one word staged at a time, as k_score_sums<1>, over one piece:
// workgroup b owns the plane rows 128 (b % tiles) + (0..127) over the positions [p_lo, p_hi) of piece b / tiles (row tiles
// fastest: the workgroups that read one piece's weights run at about the same time); wave u its rows 16 u + (0..15).  The
// words of the piece are walked whole; in its first and last word the weights of the positions outside [p_lo, p_hi) are
// staged as 0.0 without a load, like the columns >= n_cols: a plane bit there multiplies a zero.  The accumulators go, by
// exactly one lane each, to part[slot][row][column] with a plain store (a region of several pieces: k_region_add adds them
// up), or are added to sums[row][out][column] (HHGT_PIECE_DIRECT: a region of one piece, the entry's only owner in the
// call).  A piece that piece_ok refuses is counted in *bad and touches nothing.
__global__ __launch_bounds__(64 * WAVES) void k_region_sums(const uint32_t *__restrict__ planes, uint32_t n_rows, uint64_t row_words,
                                                            uint32_t tiles, const int64_t *__restrict__ pieces,
                                                            const double *__restrict__ w, uint32_t n_cols, uint64_t n_regions,
                                                            uint64_t n_slots, double *__restrict__ part, double *__restrict__ sums,
                                                            unsigned long long *__restrict__ bad)
{
    __shared__ double s_w[3u * 32u * 16u];               // 12 KiB: [class][position of the word][16 columns]
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t tile = blockIdx.x % tiles;
    const int64_t *piece = pieces + (uint64_t)(blockIdx.x / tiles) * HHGT_PIECE_FIELDS;
    if (!piece_ok(piece, row_words, n_regions, n_slots)) {
        if (tile == 0u && threadIdx.x == 0u) atomicAdd(bad, 1ull);
        return;
    }
    const uint64_t p_lo = (uint64_t)piece[HHGT_PIECE_LO], p_hi = (uint64_t)piece[HHGT_PIECE_HI];
    const uint64_t row = (uint64_t)tile * ROWS + wave * 16u + (lane & 15u);
    const uint64_t plane_words = (uint64_t)n_rows * row_words;
    const uint32_t *src = planes + (row < n_rows ? row : 0ull) * row_words;
    const uint32_t k = lane >> 4;
    const double *b_src = s_w + k * 16u + (lane & 15u);
    const uint64_t w_begin = p_lo / 32u, w_end = (p_hi + 31u) / 32u;
    const uint64_t class_stride = 32ull * row_words;     // positions of one class of the weights

    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    for (uint64_t w0 = w_begin; w0 < w_end; ++w0) {
        uint32_t bits[3];
#pragma unroll
        for (uint32_t p = 0; p < 3u; ++p) bits[p] = row < n_rows ? src[p * plane_words + w0] : 0u;
        __syncthreads();   // the previous word has been read
#pragma unroll
        for (uint32_t q = 0; q < 3u * 32u * 16u / (64u * WAVES); ++q) {
            const uint32_t item = threadIdx.x + 64u * WAVES * q;
            const uint32_t c = item % 16u, s = item / 16u % 32u, cls = item / (16u * 32u);
            const uint64_t pos = 32ull * w0 + s;
            const double x = (c < n_cols && pos >= p_lo && pos < p_hi) ? w[(cls * class_stride + pos) * n_cols + c] : 0.0;
            s_w[weight_at<1, 1>(cls, 0u, s, c)] = x;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t t = 0; t < 8u; ++t) {
            double a[3];
#pragma unroll
            for (uint32_t p = 0; p < 3u; ++p) a[p] = bit_as_f64(bits[p], 4u * t + k);
#pragma unroll
            for (uint32_t p = 0; p < 3u; ++p) {
                const double b = b_src[weight_at<1, 1>(class_of_plane(p), 0u, 4u * t, 0u)];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p], b, acc, 0, 0, 0);
            }
        }
    }
    const uint32_t col = lane & 15u;
    if (col >= n_cols) return;
    const int64_t slot = piece[HHGT_PIECE_SLOT];
    const uint64_t out = (uint64_t)piece[HHGT_PIECE_OUT];
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint64_t out_row = (uint64_t)tile * ROWS + wave * 16u + tile_row(lane, r);
        if (out_row >= n_rows) continue;
        if (slot == HHGT_PIECE_DIRECT)
            sums[(out_row * n_regions + out) * n_cols + col] += acc[r];
        else
            part[((uint64_t)slot * n_rows + out_row) * n_cols + col] = acc[r];
    }
}

// a run the kernel may add: its region inside the table, its slots inside the workspace
__device__ static bool run_ok(const int64_t *run, uint64_t n_regions, uint64_t n_slots)
{
    const int64_t out = run[HHGT_RUN_OUT], first = run[HHGT_RUN_SLOT], n = run[HHGT_RUN_PIECES];
    return out >= 0 && (uint64_t)out < n_regions && first >= 0 && n >= 0 && (uint64_t)first <= n_slots
           && (uint64_t)n <= n_slots - (uint64_t)first;
}

// one thread an entry (run, row, column): the partial sums of the run's slots added in ascending order of the slot, starting
// from 0, the total then added to sums[row][out][column] — its only owner in the call: a plain read-modify-write.  A run
// that run_ok refuses is counted in *bad and touches nothing
__global__ __launch_bounds__(ADD_THREADS) void k_region_add(const double *__restrict__ part, const int64_t *__restrict__ runs,
                                                            uint64_t n_runs, uint32_t n_rows, uint32_t n_cols, uint64_t n_regions,
                                                            uint64_t n_slots, double *__restrict__ sums,
                                                            unsigned long long *__restrict__ bad)
{
    const uint64_t per_run = (uint64_t)n_rows * n_cols;
    const uint64_t i = (uint64_t)blockIdx.x * ADD_THREADS + threadIdx.x;
    if (i >= n_runs * per_run) return;
    const uint64_t run_index = i / per_run, e = i - run_index * per_run;
    const int64_t *run = runs + run_index * HHGT_RUN_FIELDS;
    if (!run_ok(run, n_regions, n_slots)) {
        if (e == 0u) atomicAdd(bad, 1ull);
        return;
    }
    const double *src = part + (uint64_t)run[HHGT_RUN_SLOT] * per_run + e;
    double total = 0.0;
    for (int64_t s = 0; s < run[HHGT_RUN_PIECES]; ++s) total += src[(uint64_t)s * per_run];
    const uint64_t row = e / n_cols, c = e - row * n_cols;
    sums[(row * n_regions + (uint64_t)run[HHGT_RUN_OUT]) * n_cols + c] += total;
}

// d_part: double [n_slots][n_rows][n_cols].  The caller has checked the ranges: n_rows and n_pieces at least 1, the
// workgroups of either launch below 2^31, 1 <= n_cols <= HHGT_REGION_MAX_COLS
int launch_region_sums(const uint32_t *d_planes, uint32_t n_rows, uint64_t row_words, const double *d_w, uint32_t n_cols,
                       const int64_t *d_pieces, uint64_t n_pieces, const int64_t *d_runs, uint64_t n_runs, uint64_t n_slots,
                       uint64_t n_regions, double *d_part, double *d_sums, unsigned long long *d_bad, hipStream_t st)
{
    const uint32_t tiles = (uint32_t)(((uint64_t)n_rows + ROWS - 1u) / ROWS);
    hipLaunchKernelGGL(k_region_sums, dim3((uint32_t)(tiles * n_pieces)), dim3(64 * WAVES), 0, st, d_planes, n_rows, row_words, tiles,
                       d_pieces, d_w, n_cols, n_regions, n_slots, d_part, d_sums, d_bad);
    HIP_TRY(hipGetLastError());
    if (!n_runs) return HHGT_OK;
    const uint64_t n_entries = n_runs * n_rows * n_cols;
    hipLaunchKernelGGL(k_region_add, dim3((uint32_t)((n_entries + ADD_THREADS - 1u) / ADD_THREADS)), dim3(ADD_THREADS), 0, st, d_part,
                       d_runs, n_runs, n_rows, n_cols, n_regions, n_slots, d_sums, d_bad);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
