// Sums of products of standardised dosages from genotype bit planes (hhgt_grm): the S x S reduction behind the genetic
// relationship matrix.  The planes are hhgt_genotype_planes' — uint32 [3][n_rows][row_words], HET, HOM_REF, HOM_ALT — and
// every bit position carries three weights, z[0] for a HOM_REF call, z[1] for HET, z[2] for HOM_ALT: a row's value at a
// position is the weight of the class whose bit is set, 0 without a bit.  A pair's entry is the sum over the positions of
// the product of the two rows' values: a matrix product, done on the f32-input MFMA.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

static constexpr uint32_t TILE = 64;                    // pairs per tile side: a workgroup owns table[64 i-rows][64 j-rows]
static constexpr uint32_t SLICE = 2;                    // plane words per row expanded at a time: 64 bit positions
static constexpr uint32_t SPAN = HHGT_GRM_SPAN;         // plane words of one f32 chain
static_assert(SPAN % SLICE == 0, "a chain ends at a slice end");

// float of (bit position p of the slice, row r of the 128: i side 0..63, j side 64..127) in the expanded slice: the 128
// rows of a position are consecutive floats, two 256-byte bank rows, and at an odd position the two halves of each side
// change places.  Staging: a wave writes one position of the 64 rows of a side (ds_write_b32, 64 banks once each, whatever
// the swap).  Operands: lane l of a wave reads row (l & 31) of its 32 at position 2 kk + (l >> 5) — the lower lanes an even
// position, the upper lanes the odd one after it, whose swap puts their 32 rows on the other 32 banks: ds_read_b32, 64
// banks once each.  Offsets between a thread's accesses are constants: one address register per parity and side.
__device__ __forceinline__ uint32_t slot(uint32_t p, uint32_t r)
{
    return p * (2u * TILE) + (r ^ ((p & 1u) << 5));
}

// grid = (T, T) for T = ceil(n_rows / 64); the workgroups with blockIdx.y <= blockIdx.x work, tile (ti = y, tj = x).  256
// threads as 4 waves: wave (wi, wj) keeps the 32 x 32 pairs (64 ti + 32 wi + ., 64 tj + 32 wj + .) in ONE accumulator of
// v_mfma_f32_32x32x2_f32 (16 registers) and their running sums in 16 doubles.  Per slice of 2 words: wave v expands word
// (v & 1) of the 64 rows of side (v >> 1) — a lane is a row: its three plane words, and per bit position three bit tests
// and selects among the position's three weights, which are the same for the whole wave (scalar loads) —, then every
// wave runs 32 MFMAs, two bit positions each, with one ds_read_b32 per operand.  The chain of a pair is the k-ordered fmaf
// chain over the positions from 32 w_lo on; after SPAN words it is added to the doubles and restarts from 0, so its error
// does not grow with the row length.  At the end tile (ti, tj) adds its doubles to table[i][j] and, above the diagonal,
// the same values to table[j][i]; a diagonal tile holds both orders itself, and they are the same bits: a product does not
// depend on the order of its factors, and both chains take the positions in the same order.  Plain read-modify-write: no
// other workgroup of the launch touches these entries.  Rows >= n_rows and words outside [w_lo, w_hi) are staged as
// zeros.
__global__ __launch_bounds__(256, 2) void k_grm(const uint32_t *__restrict__ planes, uint32_t n_rows, uint32_t row_words,
                                                uint32_t w_lo, uint32_t w_hi, const float *__restrict__ z,
                                                double *__restrict__ table)
{
    __shared__ float s_x[32u * SLICE * 2u * TILE];   // 32 KiB
    const uint32_t ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t plane_words = (uint64_t)n_rows * row_words;
    const uint64_t z_words = 32ull * row_words;
    // staging: this thread's row and word of the slice
    const uint32_t s_side = wave >> 1, s_word = wave & 1u;
    const uint32_t s_row = (s_side ? tj : ti) * TILE + lane;
    const uint32_t *s_src = planes + (uint64_t)(s_row < n_rows ? s_row : 0u) * row_words;
    // operands: row (lane & 31) of this wave's 32 on either side, position parity (lane >> 5)
    const uint32_t wi = wave >> 1, wj = wave & 1u, half = lane >> 5;
    const float *a_src = s_x + slot(half, wi * 32u + (lane & 31u));
    const float *b_src = s_x + slot(half, TILE + wj * 32u + (lane & 31u));

    f32x16 acc;
    double sum[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f, sum[r] = 0.0;
    uint32_t in_span = 0;
    for (uint32_t w0 = w_lo; w0 < w_hi; w0 += SLICE) {
        const uint32_t w = w0 + s_word;
        const bool word = w < w_hi;               // (the same for the whole wave)
        uint32_t het = 0u, ref = 0u, alt = 0u;
        if (word && s_row < n_rows) {
            het = s_src[w];
            ref = s_src[plane_words + w];
            alt = s_src[2u * plane_words + w];
        }
        __syncthreads();   // the previous slice has been read
        if (word) {
            const float4 *zw = reinterpret_cast<const float4 *>(z + 32ull * w);     // (16-byte aligned: hhgt_grm checks z)
#pragma unroll
            for (uint32_t q = 0; q < 8u; ++q) {
                const float4 z_ref = zw[q], z_het = zw[z_words / 4u + q], z_alt = zw[z_words / 2u + q];
                const float zr[4] = {z_ref.x, z_ref.y, z_ref.z, z_ref.w}, zh[4] = {z_het.x, z_het.y, z_het.z, z_het.w},
                            za[4] = {z_alt.x, z_alt.y, z_alt.z, z_alt.w};
#pragma unroll
                for (uint32_t e = 0; e < 4u; ++e) {
                    const uint32_t b = 4u * q + e;
                    const float x = (het >> b & 1u) ? zh[e] : (ref >> b & 1u) ? zr[e] : (alt >> b & 1u) ? za[e] : 0.f;
                    s_x[slot(32u * s_word + b, TILE * s_side + lane)] = x;
                }
            }
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 32u; ++b) s_x[slot(32u * s_word + b, TILE * s_side + lane)] = 0.f;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t kk = 0; kk < 16u * SLICE; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_src[kk * 4u * TILE], b_src[kk * 4u * TILE], acc, 0, 0, 0);
        in_span += SLICE;
        if (in_span == SPAN) {
            in_span = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) sum[r] += (double)acc[r], acc[r] = 0.f;
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] += (double)acc[r];
    // C/D of the 32 x 32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) for register r
    const uint32_t j = tj * TILE + wj * 32u + (lane & 31u);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t i = ti * TILE + wi * 32u + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * half;
        if (i >= n_rows || j >= n_rows) continue;
        table[(uint64_t)i * n_rows + j] += sum[r];
        if (ti != tj) table[(uint64_t)j * n_rows + i] += sum[r];
    }
}

int launch_grm(const uint32_t *d_planes, uint32_t n_rows, uint64_t row_words, uint64_t w_lo, uint64_t w_hi, const float *d_z,
               double *d_table, hipStream_t st)
{
    if (n_rows == 0 || w_lo >= w_hi) return HHGT_OK;
    const uint32_t tiles = (n_rows + TILE - 1u) / TILE;
    if (tiles > 65535u || row_words > 0x7ffffffull) {
        hhgt_set_error("grm: %u rows of %llu words (at most %u rows, 2^27 - 1 words)", n_rows,
                       (unsigned long long)row_words, 65535u * TILE);
        return HHGT_ERR_ARG;
    }
    hipLaunchKernelGGL(k_grm, dim3(tiles, tiles), dim3(256), 0, st, d_planes, n_rows, (uint32_t)row_words, (uint32_t)w_lo,
                       (uint32_t)w_hi, d_z, d_table);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
