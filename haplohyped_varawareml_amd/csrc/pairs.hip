// Pairwise sample counts from genotype bit planes (hhgt_pair_counts): the S x S reduction behind kinship and identity by
// state.  The planes are hhgt_genotype_planes' — uint32 [3][n_rows][row_words], HET, HOM_REF, HOM_ALT, 32 variants per
// word, a variant that is not counted is a 0 bit in all three — so a pair's counters are popcounts of ANDs of two rows.
#include "common.h"
#include "plane_tiles.h"

static constexpr uint32_t TILE = 64;     // pairs per tile side: a workgroup owns table[64 i-rows][64 j-rows]
static constexpr uint32_t SLICE = 16;    // plane words per row staged at a time: 64 bytes of each row and plane

// grid = (T, T) for T = ceil(n_rows / 64); the workgroups with blockIdx.y <= blockIdx.x work, tile (ti = y, tj = x).  256
// threads as 16 x 16: thread (ty, tx) keeps the pairs (i, j) = (64 ti + ty + 16 a, 64 tj + tx + 16 b), a, b = 0..3, and
// five counters per pair in registers: NSNP, HETHET, IBS0, HET1[i][j] and HET1[j][i].  Per slice of 16 words the 64 + 64
// rows go to LDS as one uint4 (HET, M = HET | REF | ALT, REF, ALT) per row and word; per word a thread reads its 4 i-rows
// and 4 j-rows (8 ds_read_b128: the j-side address is the same down a column of threads, the i-side along a row — a wave
// reads 16 + 4 distinct slots) and does 11 VALU operations per pair.  At the end tile (ti, tj) adds its counters to
// table[i][j] and, above the diagonal, the mirrored ones to table[j][i]; a diagonal tile holds both orders itself.  Plain
// read-modify-write: no other workgroup of the launch touches these entries.  Rows >= n_rows and words outside
// [w_lo, w_hi) are staged as zeros: they count nothing.
__global__ __launch_bounds__(256, 4) void k_pair_counts(const uint32_t *__restrict__ planes, uint32_t n_rows,
                                                        uint32_t row_words, uint32_t w_lo, uint32_t w_hi,
                                                        uint4 *__restrict__ table)
{
    __shared__ u32x4 s_slice[2u * SLICE * (TILE + 1u)];   // 32.5 KiB
    const uint32_t ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint64_t plane_words = (uint64_t)n_rows * row_words;
    uint32_t nsnp[4][4], hh[4][4], ibs0[4][4], h1[4][4], h2[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) nsnp[a][b] = hh[a][b] = ibs0[a][b] = h1[a][b] = h2[a][b] = 0u;
    for (uint32_t w0 = w_lo; w0 < w_hi; w0 += SLICE) {
        stage_slice<TILE, SLICE, 4>(s_slice, planes, row_words, plane_words, ti * TILE, tj * TILE, n_rows, w0, w_hi - w0,
                                    [](uint32_t het, uint32_t ref, uint32_t alt) { return u32x4{het, het | ref | alt, ref, alt}; });
#pragma unroll 4
        for (uint32_t w = 0; w < SLICE; ++w) {
            u32x4 I[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) I[a] = s_slice[tile_slot<TILE, SLICE>(0u, w, ty + 16u * (uint32_t)a)];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const u32x4 J = s_slice[tile_slot<TILE, SLICE>(1u, w, tx + 16u * (uint32_t)b)];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    bcnt_acc(nsnp[a][b], I[a].y & J.y);
                    bcnt_acc(hh[a][b], I[a].x & J.x);
                    bcnt_acc(ibs0[a][b], (I[a].z & J.w) | (I[a].w & J.z));
                    bcnt_acc(h1[a][b], I[a].x & J.y);
                    bcnt_acc(h2[a][b], I[a].y & J.x);
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const uint32_t i = ti * TILE + ty + 16u * (uint32_t)a;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t j = tj * TILE + tx + 16u * (uint32_t)b;
            if (i >= n_rows || j >= n_rows) continue;
            asm volatile("" ::: "memory");   // one entry at a time: 16 hoisted table loads would not fit the register file
            uint4 *e = table + ((uint64_t)i * n_rows + j);
            uint4 t = *e;
            t.x += nsnp[a][b], t.y += hh[a][b], t.z += ibs0[a][b], t.w += h1[a][b];
            *e = t;
            if (ti != tj) {
                e = table + ((uint64_t)j * n_rows + i);
                t = *e;
                t.x += nsnp[a][b], t.y += hh[a][b], t.z += ibs0[a][b], t.w += h2[a][b];
                *e = t;
            }
        }
    }
}

int launch_pair_counts(const uint32_t *d_planes, uint32_t n_rows, uint64_t row_words, uint64_t w_lo, uint64_t w_hi,
                       uint32_t *d_table, hipStream_t st)
{
    if (n_rows == 0 || w_lo >= w_hi) return HHGT_OK;
    const uint32_t tiles = (n_rows + TILE - 1u) / TILE;
    if (tiles > 65535u || row_words > 0xfffffff0ull) {
        hhgt_set_error("pair_counts: %u rows of %llu words (at most %u rows, 2^32 - 16 words)", n_rows,
                       (unsigned long long)row_words, 65535u * TILE);
        return HHGT_ERR_ARG;
    }
    hipLaunchKernelGGL(k_pair_counts, dim3(tiles, tiles), dim3(256), 0, st, d_planes, n_rows, (uint32_t)row_words,
                       (uint32_t)w_lo, (uint32_t)w_hi, reinterpret_cast<uint4 *>(d_table));
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
