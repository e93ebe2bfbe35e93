// The two tiles the reductions over bit planes are made of, once each: the popcount tile of pairs.hip (k_pair_counts) and
// ld.hip (k_ld_counts), and the bit-sum tile of assoc.hip (k_assoc_sums) and score.hip (k_score_sums).  Device functions inlined
// into the kernels, and the host-side choice of a bit-sum kernel's instantiation; what a kernel counts or sums, what it owns and
// how it is launched stay in its file.
#pragma once
#include <stdint.h>
#include <type_traits>

// ---- the popcount tile: two sides of TILE plane rows, SLICE words of each at a time, as 16-byte LDS slots --------------------

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // one slot: a row's word in the three planes, and a fourth

// slot of (word w of the slice, row r of a side) in the staged slice: the TILE rows of a word are consecutive 16-byte slots
// (the 16 lanes of a ds_read_b128 group read 16 rows of one word: one 256-byte bank row), and a word's rows begin one slot
// past a bank row after the previous word's (the 8 lanes of a ds_write_b128 group store 8 words of one row).  Offsets
// between a thread's reads are constants: one address register per side.
template <uint32_t TILE, uint32_t SLICE>
__device__ __forceinline__ uint32_t tile_slot(uint32_t side, uint32_t w, uint32_t r)
{
    return (side * SLICE + w) * (TILE + 1u) + r;
}

// acc += popcount(x): v_bcnt_u32_b32 adds into its third operand.  Said as one instruction so that the 80 counters of a
// thread of k_pair_counts stay 80 scalar registers (left to the vectoriser, __builtin_popcount + add pairs them up and spills)
__device__ __forceinline__ void bcnt_acc(uint32_t &acc, uint32_t x)
{
    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(x));
}

// one slice into s_slice [2 SLICE (TILE + 1)], by 256 threads: the words w0 + (0 .. SLICE) of the rows row0_i + (0 .. TILE)
// (side 0) and row0_j + (0 .. TILE) (side 1) of planes [3][n_rows][row_stride] at `base` (plane_words = n_rows row_stride).
// item = (row of the 2 TILE, word of the slice): consecutive lanes on consecutive words of one row.  make(a, b, c) turns the
// word of planes 0, 1, 2 into the slot; rows >= n_rows and words >= words_left are staged as zeros: they count nothing.
// Between two barriers: the previous slice has been read before, this one is complete after.  UNROLL: of the items' loop.
// Row: the type the kernel indexes its rows in (the code that comes out differs between 32 and 64 bits)
template <uint32_t TILE, uint32_t SLICE, uint32_t UNROLL, typename Row, typename Make>
__device__ __forceinline__ void stage_slice(u32x4 *s_slice, const uint32_t *__restrict__ base, uint32_t row_stride,
                                            uint64_t plane_words, Row row0_i, Row row0_j, uint32_t n_rows, uint32_t w0,
                                            uint32_t words_left, Make make)
{
    __syncthreads();
#pragma unroll UNROLL
    for (uint32_t q = 0; q < 2u * TILE * SLICE / 256u; ++q) {
        const uint32_t item = threadIdx.x + 256u * q;
        const uint32_t w = item & (SLICE - 1u), rr = item / SLICE, side = rr / TILE, r = rr & (TILE - 1u);
        const Row row = (side ? row0_j : row0_i) + r;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (row < n_rows && w < words_left) {
            const uint32_t *p = base + (uint64_t)row * row_stride + w0 + w;
            v = make(p[0], p[plane_words], p[2u * plane_words]);
        }
        s_slice[tile_slot<TILE, SLICE>(side, w, r)] = v;
    }
    __syncthreads();
}

// ---- the bit-sum tile: (rows x positions) . (positions x columns) with bits on the left, on v_mfma_f64_16x16x4_f64 -----------
//
// 512 threads as 8 waves; CT = ceil(n_cols / 16) column tiles.  A wave owns 16 plane rows x all column tiles and walks the words
// of its rows, SLICE at a time.  A: lane l is plane row (l & 15) and position (l >> 4) of a step of four positions; it holds
// the slice's words of its row in each plane (the four lanes of a row load the same word) and per step takes bit
// 4 t + (l >> 4) of each as 0.0 / 1.0 (bit_as_f64).  B: the slice's weights, staged by the whole workgroup in LDS as
// [class][column tile][position][16 doubles] (weight_at) — columns >= n_cols and positions past the end as
// zeros, so that no product reads what nobody wrote —; lane l reads double (l & 15) of position 4 t + (l >> 4): the 32 lanes
// of one ds_read_b64 pass read two consecutive positions' 128 bytes, 256 consecutive bytes, every bank once.  The products are
// 0 or a weight exactly, and an accumulator takes the positions in ascending order: the same order on every call.  At the
// end register r of lane l is row (l >> 4) + 4 r (tile_row), column l & 15 (the f64 C/D map: not the f32 one): 16 lanes store
// 128 consecutive bytes.  The loads of the words, the staging loop and the store stand in each kernel: as functions
// here the latter two cost registers (k_score_sums<3> 115 against 113 for the staging, k_assoc_sums<4> 186 against 184 for the
// store) and the loads cost k_score_sums time (0.4 % at 10 columns, 0.9 % at 64: DESIGN.md 6a), with the same text inside.

typedef double f64x4 __attribute__((ext_vector_type(4)));

// bit `bit` of the word as 0.0 / 1.0: the bit, sign-extended, masks the high half of 1.0
__device__ __forceinline__ double bit_as_f64(uint32_t word, uint32_t bit)
{
    const int32_t on = ((int32_t)(word << (31u - bit))) >> 31;
    return __hiloint2double(on & 0x3ff00000, 0);
}

// where the weight of (class, column tile, position of the slice, column of the tile) lies in LDS
template <uint32_t CT, uint32_t SLICE>
__device__ __forceinline__ constexpr uint32_t weight_at(uint32_t cls, uint32_t tile, uint32_t pos, uint32_t col)
{
    return ((cls * CT + tile) * 32u * SLICE + pos) * 16u + col;
}

// the row of its 16 x 16 tile that register r of lane `lane` holds in the C/D of the f64 MFMA; its column is lane & 15
__device__ __forceinline__ constexpr uint32_t tile_row(uint32_t lane, uint32_t r) { return (lane >> 4) + 4u * r; }

// f(std::integral_constant<uint32_t, CT>) for CT = ceil(n_cols / 16), 1 <= n_cols <= 64: the kernels' instantiations
template <typename F>
static inline void by_column_tiles(uint32_t n_cols, F f)
{
    switch ((n_cols + 15u) / 16u) {
    case 1: f(std::integral_constant<uint32_t, 1>{}); break;
    case 2: f(std::integral_constant<uint32_t, 2>{}); break;
    case 3: f(std::integral_constant<uint32_t, 3>{}); break;
    default: f(std::integral_constant<uint32_t, 4>{}); break;
    }
}
