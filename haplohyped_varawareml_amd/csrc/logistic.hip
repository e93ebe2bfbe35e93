// Per-variant logistic regression of a 0 / 1 phenotype on [X | dosage] by Newton's method, from variant-major planes
// (hhgt_logistic_fit): the part of a case / control association scan that is not a sum.  include/hhgt.h has the contract.
#include "common.h"
#include "plane_tiles.h"
#include <utility>

static constexpr uint32_t WAVES = 8;                     // waves per workgroup: a variant at a time each
static constexpr uint32_t VARS = 64;                     // variants per workgroup
static constexpr uint32_t SLICE = 4;                     // sample words staged at a time: 128 rows of X
static constexpr uint32_t POS = 32u * SLICE;             // positions of a slice
static constexpr uint32_t XCOLS = HHGT_LOGIT_MAX_COLS - 1u;      // columns of X at most
static constexpr uint32_t G = HHGT_LOGIT_MAX_COLS - 1u;  // the dosage's row and column of the tile, whatever q
static constexpr uint32_t UCOL = 15;                     // the tile's column that carries U
// a column of the staged slice is POS doubles and 4 of padding: the 16 columns that the lanes of an MFMA operand read at one
// position lie 4 doubles apart modulo the banks, beside the 4 positions of the step
static constexpr uint32_t XSTRIDE = POS + 4u;

// lane `src`'s value, the same in every lane (src: a constant once the loops are unrolled)
__device__ __forceinline__ double lane_value(double v, uint32_t src)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), (int)src),
                            __builtin_amdgcn_readlane(__double2loint(v), (int)src));
}

// the sum of the lanes' values, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// What an evaluation leaves: delta = H^-1 U (the same in every lane), (H^-1)_gg, U_g, and whether every pivot stood.
struct Solved {
    double delta[HHGT_LOGIT_MAX_COLS];
    double hinv, u_g;
    bool ok;
};

// H and U from the accumulator of the tile (register r of lane l: row tile_row(l, r), column l & 15) through the wave's
// 16 x 16 doubles of LDS into rows: lane l holds row l & 15 of H (the four lanes of a row alike), a[c] for c <= row the
// lower triangle.  Rows q .. G - 1 belong to no column of X: they are made rows of the identity, which the factorisation
// passes through untouched.  Right-looking Cholesky, a pivot and a column of L broadcast per step; then L z = U by columns
// and L^T delta = z by rows, on values every lane holds.
__device__ __forceinline__ Solved solve_tile(const f64x4 &acc, double *s_tile, uint32_t lane, uint32_t q)
{
    constexpr uint32_t N = HHGT_LOGIT_MAX_COLS;
    const uint32_t row = lane & 15u;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) s_tile[tile_row(lane, r) * 16u + row] = acc[r];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // (H is symmetric: column `row` of the tile, read as a row — 16 lanes on 16 consecutive doubles)
    double a[N];
    const bool pad = row >= q && row < G;
#pragma unroll
    for (uint32_t c = 0; c < N; ++c) {
        const double h = s_tile[c * 16u + row];
        a[c] = pad ? (c == row ? 1.0 : 0.0) : h;
    }
    double u = pad ? 0.0 : s_tile[row * 16u + UCOL];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    Solved s;
    s.u_g = lane_value(u, G);
    s.ok = true;
    double diag = 0.0;
#pragma unroll
    for (uint32_t c = 0; c < N; ++c) diag = c == row ? a[c] : diag;
    double lkk[N];
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) {
        const double d = lane_value(a[k], k);
        s.ok = s.ok && d > 1e-12 * lane_value(diag, k);          // (a NaN fails)
        lkk[k] = sqrt(d);
        a[k] = a[k] / lkk[k];                                    // column k of L, in the lanes of the rows >= k
#pragma unroll
        for (uint32_t c = k + 1u; c < N; ++c) a[c] = fma(-a[k], lane_value(a[k], c), a[c]);
    }
    s.hinv = 1.0 / (lkk[G] * lkk[G]);
    double z[N];
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) {
        z[k] = lane_value(u, k) / lkk[k];
        u = fma(-a[k], z[k], u);
    }
#pragma unroll
    for (uint32_t i = N; i-- > 0u;) {
        s.delta[i] = z[i] / lkk[i];
#pragma unroll
        for (uint32_t k = 0; k < i; ++k) z[k] = fma(-lane_value(a[k], i), s.delta[i], z[k]);
    }
    return s;
}

// lane t of the caller's row of 16 lanes' value, in every lane of that row (DPP row_share: no LDS)
template <uint32_t T>
__device__ __forceinline__ double row_value(double v)
{
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x150 + T, 0xf, 0xf, false),
                            __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x150 + T, 0xf, 0xf, false));
}

// step T of a block's 16: lane l is row / column l & 15 of the tile and the position 4 T + (l >> 4), whose w, y - mu and g
// lane T of its row of 16 holds (the order of the positions among a block's lanes is made for this); xs: the lane's column
// of the staged X at the block's position l >> 4
template <uint32_t T>
__device__ __forceinline__ void tile_step(f64x4 &acc, double w, double r, double g, const double *xs, uint32_t row)
{
    const double wv = row_value<T>(w), rv = row_value<T>(r), gv = row_value<T>(g);
    const double av = row < XCOLS ? xs[4u * T] : row == G ? gv : 0.0;
    const double bv = row == UCOL ? rv : wv * av;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
}

template <uint32_t... T>
__device__ __forceinline__ void tile_steps(std::integer_sequence<uint32_t, T...>, f64x4 &acc, double w, double r, double g,
                                           const double *xs, uint32_t row)
{
    (tile_step<T>(acc, w, r, g, xs, row), ...);
}

// What a wave keeps of the variant it is fitting.
struct Fit {
    uint64_t var;
    const uint32_t *src;                                 // the variant's row of the HET plane
    uint32_t m, h, a, steps;
    double mean, hinv, u0, hinv0;
    int status;
    bool last;                                           // the steps have ended: the next evaluation gives (H^-1)_gg only
};

__device__ __forceinline__ void store_record(double *__restrict__ out, const Fit &f, double gamma, uint32_t lane)
{
    if (lane != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const bool tested = f.status == HHGT_LOGIT_TESTED;
    double *rec = out + f.var * HHGT_LOGIT_REC;
    rec[HHGT_LOGIT_GAMMA] = tested ? gamma : nan;
    rec[HHGT_LOGIT_HINV] = tested ? f.hinv : nan;
    rec[HHGT_LOGIT_U0] = f.u0;
    rec[HHGT_LOGIT_HINV0] = f.hinv0;
    rec[HHGT_LOGIT_STEPS] = (double)f.steps;
    rec[HHGT_LOGIT_STATUS] = (double)f.status;
    rec[HHGT_LOGIT_N_COMPLETE] = (double)f.m;
    rec[HHGT_LOGIT_N_HET] = (double)f.h;
    rec[HHGT_LOGIT_N_ALT] = (double)f.a;
}

// grid = ceil(n_var / VARS): a workgroup owns VARS consecutive variants and its waves draw them one at a time from a
// counter in LDS — a variant that separates the classes takes 26 evaluations where its neighbours take 5, and a wave that
// is done with one goes on to the next instead of waiting; which wave fits a variant changes nothing of its arithmetic.
// The workgroup goes round by round, a round one evaluation for every wave that has a variant, all of them over the same
// positions slice by slice: the workgroup stages the slice's rows of X as columns (positions without a valid bit and past the
// end as zeros; the columns q .. 13 are zeros from the start), then every such wave takes the slice's two blocks of 64
// positions — with a lane for a position, eta, mu, and w, y - mu, g; then the block's 16 steps of the MFMA (tile_step).  A
// variant that is not fitted costs its wave the count of its calls and no round.  The rounds end when no wave has a variant.
__global__ __launch_bounds__(64 * WAVES) void k_logistic_fit(const uint32_t *__restrict__ vplanes, uint64_t n_var, uint32_t sw,
                                                             const uint32_t *__restrict__ valid, const double *__restrict__ x,
                                                             uint32_t q, const double *__restrict__ y,
                                                             const double *__restrict__ beta0, double *__restrict__ out)
{
    __shared__ double s_x[XCOLS * XSTRIDE];
    __shared__ double s_tile[WAVES][16 * 16];
    __shared__ uint32_t s_next;                          // the next variant of the workgroup's to draw
    __shared__ int s_running;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t plane_words = n_var * sw;
    const uint64_t var0 = (uint64_t)blockIdx.x * VARS;
    const uint32_t row = lane & 15u, k = lane >> 4;
    const uint32_t spot = 4u * row + k;                  // the position of a block that this lane evaluates
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    for (uint32_t i = threadIdx.x; i < XCOLS * XSTRIDE; i += 64u * WAVES) s_x[i] = 0.0;
    if (threadIdx.x == 0) s_next = 0;
    __syncthreads();

    Fit f;
    double theta[HHGT_LOGIT_MAX_COLS];
    // the next variant of the workgroup's that is to be fitted, those that are not recorded on the way -> whether there is one
    auto draw = [&]() -> bool {
        for (;;) {
            uint32_t t = lane == 0 ? atomicAdd(&s_next, 1u) : 0u;
            t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
            if (t >= VARS || var0 + t >= n_var) return false;
            f.var = var0 + t;
            f.src = vplanes + f.var * sw;
            uint32_t m = 0, h = 0, a = 0;               // the calls among the valid positions
            for (uint32_t w = lane; w < sw; w += 64u) {
                const uint32_t ok = valid[w];
                h += __builtin_popcount(f.src[w] & ok);
                m += __builtin_popcount(f.src[plane_words + w] & ok);
                a += __builtin_popcount(f.src[2u * plane_words + w] & ok);
            }
            f.m = wave_sum(m), f.h = wave_sum(h), f.a = wave_sum(a);
            f.mean = f.m ? ((double)f.h + 2.0 * (double)f.a) / (double)f.m : 0.0;
            const uint32_t classes = (f.m > f.h + f.a) + (f.h > 0u) + (f.a > 0u);
            f.status = f.m == 0u ? HHGT_LOGIT_NO_CALL : classes < 2u ? HHGT_LOGIT_ONE_CLASS : HHGT_LOGIT_TESTED;
            f.steps = 0, f.last = false, f.hinv = f.u0 = f.hinv0 = nan;
            if (f.status == HHGT_LOGIT_TESTED) break;
            store_record(out, f, nan, lane);
        }
#pragma unroll
        for (uint32_t j = 0; j < XCOLS; ++j) theta[j] = j < q ? beta0[j] : 0.0;
        theta[G] = 0.0;
        return true;
    };
    bool running = draw();

    for (;;) {
        __syncthreads();                                 // (the previous round's flag has been read)
        if (threadIdx.x == 0) s_running = 0;
        __syncthreads();
        if (running && lane == 0) s_running = 1;
        __syncthreads();
        if (!s_running) break;

        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (uint32_t w0 = 0; w0 < sw; w0 += SLICE) {
            __syncthreads();                             // the previous slice has been read
            for (uint32_t item = threadIdx.x; item < POS * q; item += 64u * WAVES) {
                const uint32_t p = item / q, j = item - p * q;
                const uint32_t word = w0 + (p >> 5);
                const bool on = word < sw && ((valid[word < sw ? word : 0u] >> (p & 31u)) & 1u);
                s_x[j * XSTRIDE + p] = on ? x[(32ull * w0 + p) * q + j] : 0.0;
            }
            __syncthreads();
            if (!running) continue;                      // (the barriers stand outside: every wave meets them)
#pragma unroll 1
            for (uint32_t blk = 0; blk < POS / 64u; ++blk) {
                // a lane for a position: lane 16 k + t takes 4 t + k, the position of step t for the lanes of its row
                const uint32_t word = w0 + 2u * blk + (spot >> 5), bit = spot & 31u;
                const bool in = word < sw;
                const uint32_t wi = in ? word : 0u;
                const bool on = in && ((valid[wi] >> bit) & 1u);
                const uint32_t het = (f.src[wi] >> bit) & 1u, comp = (f.src[plane_words + wi] >> bit) & 1u,
                               alt = (f.src[2u * plane_words + wi] >> bit) & 1u;
                const double g = !on ? 0.0 : comp ? (double)(het + 2u * alt) : f.mean;
                const double yv = on ? y[32ull * wi + bit] : 0.0;
                double eta = 0.0;
#pragma unroll
                for (uint32_t j = 0; j < XCOLS; ++j) eta = fma(s_x[j * XSTRIDE + 64u * blk + spot], theta[j], eta);
                eta = fma(g, theta[G], eta);
                const double mu = 1.0 / (1.0 + exp(-eta));
                const double w = on ? mu * (1.0 - mu) : 0.0, r = on ? yv - mu : 0.0;
                // a lane for a row of [X | g], a column of [w X | w g | y - mu] and one position in four
                tile_steps(std::make_integer_sequence<uint32_t, 16>{}, acc, w, r, g,
                           s_x + (row < XCOLS ? row : 0u) * XSTRIDE + 64u * blk + k, row);
            }
        }
        if (!running) continue;

        const Solved s = solve_tile(acc, s_tile[wave], lane, q);
        bool done = false;
        if (!s.ok) {
            f.status = f.steps == 0 && !f.last ? HHGT_LOGIT_COLLINEAR : HHGT_LOGIT_NOT_CONVERGED;
            done = true;
        } else if (f.last) {
            f.hinv = s.hinv;
            done = true;
        } else {
            if (f.steps == 0) f.u0 = s.u_g, f.hinv0 = s.hinv;
            double biggest = 0.0;
#pragma unroll
            for (uint32_t j = 0; j < HHGT_LOGIT_MAX_COLS; ++j) {
                theta[j] += s.delta[j];
                biggest = fmax(biggest, fabs(s.delta[j]));
            }
            ++f.steps;
            if (biggest <= 1e-8) {
                f.last = true;
            } else if (f.steps == HHGT_LOGIT_MAX_STEPS || !(biggest < __longlong_as_double(0x7ff0000000000000ll))) {
                f.status = HHGT_LOGIT_NOT_CONVERGED;
                done = true;
            }
        }
        if (done) {
            store_record(out, f, theta[G], lane);
            running = draw();
        }
    }
}

int launch_logistic_fit(const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, const uint32_t *d_valid, const double *d_x,
                        uint32_t q, const double *d_y, const double *d_beta0, double *d_out, hipStream_t st)
{
    if (n_var == 0) return HHGT_OK;
    const uint64_t blocks = (n_var + VARS - 1u) / VARS;
    if (blocks > 0x7fffffffull || sw >= (1ull << 27) || q < 1u || q > XCOLS) {
        hhgt_set_error("logistic_fit: %llu variants of %llu words, %u columns of X (at most %llu variants, 2^27 - 1 words, 1 to %u "
                       "columns)", (unsigned long long)n_var, (unsigned long long)sw, q, 0x7fffffffull * VARS, XCOLS);
        return HHGT_ERR_ARG;
    }
    hipLaunchKernelGGL(k_logistic_fit, dim3((uint32_t)blocks), dim3(64 * WAVES), 0, st, d_vplanes, n_var, (uint32_t)sw, d_valid,
                       d_x, q, d_y, d_beta0, d_out);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
