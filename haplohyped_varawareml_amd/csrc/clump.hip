// LD clumping from link bits (hhgt_ld_clump; include/hhgt.h has the rule and the contract; hhgt_ld_decisions, which makes the
// bits, sits beside k_ld_exceeds in ld.hip).  The greedy walk in p-value order is the lexicographically first maximal
// independent set of the link graph among the eligible variants: variant k is an index iff it is eligible and no linked
// eligible variant of lower rank is one.  Three kinds of launch: the blockers of every variant, rounds over double-buffered
// state, the owners.  No workgroup waits for another: a round is a launch.
#include "common.h"

enum : uint8_t { UNDECIDED = 0, INDEX = 1, NOT_INDEX = 2 };

// one wave per (variant k, word q): lane l stands for the distance d = 64 q + l on either side.  Back: bit d of bits[k] is
// the pair (k - 1 - d, k); forward: the pair (k, k + 1 + d) is bit d of bits[k + 1 + d] — the transposition, gathered here
// once (lane l reads word q of another variant each).  A blocker is a linked neighbour that is eligible and of lower rank;
// equal ranks block neither way.  Three ballots leave as fwd[k][q], blk[k][q] (back) and blk[k][nq + q] (forward); the wave
// of word 0 also sets the variant's first state.
__global__ __launch_bounds__(256) void k_clump_blockers(const uint64_t *__restrict__ bits, uint32_t n_var, uint32_t window,
                                                        uint32_t nq, const uint32_t *__restrict__ rank,
                                                        const uint8_t *__restrict__ eligible, uint64_t *__restrict__ fwd,
                                                        uint64_t *__restrict__ blk, uint8_t *__restrict__ state)
{
    const uint64_t unit = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (unit >= (uint64_t)n_var * nq) return;
    const uint32_t k = (uint32_t)(unit / nq), q = (uint32_t)(unit % nq), lane = threadIdx.x & 63u, d = q * 64u + lane;
    const uint32_t mine = rank[k];
    bool back = false, link = false, ahead = false;
    if (d < window && k >= d + 1u && ((bits[unit] >> lane) & 1ull)) {
        const uint32_t u = k - 1u - d;
        back = eligible[u] != 0 && rank[u] < mine;
    }
    if (d < window && (uint64_t)k + 1u + d < n_var) {
        const uint32_t v = k + 1u + d;
        link = (bits[(uint64_t)v * nq + q] >> lane) & 1ull;
        ahead = link && eligible[v] != 0 && rank[v] < mine;
    }
    const uint64_t b = __ballot(back), f = __ballot(link), a = __ballot(ahead);
    if (lane == 0u) {
        fwd[unit] = f;
        blk[(uint64_t)k * 2u * nq + q] = b;
        blk[(uint64_t)k * 2u * nq + nq + q] = a;
        if (q == 0u) state[k] = eligible[k] != 0 ? UNDECIDED : NOT_INDEX;
    }
}

// the neighbour that bit `bit` of word j of a variant's 2 nq words (nq back, nq forward) stands for
__device__ __forceinline__ uint32_t clump_neighbour(uint32_t k, uint32_t j, uint32_t nq, uint32_t bit)
{
    return j < nq ? k - 1u - (j * 64u + bit) : k + 1u + ((j - nq) * 64u + bit);
}

// the lanes of a group of LPV consecutive lanes, as a mask over the wave
template <uint32_t LPV> __device__ __forceinline__ uint64_t group_mask(uint32_t lane)
{
    return ((1ull << LPV) - 1ull) << (lane & ~(LPV - 1u));
}

// one round: LPV lanes per variant (the power of two >= 2 nq, at most 32), 256 / LPV variants per workgroup.  Lane j of an
// undecided variant walks the set bits of blocker word j and reads those neighbours' states of the previous round; the
// group's verdict is two ballots.  Every variant's state is written to `next`, decided ones unchanged.  The variants a
// wave decided are counted in one atomic add (a vector atomic) to the round's counter.
template <uint32_t LPV>
__global__ __launch_bounds__(256) void k_clump_round(const uint64_t *__restrict__ blk, uint32_t n_var, uint32_t nq,
                                                     const uint8_t *__restrict__ prev, uint8_t *__restrict__ next,
                                                     uint32_t *__restrict__ counter)
{
    const uint64_t kk = (uint64_t)blockIdx.x * (256u / LPV) + threadIdx.x / LPV;
    const uint32_t k = (uint32_t)kk, j = threadIdx.x % LPV, lane = threadIdx.x & 63u;
    const bool live = kk < n_var;
    const uint8_t s = live ? prev[k] : (uint8_t)NOT_INDEX;
    bool index = false, wait = false;
    if (s == UNDECIDED && j < 2u * nq) {
        uint64_t w = blk[(uint64_t)k * 2u * nq + j];
        while (w) {
            const uint8_t t = prev[clump_neighbour(k, j, nq, (uint32_t)__builtin_ctzll(w))];
            w &= w - 1ull;
            index |= t == INDEX;
            wait |= t == UNDECIDED;
        }
    }
    const uint64_t g = group_mask<LPV>(lane);
    const bool any_index = __ballot(index) & g, any_wait = __ballot(wait) & g;
    const uint8_t now = s != UNDECIDED ? s : any_index ? (uint8_t)NOT_INDEX : any_wait ? (uint8_t)UNDECIDED : (uint8_t)INDEX;
    const bool leader = live && j == 0u;
    if (leader) next[k] = now;
    const uint32_t decided = (uint32_t)__popcll(__ballot(leader && s == UNDECIDED && now != UNDECIDED));
    if (lane == 0u && decided) atomicAdd(counter, decided);
}

__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// the owners, in the same shape: lane j walks word j of ALL links of its variant (bits[k] back, fwd[k] forward) and keeps
// the index of lowest (rank, offset) among them; the group's minimum is the owner of a variant that is no index itself
template <uint32_t LPV>
__global__ __launch_bounds__(256) void k_clump_owners(const uint64_t *__restrict__ bits, const uint64_t *__restrict__ fwd,
                                                      uint32_t n_var, uint32_t window, uint32_t nq,
                                                      const uint32_t *__restrict__ rank, const uint8_t *__restrict__ state,
                                                      int32_t *__restrict__ owner)
{
    const uint64_t kk = (uint64_t)blockIdx.x * (256u / LPV) + threadIdx.x / LPV;
    const uint32_t k = (uint32_t)kk, j = threadIdx.x % LPV;
    const bool live = kk < n_var;
    const uint8_t s = live ? state[k] : (uint8_t)INDEX;
    uint64_t best = ~0ull;
    if (s != INDEX && j < 2u * nq) {
        uint64_t w = j < nq ? bits[(uint64_t)k * nq + j] : fwd[(uint64_t)k * nq + (j - nq)];
        while (w) {
            const uint32_t bit = (uint32_t)__builtin_ctzll(w);
            w &= w - 1ull;
            if (j < nq && (j * 64u + bit >= window || j * 64u + bit + 1u > k)) continue;     // past the window, before variant 0
            const uint32_t nb = clump_neighbour(k, j, nq, bit);
            if (state[nb] == INDEX) best = umin64(best, ((uint64_t)rank[nb] << 32) | nb);
        }
    }
#pragma unroll
    for (uint32_t o = LPV / 2u; o > 0u; o /= 2u) best = umin64(best, (uint64_t)__shfl_xor((unsigned long long)best, (int)o));
    if (live && j == 0u) owner[k] = s == INDEX ? (int32_t)k : best == ~0ull ? -1 : (int32_t)(uint32_t)best;
}

static uint32_t clump_words(uint32_t window) { return (window + 63u) / 64u; }

// lanes per variant: the power of two >= 2 nq (2 .. 32)
static uint32_t clump_lanes(uint32_t nq)
{
    uint32_t lpv = 2;
    while (lpv < 2u * nq) lpv *= 2u;
    return lpv;
}

int launch_clump_blockers(const uint64_t *d_bits, uint64_t n_var, uint32_t window, const uint32_t *d_rank, const uint8_t *d_eligible,
                          const ClumpWs &ws, hipStream_t st)
{
    const uint32_t nq = clump_words(window);
    const uint64_t blocks = (n_var * nq + 3u) / 4u;
    if (n_var > 0x7fffffffull || blocks > 0x7fffffffull) {
        hhgt_set_error("ld_clump: %llu variants at window %u (at most 2^31 - 1 variants, 2^33 link words)",
                       (unsigned long long)n_var, window);
        return HHGT_ERR_ARG;
    }
    hipLaunchKernelGGL(k_clump_blockers, dim3((uint32_t)blocks), dim3(256), 0, st, d_bits, (uint32_t)n_var, window, nq, d_rank,
                       d_eligible, ws.fwd, ws.blk, ws.state[0]);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

// (n_var < 2^31 and at least 8 variants per workgroup: the grids below fit)
int launch_clump_round(uint64_t n_var, uint32_t window, const ClumpWs &ws, uint32_t from, uint32_t *d_counter, hipStream_t st)
{
    const uint32_t nq = clump_words(window), lpv = clump_lanes(nq), grid = (uint32_t)((n_var + 256u / lpv - 1u) / (256u / lpv));
    void (*round)(const uint64_t *, uint32_t, uint32_t, const uint8_t *, uint8_t *, uint32_t *) = nullptr;
    switch (lpv) {
    case 2: round = k_clump_round<2>; break;
    case 4: round = k_clump_round<4>; break;
    case 8: round = k_clump_round<8>; break;
    case 16: round = k_clump_round<16>; break;
    default: round = k_clump_round<32>; break;
    }
    hipLaunchKernelGGL(round, dim3(grid), dim3(256), 0, st, ws.blk, (uint32_t)n_var, nq, ws.state[from], ws.state[from ^ 1u], d_counter);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

int launch_clump_owners(const uint64_t *d_bits, uint64_t n_var, uint32_t window, const uint32_t *d_rank, const ClumpWs &ws,
                        uint32_t from, int32_t *d_owner, hipStream_t st)
{
    const uint32_t nq = clump_words(window), lpv = clump_lanes(nq), grid = (uint32_t)((n_var + 256u / lpv - 1u) / (256u / lpv));
    void (*owners)(const uint64_t *, const uint64_t *, uint32_t, uint32_t, uint32_t, const uint32_t *, const uint8_t *, int32_t *) = nullptr;
    switch (lpv) {
    case 2: owners = k_clump_owners<2>; break;
    case 4: owners = k_clump_owners<4>; break;
    case 8: owners = k_clump_owners<8>; break;
    case 16: owners = k_clump_owners<16>; break;
    default: owners = k_clump_owners<32>; break;
    }
    hipLaunchKernelGGL(owners, dim3(grid), dim3(256), 0, st, d_bits, ws.fwd, (uint32_t)n_var, window, nq, d_rank, ws.state[from],
                       d_owner);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
