// lz4bits.hip — LZ4 block encode of 0/1 byte planes by walking the ONES, not the bytes (gfx950).
//
// Same place in the path as lz4.hip (the shuffle + LZ4 step of the HDF5 filter the reference invokes at
// /root/reference/src/haplohyped/vcf_to_h5.py:134-135), same output contract (a valid LZ4 block stream per Blosc
// stream, "decompresses to identical bytes"), for the case the path is built for: typesize 2, 8 KiB Blosc blocks,
// i.e. two 4 KiB byte planes per block, each the haplotype of one sample over 4096 variants — bytes that are 0 or 1
// and about 94 % zeros.  The byte-wise encoder in lz4.hip spends ~3.8 k vector + ~3.3 k scalar instructions per plane
// looking at every one of the 4096 positions (64 per window, one per lane); it is bound by instruction issue with HBM
// at 6 %.  This kernel turns the plane into a 4096-bit map and works on the LIST OF ONES (~260 per plane):
//
//   * one lane per one, 64 ones per window (4-5 windows per plane instead of 52-64);
//   * candidate table keyed on the GAP behind the one (distance to the next one, clipped to 40: 64 entries, no hash),
//     updated by ONE ds_wrxchg_rtn_b32 per window: the LDS serves lanes that hit the same address in ascending lane
//     order (tools/micro/lds_xchg_order.hip, checked by a test), so every lane gets the most recent earlier one with its
//     key — exact sequential table semantics, 64 insertions at once.  (The first version keyed the table on the 12 bits
//     at the one, LZ4's habit; on these planes that context is "a one and eleven zeros" nearly everywhere.  An equal
//     first gap is what a match of ones needs to get past its first step: ratio 5.31 -> 5.86 at two candidates.)
//   * match lengths come from comparing GAPS between ones, not bytes: equal gaps, then one plus the shorter of the
//     first unequal pair.  The gaps also exist as BYTES (clipped to 255), so a candidate is judged by one unaligned
//     4-byte fetch, an xor and a count-trailing-zeros (three gaps + the open one); the longest agreement along the chain
//     wins — the zeros the two have in common IN FRONT count as well: a match is pulled back over them (up to 64) —
//     (picking by length packs tighter than picking by the local saving: the parse is greedy) and only the winner
//     is worked out exactly from the positions, extended past the third gap where it still agrees, pulled back over
//     the zeros in front, and priced;
//   * every one decides locally between "match" and "literal" by cost (3 bytes per sequence against the literals and
//     runs it replaces) and thereby where the next coded one is: the greedy parse is a linked list nxt(j), followed
//     inside a window by pointer doubling (6 rounds), not by a serial loop;
//   * behind whatever a coded one ends with, the zeros up to the next one go out as an offset-1 run — if there are
//     four that the NEXT coded one's match does not pull back over anyway (decided at layout time, where the next
//     coded one is the neighbouring queue entry; round 3: run rule and an 8-zero pull-back that knew nothing of
//     each other packed 8 % looser with the same candidates);
//   * every coded one lays out and writes its (at most two) sequences itself, literals generated from the bit map.
//
// tools/sim/gapenc_ref.c states the same algorithm on the CPU, decision for decision; the kernel's streams are
// compared with it byte for byte (tests/test_gpu_lz4_bitplanes.py) and decoded by liblz4 / the oracle like every
// other stream.  Planes of bit-plane input that hold missing calls are coded by the exception-aware path of
// k_lz4_bitplanes_uni.  Planes neither path can code (a call beyond 0 / 1 / missing, int8 input with a byte > 1, too
// many ones) are left to the byte-wise encoder (csize = MARK; lz4.hip's kernel then runs in "marked streams only" mode).
#include "common.h"

#define BP_N 4096
#ifndef BP_MAXONES
#define BP_MAXONES 636
#endif
// Queue and staging area are what is left of 5120 bytes of LDS per plane — 32 single-wave workgroups of k_lz4_bitplanes_uni
// per CU, eight waves per SIMD — behind the arrays whose sizes the coder's decisions hang on: 896 bytes on the plain path,
// 760 on the exception-aware one, which carries a second bit map and the ones' classes (624 bytes) and a shorter list.
// Neither size changes a stream: a window whose coded ones would not fit sends a batch off first, staged bytes leave
// when the next batch would not fit, and a batch larger than the whole area goes to the stream's slot directly.
// (DESIGN.md 3.2 "One plane per workgroup" has the stage times of the splits that were tried.)
#ifndef BP_QCAP
#define BP_QCAP 80      // queued coded ones a wave can hold (a window adds at most 64 to at most 64)
#endif
#ifndef BP_STAGE
#define BP_STAGE 240    // staging area
#endif
#ifndef BP_WAVES
#define BP_WAVES 7       // waves per SIMD the kernels are compiled for (k_lz4_bitplanes: LDS must allow 2 x BP_WAVES workgroups per CU)
#endif
#ifndef BP_MAXONES_EXC
#define BP_MAXONES_EXC 540
#endif
#ifndef BP_QCAP_EXC
#define BP_QCAP_EXC 80
#endif
#ifndef BP_STAGE_EXC
#define BP_STAGE_EXC 104
#endif
#define BP_SPARE 8          // bytes in front of the staging area that nobody reads
#define BP_PLANE_LDS 5120   // k_lz4_bitplanes_uni: LDS of a workgroup = a plane (163 840 / 32)
template <bool EXC> struct BpCfg {
    static constexpr uint32_t MAXONES = EXC ? BP_MAXONES_EXC : BP_MAXONES;
    static constexpr uint32_t QCAP = EXC ? BP_QCAP_EXC : BP_QCAP;
    static constexpr uint32_t STAGE = EXC ? BP_STAGE_EXC : BP_STAGE;
    static constexpr uint32_t PTRASH = MAXONES + 7;   // P's spare entry: written by lanes that have nothing to store, never read
};
static_assert(BP_QCAP >= 65 && BP_QCAP_EXC >= 65, "a batch of 64 needs the entry behind it in the queue");
static_assert(BP_SPARE >= 6 && BP_SPARE % 4 == 0, "store k of an entry (k < 6) has spare byte k; the staged bytes behind them leave as dwords");
#define BP_HLOG 6
#define BP_GAPCLIP 40
#define BP_MINM 6     // total length a hash match must have
#define BP_TMIN 4     // zeros an offset-1 run must cover to be worth its 3 bytes
#define BP_BACK 64    // zeros in front of the one a match is pulled back over (round 2: 8)
#define BP_STEPS 16   // exact extension of the chosen candidate
#define BP_PICK 3     // full gaps the pick looks at (one dword of gap bytes)
#define BP_LAZY_MIN 3 // LAZY: bytes the next one's match must reach further, on top of what giving up costs
#ifdef BP_MARKS   // development: section markers in the ISA listing (hipcc -S -DBP_MARKS), tools/isa_sections.py counts per section
#define BP_MARK(name) asm volatile("; ==MARK " name)
#else
#define BP_MARK(name)
#endif
#ifndef BP_SKIP
#define BP_SKIP 0   // development: 1 no emission, 2 no layout either, 3 no selection, 4 no window loop, 5 phase A only, 6 plane input: load + bit map only (invalid output; timing only)
#endif
#define BP_EMPTY_BYTES 26u   // the stream of a plane of 4096 zeros (k_lz4_bitplanes_uni writes it itself)
#define BP_MFLIMIT (BP_N - 12)
#define BP_MATCHLIMIT (BP_N - 5)

template <bool CHAIN, bool EXC> struct BpLds {
    uint32_t bm[132];                // bit map of the plane's nonzero bytes: 128 dwords + zero padding
    uint32_t xm[EXC ? 132 : 1];      // EXC: which of them are 0xF7 (missing calls)
    uint32_t cls[EXC ? 24 : 1];      // EXC: the same per ONE: bit i = the one with P-index i is a missing call
    uint32_t tab[1 << BP_HLOG];      // min(gap behind the one + 1, BP_GAPCLIP) -> one index + 1
    uint8_t flag[72];                // pointer-doubling marks of a window ([0, 64]; [68]: where lanes with nothing to mark write)
    uint16_t wpre[64];               // ones in front of bit-map word w (64-bit words)
    uint16_t P[BpCfg<EXC>::MAXONES + 8];      // P[j + 1] = q_j + 1 (P[0] = 0: a virtual one at -1; P[m + 1] = P[m + 2] = n + 1)
    uint16_t chain[CHAIN ? BpCfg<EXC>::MAXONES + 8 : 4];   // chain[j + 1] = (previous one with the same context hash) + 1, 0 = none
    uint32_t gbw[(BpCfg<EXC>::MAXONES + 16) / 4];   // gap bytes: zeros behind the one with P-index i, clipped to 255 (255 from the last one on)
    uint2 queue[BpCfg<EXC>::QCAP + 1];       // coded ones waiting for layout + emission (bp_emit_batch takes 64 at a time); [QCAP]: written by lanes that queue nothing
    uint8_t stage[BP_SPARE + BpCfg<EXC>::STAGE];   // [0, BP_SPARE): written by lanes that have no byte to store (store k of an entry: byte k); behind them the output staged, written out in coalesced dwords
};

// a queued coded one: what its sequences need that does not depend on the sequences in front of it
//   x: E (13 bits) | msr = q - nb (13) << 13 | (rs - E) << 26 | onM << 30 | onT << 31        (E: end of what the one codes;
//      onT: the run is long enough — whether it is emitted is decided against the next entry, bp_emit_batch.  The two on
//      top: "this one queues something" is x >= BP_ENT_ANY, one compare whose result is the lane mask; onT is the sign.
//      msr and off mean something only with onM)
//   y: re (13 bits) | off << 13                                                                (re: start of the next coded one)
#define BP_ENT_ANY (1u << 30)
__device__ __forceinline__ uint2 bp_entry(uint32_t E, uint32_t msr, bool onM, bool onT, uint32_t rs, uint32_t re, uint32_t off)
{
    return make_uint2(E | ((msr & 0x1FFFu) << 13) | ((rs - E) << 26) | (onM ? 1u << 30 : 0u) | (onT ? 1u << 31 : 0u), re | (off << 13));
}

// 32 bits of the map starting at bit q (0 <= q < 4096 + 96)
__device__ __forceinline__ uint32_t bp_bits(const uint32_t *bm, uint32_t q)
{
    const uint32_t i = q >> 5;
    const uint32_t lo = bm[i], hi = bm[i + 1];
    return __builtin_amdgcn_alignbit(hi, lo, q & 31u);
}

// four gap bytes starting at byte i of the gap array (two aligned dwords, one funnel shift)
__device__ __forceinline__ uint32_t bp_gap4(const uint32_t *gbw, uint32_t i)
{
    const uint32_t w = i >> 2;
    return __builtin_amdgcn_alignbit(gbw[w + 1u], gbw[w], (i & 3u) << 3);
}

// extension bytes of an LZ4 length field: x >= 15 ? (x - 15) / 255 + 1 : 0 = (x + 240) / 255 for every x; the division as
// a 24-bit multiply and a shift (exact below 65536; the compiler's v_mul_hi_u32 runs at a quarter of the rate, and the
// kernel evaluates this eight times per window)
__device__ __forceinline__ uint32_t bp_len_ext(uint32_t x) { return __umul24(x + 240u, 32897u) >> 23; }

// a pair (one's side, candidate's side) of values below 65536 in the halves of one register: positions P[...] <= BP_N + 1, gaps
// and lengths <= BP_N.  One v_pk_* instruction works on both, an SDWA compare or minimum takes its two sides from the halves.
// (Built from two 16-bit LDS loads by one v_perm_b32: the compiler does not load into halves — ds_read_u16_d16 / _d16_hi — here,
// and it turns this shift-and-or into the permute whatever is done to hide it; DESIGN.md 3.2 "Pairs in 16-bit halves".)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 bp_pair(uint16_t a, uint16_t b)
{
    return __builtin_bit_cast(u16x2, (uint32_t)a | ((uint32_t)b << 16));
}

#define BP_FENCE() asm volatile("" ::: "memory")
// the compiler forgets what it knows about x, at no fixed place in the order of things (it may move this, and drop it with x)
#define BP_HIDE(x) asm("" : "+v"(x))
// literal bytes of positions whose map bits are b (and, EXC, whose missing-call bits are x): 0, 1 or 0xF7
template <bool EXC> __device__ __forceinline__ uint32_t bp_lit(uint32_t b, uint32_t x, uint32_t k)
{
    const uint32_t v = (b >> k) & 1u;
    if (!EXC) return v;
    // (a missing call's bit in x stands on a bit of b, the map of the nonzero bytes: 1 + 0xF6, one multiply-add behind the
    // v_bfe_u32 that BP_HIDE holds the compiler to)
    uint32_t e = (x >> k) & 1u;
    BP_HIDE(e);
    return __umul24(e, 0xF6u) + v;
}

// the compiler forgets what it knows about x: what was derived from x in front of this point is worked out again behind it,
// not carried in registers across (the length fields' extension counts across the size scan of a batch)
#define BP_FORGET(x) asm volatile("" : "+v"(x))
#ifndef BP_EMITSKIP
#define BP_EMITSKIP 0   // development (timing only, invalid streams): 1 no literal bytes, 2 no long literal runs, 3 no sequence bytes at all
#endif
// the (at most two) sequences of one queue entry, in one pass.  The FIRST is the match M (onM) or, without one, the run T:
// literals [pe, s1) generated from the bit map — the only literal run of an entry that needs it — then (len1, off1).  The
// SECOND is the run T behind a match: its literals are [E, rs), none or one byte, and that byte is a zero (a run is only
// queued over >= BP_TMIN zeros up to the next nonzero byte at or behind E, so byte E is none; tools/sim/gapenc_ref.c's
// last loop, where prev_end = e behind a match): token, the constant 0, the offset bytes 1, 0, and the length.
// OUT is the staging area (S.stage; LDS: ds_write_b8) or, for a batch too large for it, a pointer into the stream's slot in
// global memory.  TR (staging area only): out[0 .. BP_SPARE) are bytes nobody reads — lanes with nothing to store write there
// instead of sitting out an exec-mask region: `if (p) store` costs two scalar instructions and often a branch, `store at
// (p ? a : 0)` one vector select with an inline constant, and a wave pays for its branch points.
// at: where the entry's bytes start in out (staged: BP_SPARE and the batch's place in the area are in it, added once per entry
// and not to each store's address); pe: where its literals start in the plane; (on1, ll1, ml1 = length - 4, off1): the
// first sequence; (on2, lit2: it has its one literal, ml2): the second.  The counts of extension bytes are worked out here
// again, not handed over from the caller's size scan (BP_FORGET there): three multiplies against three registers.
// (Up to round 8 a batch called bp_put_seq twice, for M and for T, each with its own fetch from the bit map behind its own
// `any literals?` ballot, its own rare-length branch and its own long-literal loop: profiles/r09_emit_split.txt.)
template <bool EXC, bool TR, typename OUT>
__device__ __forceinline__ void bp_put_entry(const uint32_t *bm, const uint32_t *xm, OUT out, uint32_t at, uint32_t pe, bool on1, uint32_t ll1, uint32_t ml1,
                                             uint32_t off1, bool on2, bool lit2, uint32_t ml2, uint32_t lane)
{
    if (BP_EMITSKIP == 3) return;
    const uint32_t llx1 = bp_len_ext(ll1), mlx1 = on1 ? bp_len_ext(ml1) : 0u, mlx2 = on2 ? bp_len_ext(ml2) : 0u, ll2 = lit2 ? 1u : 0u;
    // byte v to out[a + k], k a constant, if p.  Staged: the select picks a or 0, and + k rides in the store's offset field —
    // a lane with nothing to store writes spare byte k (behind BP_HIDE: or the compiler adds k in front of the select, one
    // v_add per store)
    auto put = [&](bool p, uint32_t a, uint32_t k, uint32_t v) {
        if (TR) {
            uint32_t i = p ? a : 0u;
            BP_HIDE(i);
            out[i + k] = (uint8_t)v;
        } else if (p) out[a + k] = (uint8_t)v;
    };
    // the same for two neighbouring bytes under one predicate: one select (spare bytes 0, 1)
    auto put2 = [&](bool p, uint32_t a, uint32_t v0, uint32_t v1) {
        if (TR) {
            uint32_t i = p ? a : 0u;
            BP_HIDE(i);
            out[i] = (uint8_t)v0;
            out[i + 1u] = (uint8_t)v1;
        } else if (p) {
            out[a] = (uint8_t)v0;
            out[a + 1u] = (uint8_t)v1;
        }
    };
    const uint32_t lit = at + 1u + llx1, o1 = lit + ll1;       // first sequence: its literals, its offset
    const uint32_t at2 = o1 + 2u + mlx1, o2 = at2 + 1u + ll2;  // second sequence: its token, its offset
    // ONE wave-uniform branch, over both sequences, for lengths that need more than one extension byte (>= 270) ...
    // (in front of the straight-line stores and the second sequence in front of the first: every value dies with its last
    // store, the literals' three stay — the other way round the kernel takes 72 registers instead of 70)
    if (__builtin_expect(__builtin_amdgcn_ballot_w64((llx1 > 1u) | (mlx1 > 1u) | (mlx2 > 1u)) != 0ull, 0)) {   // (rare)
        auto more = [&](uint32_t a, uint32_t v, uint32_t nx) {   // extension bytes 1 .. nx - 1 of the length v, at a + 1 ...
            uint32_t r = v - 15u - 255u;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (uint32_t k = 1; k < nx; ++k) {
                out[a + k] = (uint8_t)(k + 1u == nx ? r : 255u);
                r -= 255u;
            }
        };
        more(at + 1u, ll1, llx1);
        more(o1 + 2u, ml1, mlx1);
        more(o2 + 2u, ml2, mlx2);
    }
    // ... and straight-line byte stores for what nearly every sequence has: token, at most one extension byte per length,
    // offset
    put(on2, at2, 0u, (ll2 << 4) | (ml2 < 15u ? ml2 : 15u));
    put(lit2, at2, 1u, 0u);
    put2(on2, o2, 1u, 0u);
    put(mlx2 != 0u, o2, 2u, mlx2 == 1u ? ml2 - 15u : 255u);
    put(on1, at, 0u, ((ll1 < 15u ? ll1 : 15u) << 4) | (ml1 < 15u ? ml1 : 15u));
    put(llx1 != 0u, at, 1u, llx1 == 1u ? ll1 - 15u : 255u);
    put2(on1, o1, off1, off1 >> 8);
    put(mlx1 != 0u, o1, 2u, mlx1 == 1u ? ml1 - 15u : 255u);
    // Most literal runs are 1-3 bytes ("1", "1 0"): up to 6 go out as byte stores of the owning lane.  Longer runs (the
    // literals of all the ones in between that code nothing pile up in front of the next sequence) are written by the whole
    // wave, one run at a time — a lockstep per-lane loop would run max(ll) times for all.
    if (BP_EMITSKIP != 1) {
        const uint32_t b = bp_bits(bm, pe), x = EXC ? bp_bits(xm, pe) : 0u;   // the entry's ONE fetch from the bit map
        uint32_t nsm = ll1 <= 6u ? ll1 : 0u;   // bytes this lane stores itself
        BP_HIDE(nsm);                          // (one number for the six compares, not a compare of ll1 per byte)
#pragma unroll
        for (uint32_t k = 0; k < 6u; ++k) {
            uint32_t v = bp_lit<EXC>(b, x, k);
            // (staged: the byte stays 32 bits wide up to the store, bit k is one v_bfe_u32; left to itself the compiler narrows it
            // to a 16-bit shift and a mask.  Not so in the direct form: the int8 kernel goes from 64 to 66 VGPRs with it)
            if (TR) BP_HIDE(v);
            put(k < nsm, lit, k, v);
        }
        unsigned long long big = BP_EMITSKIP == 2 ? 0ull : __builtin_amdgcn_ballot_w64(ll1 > 6u);
        while (big != 0ull) {
            const int l = __builtin_ctzll(big);
            big &= big - 1ull;
            const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)ll1, l);
            const uint32_t src = (uint32_t)__builtin_amdgcn_readlane((int)pe, l);
            const uint32_t dst = (uint32_t)__builtin_amdgcn_readlane((int)lit, l);
            for (uint32_t k = lane; k < n; k += 64u) out[dst + k] = (uint8_t)bp_lit<EXC>(bp_bits(bm, src + k), EXC ? bp_bits(xm, src + k) : 0u, 0u);
        }
    }
}

// staged bytes [0, n) -> global, whole dwords coalesced, the last 1-3 bytes singly
__device__ __forceinline__ void bp_flush(const uint8_t *stage, uint8_t *__restrict__ dst, uint32_t n, uint32_t lane)
{
    struct __attribute__((packed)) PU32 {
        uint32_t v;
    };
    const uint32_t nd = n >> 2;
    for (uint32_t i = lane; i < nd; i += 64u) reinterpret_cast<PU32 *>(dst + 4u * i)->v = reinterpret_cast<const uint32_t *>(stage)[i];
    const uint32_t t = (nd << 2) + lane;
    if (t < n) dst[t] = stage[t];
}

// layout + emission of the first n (<= 64) of the qn queued coded ones, one per lane, in stream order (n < qn unless the
// stream ends with entry n - 1: every entry sees its successor).  The end of a coded one's last sequence is where the
// next one's literals start (pe): the neighbouring lane's value, no scan.
struct BpOut {
    uint32_t prev_end, gop, sop;   // end of the last sequence; bytes written to global / staged
};   // (by value: a reference across the "memory" fences would pin the counters to scratch memory)

template <bool EXC, typename LDS>
__device__ __forceinline__ BpOut bp_emit_batch(LDS &S, const uint32_t *bm, uint8_t *__restrict__ out, uint32_t n, uint32_t qn, BpOut st, uint32_t lane)
{
    const uint32_t *xm = S.xm;
    uint32_t prev_end = st.prev_end, gop = st.gop, sop = st.sop;
    const bool have = lane < n;
    uint2 en = S.queue[lane];   // (lane < 64 <= QCAP: inside the queue whatever n is)
    en.x = have ? en.x : 0u;
    en.y = have ? en.y : 0u;
    const uint32_t E = en.x & 0x1FFFu, msr = (en.x >> 13) & 0x1FFFu, rs = E + ((en.x >> 26) & 1u), re = en.y & 0x1FFFu, off = en.y >> 13;
    const bool onM = (en.x >> 30) & 1u;
    bool onT = (int)en.x < 0;
    {   // the run is dropped when the next coded one's match starts so far in front of its one that fewer than BP_TMIN
        // zeros are left to the run (the next coded one with a match IS the next entry: msr <= re says so)
        uint32_t nx = S.queue[lane + 1u].x;
        nx = lane + 1u < qn ? nx : 0u;
        const uint32_t nmsr = (nx >> 13) & 0x1FFFu;
        const bool nM = (nx >> 30) & 1u;
        uint32_t nbk = nM && nmsr <= re ? re - nmsr : 0u;
        const uint32_t zt = re - rs;
        nbk = nbk < zt ? nbk : zt;
        onT = onT && zt - nbk >= BP_TMIN;
    }
    // end of this one's last sequence.  An entry whose run was dropped and that has no match emits nothing and hands on
    // its predecessor's end — which is an emitting entry's: a run is only dropped in front of an entry WITH a match
    const uint32_t F0 = onT ? re : E;
    uint32_t Fp = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)F0, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    Fp = lane ? Fp : prev_end;
    const uint32_t F = (onM || onT) ? F0 : Fp;
    uint32_t pe = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)F, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    pe = lane ? pe : prev_end;
    prev_end = (uint32_t)__builtin_amdgcn_readlane((int)F, (int)(n - 1u));   // (handed on here: F is not carried across the stores)
    const uint32_t ms = msr > pe ? msr : pe;                           // the previous sequence may have taken some of the zeros in front
    // the entry's first sequence: M, or T alone (its literals start at pe either way); its second: T behind M
    const bool on1 = onM | onT, on2 = onM & onT;
    const uint32_t s1 = onM ? ms : rs, e1 = onM ? E : re;
    uint32_t ll1 = on1 ? s1 - pe : 0u, ml1 = e1 - s1 - 4u;
    const uint32_t off1 = onM ? off : 1u;
    const bool lit2 = on2 & (rs != E);
    uint32_t ml2 = re - rs - 4u;
    const uint32_t sz = (on1 ? 3u + bp_len_ext(ll1) + ll1 + bp_len_ext(ml1) : 0u) + (on2 ? 3u + (lit2 ? 1u : 0u) + bp_len_ext(ml2) : 0u);
    const uint32_t sincl = wave_scan_sum_dpp(sz, lane);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)sincl, 63);
    BP_MARK("sizes_done");
    // the batch's bytes go to the staging area; what is staged leaves in coalesced dwords when the next batch would not
    // fit (a batch larger than the whole area is written to global memory directly)
    if (__builtin_expect(sop + total > BpCfg<EXC>::STAGE, 0)) {
        bp_flush(S.stage + BP_SPARE, out + gop, sop, lane);
        gop += sop;
        sop = 0;
    }
    const uint32_t at = sincl - sz;
    BP_FORGET(ll1);
    BP_FORGET(ml1);
    BP_FORGET(ml2);
    if (__builtin_expect(total > BpCfg<EXC>::STAGE, 0)) {   // (wave-uniform, rare: a batch with hundreds of literals)
        bp_put_entry<EXC, false>(bm, xm, out + gop, at, pe, on1, ll1, ml1, off1, on2, lit2, ml2, lane);
        gop += total;
    } else {
        bp_put_entry<EXC, true>(bm, xm, S.stage, at + (sop + BP_SPARE), pe, on1, ll1, ml1, off1, on2, lit2, ml2, lane);
        sop += total;
    }
    return BpOut{prev_end, gop, sop};
}

// ---- the plane coder: one wave codes one plane (`wave`: which of the block's two), in the phases below (bp_code_plane at the end calls them in order)
// The lanes of the wave exchange data through the wave's BpLds (S) with no barrier in between: the LDS executes a wave's
// instructions in order.  What the COMPILER must not do is move a lane's read in front of another lane's earlier write;
// every such hand-over below is an access whose address it cannot tell apart from the lane's own writes, and BP_FENCE marks
// the phase boundaries for good measure: a phase whose writes other lanes read next ends with one.  (volatile pointers
// would also do — and turn every access into a serialised flat load with its own wait, which made this kernel 2x slower
// than it had to be.)
// How state travels, one rule per kind:
//   * a phase RETURNS its results by value, as a small struct (like BpOut, and for BpOut's reason);
//   * a phase TAKES the window's values as plain scalar parameters, not as those structs: the compiler simplifies every phase
//     on its own before it inlines it, a scalar parameter is known to hold a defined value there and a struct's field is not,
//     and what it makes of a bool that might be anything stays in the inlined code (lane masks turned into bytes in vector
//     registers: 0.7 % of the step at clevel 9).  bp_lane_one's BpOne goes as a struct only to bp_table_insert, which
//     does no arithmetic on it that differs;
//   * the four arrays several phases share — bm, P, wpre, flag — come as pointer parameters ("P: parameter" in the
//     headers below): bp_code_plane takes their addresses once, in front of everything, and the order in which the compiler
//     meets them decides its schedule (taken inside the phases, at first use, the int8 kernel needs 66 vector registers
//     instead of 64).  Every other array (cls, tab, chain, gbw, queue, stage, xm) a phase reaches through S.

// development probes; all three are empty in the default build
// -DBP_PROBE_SALU=n / -DBP_PROBE_VALU=n: n extra independent scalar / vector instructions per window — which issue port is
// the tight one?
__device__ __forceinline__ void bp_probe_salu()
{
#ifdef BP_PROBE_SALU
#pragma unroll
    for (int pr = 0; pr < BP_PROBE_SALU; ++pr) asm volatile("s_mov_b32 s90, 0" ::: "s90");
#endif
}

__device__ __forceinline__ void bp_probe_valu()
{
#ifdef BP_PROBE_VALU
    uint32_t pv;
#pragma unroll
    for (int pr = 0; pr < BP_PROBE_VALU; ++pr) asm volatile("v_mov_b32 %0, 0" : "=v"(pv));
#endif
}

// -DBP_PROBE_HANDOFF (round 4): the least a wave would pay to hand its stream to another workgroup INSIDE this launch
// (framing fused by a look-back, or "the chunk's last stream frames the chunk"): its stores drained, then one returning
// agent-scope atomic on a word the 256 streams of its chunk share (a spare word behind the chunk's first scratch slot).
// LZ4 stage with it: tools/dev/lz4_handoff.sh, DESIGN.md 3.3.  Returns the stream's size, op.
__device__ __forceinline__ uint32_t bp_probe_handoff(uint8_t *__restrict__ scratch, uint64_t sidx, uint64_t slot_bytes, uint32_t op, uint32_t lane)
{
#ifdef BP_PROBE_HANDOFF
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t old = 0;
    if (lane == 0) old = atomicAdd(reinterpret_cast<uint32_t *>(scratch + (sidx & ~255ull) * slot_bytes + slot_bytes - 8u), 1u);
    old = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
    op += old == 0xFFFFFFF0u ? 1u : 0u;   // (keeps the returned value alive; never true)
#endif
    return op;
}

// the ones of one 32-position half of the lane's 64 positions (bits w, EXC: missing-call bits x; the half starts at position
// base - 1) go to P[at...] (P: parameter, see above); returns the P-index behind the last one stored.  Each round is a count-trailing-zeros, a clear
// and a store, and there are as many rounds as the fullest word of the wave has ones.
// (no `if (w != 0)` around the body: a lane that has run out stores to P's spare entry — an exec-mask region costs two
// scalar instructions and a branch per round, and scalar issue is this kernel's tightest port)
template <bool EXC, typename LDS>
__device__ __forceinline__ uint32_t bp_list_half(LDS &S, uint16_t *P, uint32_t w, uint32_t x, uint32_t at, uint32_t base)
{
    while (__builtin_amdgcn_ballot_w64(w != 0u) != 0ull) {
        const bool on = w != 0u;
        const uint32_t bpos = (uint32_t)__builtin_ctz(w | 0x80000000u);
        if (EXC && on && ((x >> bpos) & 1u)) atomicOr(&S.cls[at >> 5], 1u << (at & 31u));   // (LDS: ds_or_b32)
        P[on ? at : BpCfg<EXC>::PTRASH] = (uint16_t)(base + bpos);
        at += on ? 1u : 0u;
        w &= w - 1u;
    }
    return at;
}

// the list of ones.  Reads nothing from S; writes wpre (every lane its own entry), P[0 .. m + 4] (P[0] = 0, the m ones, the
// four sentinels behind them) and, EXC, the class bits in cls (zeroed by the kernel before the call).  The lane's bit-map
// words (wlo, whi; EXC: xlo, xhi) and the scan over their counts (cnt, incl) come in registers.  Returns nothing.
// (P, wpre: parameters, see above.)
// (the two halves of the lane's 64 positions one after the other: twice ~6 rounds, where one loop over the 64-bit word ran
// ~11 rounds of twice the work)
template <bool EXC, typename LDS>
__device__ __forceinline__ void bp_list_ones(LDS &S, uint16_t *P, uint16_t *wpre, uint32_t wlo, uint32_t whi, uint32_t xlo, uint32_t xhi, uint32_t incl,
                                             uint32_t cnt, uint32_t m, uint32_t lane)
{
    wpre[lane] = (uint16_t)(incl - cnt);
    BP_FENCE();
    P[lane == 0u ? 0u : BpCfg<EXC>::PTRASH] = 0;
    const uint32_t base = 64u * lane + 1u;
    const uint32_t at = bp_list_half<EXC>(S, P, wlo, xlo, incl - cnt + 1u, base);
    bp_list_half<EXC>(S, P, whi, xhi, at, base + 32u);
    P[lane < 4u ? m + 1u + lane : BpCfg<EXC>::PTRASH] = (uint16_t)(BP_N + 1);
    BP_FENCE();
}

// gap bytes of all ones (a candidate is compared on them, 4 at a time).  Reads P (bp_list_ones); writes gbw[0 .. m + 8)
// as bytes: the zeros behind the one with P-index i, clipped to 255, and 255 from the last one on.  Returns nothing.
// (P: parameter, see above.)
template <bool EXC, typename LDS>
__device__ __forceinline__ void bp_gap_bytes(LDS &S, const uint16_t *P, uint32_t m, uint32_t lane)
{
    uint8_t *gb = reinterpret_cast<uint8_t *>(S.gbw);
    for (uint32_t i = lane; i < m + 8u; i += 64u) {
        const uint32_t i1 = i + 1u < BpCfg<EXC>::PTRASH ? i + 1u : BpCfg<EXC>::PTRASH;   // (i < m + 8 <= 644: the loads stay inside P)
        uint32_t g = (uint32_t)P[i1] - (uint32_t)P[i1 - 1u] - 1u;
        g = g < 255u ? g : 255u;
        gb[i] = (uint8_t)(i < m ? g : 255u);
    }
    BP_FENCE();
}

// the candidate table starts empty.  Writes tab; reads nothing.  (No fence: the first access behind it is the window's
// exchange on tab itself, bp_table_insert.)
template <typename LDS>
__device__ __forceinline__ void bp_clear_table(LDS &S, uint32_t lane)
{
#pragma unroll
    for (int k = 0; k < (1 << BP_HLOG) / 64; ++k) S.tab[64 * k + lane] = 0u;
}

// a lane's one of the window that starts at one jw (lane l has one j = jw + l; jw = -1 first: the virtual one at -1)
struct BpOne {
    int j, q;                    // index of the one (-1: the virtual one), its position
    uint32_t jj, q1, qn1, qp1;   // index into P (0 for a lane behind the last one); P[jj], P[jj + 1], P[jj - 1] (0 for jj = 0)
    uint32_t c5a;                // EXC: classes of this one (bit 0) and of the four ones behind it
    bool valid, can;             // there is a one j; it may start a table match
};

// Reads P (parameter, see above) and, EXC, cls (both bp_list_ones); writes nothing.  Returns the lane's one.
template <int DEPTH, bool EXC, typename LDS>
__device__ __forceinline__ BpOne bp_lane_one(LDS &S, const uint16_t *P, int jw, uint32_t m, uint32_t lane)
{
    BpOne o;
    o.j = jw + (int)lane;
    o.valid = o.j < (int)m;
    o.jj = o.valid ? (uint32_t)(o.j + 1) : 0u;
    o.q1 = P[o.jj], o.qn1 = P[o.jj + 1u];
    o.qp1 = P[(o.jj ? o.jj : 1u) - 1u];   // (jj = 0 reads P[0] = 0: one address, no exec-mask region around the load and no wait of its own)
    // (the three loads leave together and share one wait: left to itself the compiler moves the load of qn1 into the exec-mask
    // region of bp_table_insert, its only reader without the lazy rule — a second LDS round trip in front of the exchange)
    BP_FORGET(o.qn1);
    o.q = (int)o.q1 - 1;
    o.can = DEPTH > 0 && o.valid && o.j >= 0 && o.q + 12 <= BP_N;
    o.c5a = EXC ? (bp_bits(S.cls, o.jj) & 31u) : 0u;
    return o;
}

// candidate table: keyed on the gap behind the one; exact recency through the LDS's lane order.  Reads and writes tab by
// ONE exchange (cleared by bp_clear_table, filled by this phase in the windows before); CHAIN: writes chain[jj], what this
// one replaced, the next candidate down the chain.  Returns jc1: the most recent earlier one with the lane's key + 1, 0: none.
template <bool CHAIN, bool EXC, typename LDS>
__device__ __forceinline__ uint32_t bp_table_insert(LDS &S, BpOne o)
{
    uint32_t jc1 = 0;
    if (o.can) {
        const uint32_t g1 = o.qn1 - o.q1;
        const uint32_t idx = (g1 < BP_GAPCLIP ? g1 : BP_GAPCLIP) ^ ((EXC && (o.c5a & 1u)) ? 63u : 0u);
        jc1 = atomicExch(&S.tab[idx], (uint32_t)(o.j + 1));
        if (CHAIN) S.chain[o.jj] = (uint16_t)jc1;
    }
    BP_FENCE();
    return jc1;
}

struct BpPick {
    int best;            // the winner's score; < 0: no candidate agrees at all
    uint32_t bjq, bk;    // best >= 0: its P-index, full gaps it agrees on (0..BP_PICK)
    uint32_t a4;         // the lane's own next four gap bytes
};

// pick: the candidate with the longest forward agreement, judged on the gap BYTES — up to BP_PICK equal gaps, then 1 + the
// smaller of the next pair.  All a candidate costs is one unaligned 4-byte fetch from the gap bytes, an xor and a
// count-trailing-zeros; ties go to the nearer one.  Reads gbw (bp_gap_bytes), chain (bp_table_insert, this window and
// earlier ones: jc1 and everything down the chain lies in front of the lane's one) and, EXC, cls; writes nothing.  Returns
// the winner and the lane's own gap bytes, which the pricing needs again.
template <int DEPTH, bool EXC, typename LDS>
__device__ __forceinline__ BpPick bp_pick(LDS &S, uint32_t jj, uint32_t c5a, uint32_t jc1)
{
    constexpr bool CHAIN = DEPTH > 1;
    const uint32_t a4 = bp_gap4(S.gbw, jj);
    const uint8_t *gbb = reinterpret_cast<const uint8_t *>(S.gbw);
    // zeros in front of this one (clipped to 255).  (jj = 0, a lane without a one of its own, reads gbb[0]: it has no candidate
    // (jc1 = 0 there) and fa goes into candidates' scores only — one address for all lanes, no exec-mask region)
    uint32_t fa = (uint32_t)gbb[(jj ? jj : 1u) - 1u];
    fa = fa < BP_BACK ? fa : BP_BACK;   // (what a match takes along at most, clipped once for all candidates ...
    BP_FORGET(fa);                      // ... and kept so: the compiler would fold the clip back into every candidate's minimum)
    const uint32_t na4 = ~a4;
    const uint32_t stop4 = ((na4 - 0x01010101u) & ~na4 & 0x80808080u) | 0xFF000000u;   // a 255 agrees with nothing; 3 gaps at most
    int best = -1;
    uint32_t bjq = 0, bk = 0;
    // one candidate per lane: jc1, then what the chain holds behind it.  (A lane that may start no match has jc1 = 0 from
    // bp_table_insert, so `have` is one compare; a lane without a candidate reads the entries of one 1: a safe address, no
    // exec-mask region)
    auto consider = [&](const bool have) {
        const uint32_t jq = have ? jc1 : 1u;
        const uint32_t b4 = bp_gap4(S.gbw, jq);
        const uint32_t fb = (uint32_t)gbb[jq - 1u];
        uint32_t nextc = 0;
        if (CHAIN) nextc = S.chain[jq];
        const uint32_t x = (a4 ^ b4) | stop4;
        uint32_t k = (uint32_t)__builtin_ctz(x) >> 3;                           // agreeing gaps: 0..3
        bool same = true;
        if (EXC) {   // ... of which only those count whose next ones are of the same class; the first byte must agree at all
            const uint32_t xc = c5a ^ (bp_bits(S.cls, jq) & 31u);
            same = (xc & 1u) == 0u;
            const uint32_t tv = (uint32_t)__builtin_ctz((xc >> 1) | 8u);
            k = k < tv ? k : tv;
        }
        const uint32_t below = (1u << (8u * k)) - 1u;
        const uint32_t sumg = __builtin_amdgcn_sad_u8(a4 & below, 0u, k + 1u);  // their zeros + their ones + this one
        const uint32_t za = (a4 >> (8u * k)) & 0xFFu, zb = (b4 >> (8u * k)) & 0xFFu;
        const uint32_t fz = fa < fb ? fa : fb;                                  // the zeros in front a match would take along (fa: at most BP_BACK)
        const int score = (int)(sumg + (za < zb ? za : zb) + fz);
        const bool up = have & same & (score > best);   // (selects, not a branch)
        best = up ? score : best;
        bjq = up ? jq : bjq;
        bk = up ? k : bk;
        jc1 = have ? nextc : 0u;
    };
    if (DEPTH <= 2) {
        // one or two candidates: straight-line code.  The loop below asks the wave in front of every candidate whether any lane
        // still has one — a compare, its mask to the scalar unit, a branch, DEPTH + 1 times per window — and in a window of these
        // planes some lane nearly always has
#pragma unroll
        for (int left = 0; left < DEPTH; ++left) consider(jc1 != 0u);
    } else {
        // (counted down: counted up, the compiler keeps this counter in a vector register where the loop is a function of its
        // own, and a vector compare ends each of up to DEPTH rounds; so written it stays on the scalar unit, as it was inline)
#pragma unroll 1
        for (int left = DEPTH; left > 0; --left) {
            const bool have = jc1 != 0u;
            if (__builtin_amdgcn_ballot_w64(have) == 0ull) break;
            consider(have);
        }
    }
    return BpPick{best, bjq, bk, a4};
}

// what a one's table match is worth
struct BpMatch {
    bool hv;            // the one codes a match
    uint32_t len, nb;   // hv: bytes from the one on, zeros in front of the one the match is pulled back over
    uint32_t c1;        // hv: P[candidate] (the offset is q1 - c1)
    uint32_t a_last;    // hv: P-index of the last one the match covers
    uint32_t z_last;    // hv: zeros the match takes behind that one (0: it ends with the one)
    bool anycut;        // (wave-uniform) some lane's candidate reached past the stream's match limit: a match of this window may
                        // have been cut there, and what follows from a_last and z_last does not hold for such a match
};   // (len, nb, c1 without hv: anything — every reader asks hv first; zeroing them was three selects per window)

// hv: the match ends at the match limit or was cut there.  Asked only behind anycut, where the next one and the start of the run
// come from the bit map — which is right for every match, so the test may say yes to one that merely ends there
__device__ __forceinline__ bool bp_at_limit(bool hv, uint32_t E) { return hv & (E >= BP_MATCHLIMIT); }

// the chosen candidate, exactly (positions from P): agreement may continue past the third gap (periodic planes; rare), then
// the costs decide between this match and literals.  Reads P (parameter, see above) and, EXC, cls (bp_list_ones); writes
// nothing.  Takes the pick's result and the lane's one as scalars.  Returns the
// lane's match (hv = false where there is no candidate or literals are cheaper).
template <bool EXC, typename LDS>
__device__ __forceinline__ BpMatch bp_extend_and_price(LDS &S, const uint16_t *P, bool got, uint32_t bjq, uint32_t bk, uint32_t a4, uint32_t jj, int q,
                                                       uint32_t q1, uint32_t qp1, uint32_t m)
{
    uint32_t len = 0, nb = 0, c1 = 0, a_last = jj, z_last = 0;
    bool hv = false, anycut = false;
    if (__builtin_amdgcn_ballot_w64(got) != 0ull) {
        const uint32_t jq = got ? bjq : 1u;
        const uint32_t cc1 = P[jq], cp1 = P[jq - 1u];
        // the zeros in front that the one and its candidate share: what the match is pulled back over, at most BP_BACK
        const uint32_t gq = q1 - qp1 - 1u, gc = cc1 - cp1 - 1u;
        uint32_t cnb = gq < gc ? gq : gc;
        cnb = cnb < BP_BACK ? cnb : BP_BACK;
        // The one's side (a) and the candidate's side (b) walk in step, so b is a fixed distance behind a: ONE index is loop
        // state, doubled (a2 = 2 a: the byte offset into P).  The two positions travel as the halves of one register —
        // (pa, pb), at most BP_N + 1 each — and one packed subtraction gives both steps d = (ga + 1, gb + 1).  What the
        // loop used to add up it no longer does: the steps taken telescope to pa - q1, and the last step's gaps are read
        // off the d the lane stopped at.  The step count s = a - jj needs no counter either: s < BP_PICK can only hold at a
        // lane's first step, and s >= BP_STEPS and a >= m are one limit on a (lim2).  Same decisions, tools/sim/gapenc_ref.c's.
        const uint8_t *P8 = reinterpret_cast<const uint8_t *>(P);
        const uint32_t back2 = 2u * (jj - jq);      // (jq < jj: the candidate lies in front)
        uint32_t a2 = 2u * (jj + bk);               // twice the P-index of the one the first open comparison starts at
        const uint32_t lim = m < jj + BP_STEPS ? m : jj + BP_STEPS;
        uint32_t lim2 = bk < BP_PICK ? 0u : 2u * lim;   // (s < BP_PICK: a limit every a has reached)
        BP_FORGET(lim2);   // (or the compiler turns the select back into a lane mask that lives across the loop, and the lazy forms run out of scalar registers)
        u16x2 pp = bp_pair(*reinterpret_cast<const uint16_t *>(P8 + a2), *reinterpret_cast<const uint16_t *>(P8 + a2 - back2));
        u16x2 dl = bp_pair(1, 1);
        // what the bk agreed gaps cost as literals and runs: 1 + min(gap, BP_TMIN) each (the gaps behind them masked away once,
        // not one select per gap)
        uint32_t am = a4 & ((1u << (8u * bk)) - 1u);
        BP_FORGET(am);   // (or mask and byte select merge into one operation per gap, each with a constant in a scalar register)
        uint32_t costR = bk;
#pragma unroll
        for (uint32_t s = 0; s < BP_PICK; ++s) {
            const uint32_t g = (am >> (8u * s)) & 0xFFu;
            costR += g < BP_TMIN ? g : BP_TMIN;
        }
        uint32_t st2 = got ? 2u : 0u;   // what a2 advances by: 2 while the lane goes on, 0 once it has stopped (as a number, not a lane mask: the ballot is one compare's)
        for (;;) {   // (the trip count is what the wave needs)
            const bool act = st2 != 0u;
            if (__builtin_amdgcn_ballot_w64(act) == 0ull) break;
            // (branch-free body: lanes that are done keep their values through selects; a + 1, b + 1 <= m + 4 stay inside P)
            const u16x2 nn = bp_pair(*reinterpret_cast<const uint16_t *>(P8 + a2 + 2u), *reinterpret_cast<const uint16_t *>(P8 + a2 - back2 + 2u));
            const u16x2 d = nn - pp;
            const uint32_t da = d.x, db = d.y;
            const bool cdiff = EXC && (((bp_bits(S.cls, (a2 >> 1) + 1u) ^ bp_bits(S.cls, ((a2 - back2) >> 1) + 1u)) & 1u) != 0u);
            const bool stop = (da != db) | (((__builtin_bit_cast(uint32_t, d) >> 8) & 0xFFu) != 0u) | (a2 >= lim2) | cdiff;   // (da >= 256 by its high byte: no constant in a scalar register)
            costR += act ? (da < BP_TMIN + 1u ? da : BP_TMIN + 1u) : 0u;
            dl = act ? d : dl;
            st2 = stop ? 0u : st2;
            a2 += st2;
            pp = st2 != 0u ? nn : pp;
        }
        const uint32_t a = a2 >> 1;
        const uint32_t z1 = dl.x < dl.y ? dl.x : dl.y, zl = z1 - 1u, tailz = (uint32_t)dl.x - z1;
        const uint32_t clen = (uint32_t)pp.x - q1 + z1;
        const uint32_t costH = 3u + (clen + cnb >= 19u ? 1u : 0u) - cnb + (tailz >= BP_TMIN ? 3u : tailz);
        uint32_t end = (uint32_t)q + clen;
        const bool cut = end > BP_MATCHLIMIT;
        end = end < BP_MATCHLIMIT ? end : BP_MATCHLIMIT;
        // signed compares: costH may go below zero when many zeros are pulled in
        const int gain = (int)costR - (int)costH;
        hv = got & (gain > 0) & ((int)end - q >= 4) & ((int)end - (q - (int)cnb) >= BP_MINM) & (q <= BP_MFLIMIT);   // (& not &&: no nest of exec-mask regions)
        len = end - (uint32_t)q;
        nb = cnb;
        c1 = cc1;
        a_last = a;
        z_last = zl;
        // (the ballot of ONE compare, taken here and handed on as a scalar: `cut & hv` per lane crossed this block's end as a
        // number and was compared again in front of each of the two branches that ask.  A lane without a candidate has
        // clen = 1 here and says yes only for a one in the plane's last five bytes)
        anycut = __builtin_amdgcn_ballot_w64(cut) != 0ull;
    }
    return BpMatch{hv, len, nb, c1, a_last, z_last, anycut};
}

// one-step lazy rule (the file-writing paths' effort level; tools/sim/gapenc_ref.c states it): a one gives up its match when
// the NEXT one lies inside that match and has a match of its own that ends further by at least BP_LAZY_MIN + what giving up
// costs (the zeros this one's match was pulled back over, the zeros between this one and the start of the next one's
// match).  The next one is the neighbouring lane (the window's last lane keeps its match); in a run of lanes that all would
// give up, every other one does, counted from the far end.  Touches no LDS: the neighbour's match comes over DPP.  Returns
// the lane's match, or no match where it gave up.
__device__ __forceinline__ BpMatch bp_lazy_rule(bool hv, uint32_t len, uint32_t nb, uint32_t c1, uint32_t a_last, uint32_t z_last, bool anycut, int j, int q,
                                             uint32_t jj, uint32_t q1, uint32_t qn1, uint32_t m, uint32_t lane)
{
    const uint32_t E0 = hv ? (uint32_t)q + len : (uint32_t)(q + 1);
    const uint32_t hvN = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(hv ? 1u : 0u), 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
    const uint32_t EN = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)E0, 0x130, 0xf, 0xf, false);
    const uint32_t nbN = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)nb, 0x130, 0xf, 0xf, false);   // (means something with hvN)
    const int msN = (int)qn1 - 1 - (int)nbN;                        // where the next one's match starts
    const int between = msN - (int)q1 > 0 ? msN - (int)q1 : 0;     // zeros between this one and that start
    const bool Ln = hv & (hvN != 0u) & (lane < 63u) & (j + 1 < (int)m) & (qn1 <= E0) &
                    ((int)EN - (int)E0 >= (int)(BP_LAZY_MIN + nb) + between);
    const unsigned long long lm = __builtin_amdgcn_ballot_w64(Ln);
    const unsigned long long rest = ~(lm >> lane);                 // first zero bit = end of this lane's run
    const uint32_t tlo = (uint32_t)__builtin_ctz((uint32_t)rest | 0x80000000u), thi = (uint32_t)__builtin_ctz((uint32_t)(rest >> 32) | 0x80000000u);
    const uint32_t t = (uint32_t)rest != 0u ? tlo : 32u + thi;     // (lm >> lane has zeros from bit 64 - lane on: the run ends inside)
    const bool give = Ln && (t & 1u);
    return BpMatch{hv && !give, len, nb, c1, give ? jj : a_last, give ? 0u : z_last, anycut};
}

struct BpNext {
    uint32_t E;     // end of what this one codes (0 for the virtual one)
    uint32_t nxt;   // index of the first one at or behind E: the next coded one if this one is coded
};

// where the greedy parse goes on behind this one: first one at or behind E = the number of ones in front of position E.  A
// one that codes itself alone (E = q + 1) has itself and its predecessors in front: its own P-index.  A match ends in the
// zeros behind the last one it covers (or exactly at the next one): that one's P-index.  Only a match that was cut at the
// stream's match limit (a handful of ones at the very end of a plane) needs the count from the bit map: reads bm (the
// kernel, before bp_code_plane) and wpre (bp_list_ones) then, nothing otherwise (both parameters, see above); writes nothing.
__device__ __forceinline__ BpNext bp_next_one(const uint32_t *bm, const uint16_t *wpre, bool hv, uint32_t len, uint32_t a_last, bool anycut, int q, uint32_t jj,
                                           uint32_t m)
{
    const uint32_t E = hv ? (uint32_t)q + len : (uint32_t)(q + 1);
    uint32_t nxt = hv ? a_last : jj;
    if (__builtin_expect(anycut, 0)) {   // (wave-uniform, rare)
        const bool clamped = bp_at_limit(hv, E);
        const uint32_t w = E >> 6, bb = E & 63u, wc = w < 63u ? w : 63u;
        const uint32_t lo = bm[2u * wc], hi = bm[2u * wc + 1u];
        const uint32_t mlo = bb >= 32u ? 0xFFFFFFFFu : ((1u << bb) - 1u);
        const uint32_t mhi = bb > 32u ? ((1u << (bb - 32u)) - 1u) : 0u;
        const uint32_t in_map = (uint32_t)wpre[wc] + (uint32_t)__popc(lo & mlo) + (uint32_t)__popc(hi & mhi);
        nxt = clamped ? (w >= 64u ? m : in_map) : nxt;
    }
    return BpNext{E, nxt};
}

struct BpSel {
    bool sel;   // this one is coded
    int cur;    // next one to be coded behind this window (unchanged where the window's last coded one is not known yet)
};

// which ones of the window are coded: follow nxt from `cur` by pointer doubling.  Writes and reads flag[0 .. 64] (and its
// two spare bytes), in rounds that a fence separates: a lane marks where it jumps to, then reads its own mark; nobody else
// uses flag (parameter, see above).  (Measured against the plain walk on the scalar unit — one v_readlane + 5 scalar instructions per coded one,
// half the vector instructions: 14.8 against 13.0 ms per step; rebuilt leaner in round 4, one v_readlane + ~6 scalar
// instructions and no LDS: LZ4 stage 14.0 against 12.1 ms.  A wave's dependent chain is what counts, not its instruction total.)
__device__ __forceinline__ BpSel bp_select_coded(uint8_t *flag, bool valid, uint32_t nxt, int jw, int cur, uint32_t lane)
{
    bool sel = false;
    if (cur < jw + 64) {   // (wave-uniform) otherwise the whole window lies inside an earlier match
        const uint32_t e0 = (uint32_t)(cur - jw);
        // nxt > j: always forward.  (65 for a lane without a one: `the coded one whose successor lies outside` below is p0 == 64
        // alone; such a lane, if reached, marks flag[65], which like flag[64] nobody reads)
        uint32_t jump = valid ? (nxt - (uint32_t)jw < 64u ? nxt - (uint32_t)jw : 64u) : 65u;
        const uint32_t p0 = jump;
        flag[lane] = lane == e0 ? 1u : 0u;
        flag[lane == 0u ? 64u : 69u] = 0u;
        BP_FENCE();
        uint32_t mark = lane == e0 ? 1u : 0u;   // the lane's flag: 0 or 1
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            flag[mark != 0u ? jump : 68u] = 1u;   // (no exec-mask region: a scalar instruction costs this kernel four times a vector one)
            BP_FENCE();
            mark = flag[lane];
            // (the lane is bits 2-7 of the address: no mask for jump = 64, 65, whose result is not used)
            const uint32_t j2 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(jump << 2), (int)jump);
            jump = jump < 64u ? j2 : 64u;
        }
        sel = mark != 0u && valid;
        // (mark and p0 as numbers, one compare for the ballot: not two lane masks joined and turned into a number again)
        const unsigned long long ex = __builtin_amdgcn_ballot_w64(__umul24(mark, p0) == 64u);
        // the coded one whose successor lies outside the window hands over to the next window
        if (ex != 0ull) cur = (int)__builtin_amdgcn_readlane((int)nxt, (int)(__ffsll((long long)ex) - 1));
    }
    return BpSel{sel, cur};
}

struct BpQueued {
    BpOut out;     // where the stream stands
    uint32_t qn;   // queued coded ones
};

// the coded ones that emit something — a match M (if hv) and / or a tail run T over the zeros up to the next coded one — are
// queued; layout and emission run on 64 of them at a time (bp_emit_batch), every lane busy, where the first version laid out
// and emitted per window with the ~30 % of its lanes that were coded ones.  Reads P (bp_list_ones) and, for a clamped match,
// bm (both parameters, see above); writes queue, which bp_emit_batch reads behind a fence, and moves what a batch leaves to the queue's front (read, fence,
// write); bp_emit_batch fills stage.  Returns the stream's state and the queue's length.
template <bool EXC, typename LDS>
__device__ __forceinline__ BpQueued bp_queue_and_drain(LDS &S, const uint32_t *bm, const uint16_t *P, uint8_t *out, int q, uint32_t q1, bool hv, uint32_t nb,
                                                       uint32_t c1, uint32_t z_last, bool anycut, uint32_t E, uint32_t nxt, bool sel, int jw, uint32_t m,
                                                       uint32_t prev_end, uint32_t gop, uint32_t sop, uint32_t qn, uint32_t lane)
{
    const bool onM = sel && hv;
    // the run behind E starts one later when byte E - 1 is a one (an offset-1 run copies its predecessor): always for a one
    // that codes itself alone (and the virtual one in front of the stream), for a match when it ends with its last one
    uint32_t rs = E + ((!hv || z_last == 0u) ? 1u : 0u);
    if (__builtin_expect(anycut, 0))   // (wave-uniform, rare: a match cut at the match limit — ask the bit map)
        rs = bp_at_limit(hv, E) ? E + ((bp_bits(bm, E - 1u) & 1u) ? 1u : 0u) : rs;
    uint32_t re = (uint32_t)P[(nxt < m ? nxt : m) + 1u] - 1u;   // position of the next one (n behind the last)
    re = re < BP_MATCHLIMIT ? re : BP_MATCHLIMIT;
    const bool onT = sel && (int)re - (int)rs >= BP_TMIN && rs <= BP_MFLIMIT;   // (long enough; emitted or not: bp_emit_batch)
    uint2 ent = bp_entry(E, (uint32_t)(q - (int)nb), onM, onT, rs, re, q1 - c1);   // (packed here: two registers live across a make-room batch)
    // onM || onT, read off the packed entry: ONE compare, and its result is the ballot (as `onM || onT` the two lane masks are
    // joined on the scalar unit, turned into 0 / 1 per lane and compared again — the compiler's way from a lane mask to a ballot)
    BP_HIDE(ent.x);
    const bool want = ent.x >= BP_ENT_ANY;
    const unsigned long long wm = __builtin_amdgcn_ballot_w64(want);
    const uint32_t nw = (uint32_t)__builtin_popcountll(wm);
    const bool last = jw + 64 >= (int)m;
    // one call site for the batch code: first make room if this window's coded ones would not fit (rare), then queue
    // them, then drain whole batches (everything at the end)
    for (int phase = 0; phase < 2; ++phase) {
        if (phase == 1) {
            const uint32_t slot = qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(wm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)wm, 0u));
            S.queue[want ? slot : BpCfg<EXC>::QCAP] = ent;
            qn += nw;
            BP_MARK("queued");
        }
        // a batch leaves the queue when the entry behind its last one is there too (the run rule looks at it) — or when
        // the stream ends
        while (phase == 0 ? qn + nw > BpCfg<EXC>::QCAP : (qn >= 65u || (last && qn != 0u))) {   // (wave-uniform)
            const uint32_t keep = phase == 1 && last ? 0u : 1u;
            const uint32_t nb_ = qn - keep < 64u ? qn - keep : 64u;
            BP_FENCE();
            const BpOut r = bp_emit_batch<EXC>(S, bm, out, nb_, qn, BpOut{prev_end, gop, sop}, lane);
            prev_end = r.prev_end, gop = r.gop, sop = r.sop;
            BP_FENCE();
            const bool mvp = lane + nb_ < qn;
            const uint2 mv = S.queue[mvp ? nb_ + lane : BpCfg<EXC>::QCAP];
            BP_FENCE();
            S.queue[mvp ? lane : BpCfg<EXC>::QCAP] = mv;
            qn -= nb_;
        }
    }
    return BpQueued{BpOut{prev_end, gop, sop}, qn};
}

// the last literals: everything behind the last sequence's end, as a sequence without a match.  Reads bm (parameter, see
// above) and, EXC, xm (the kernel); writes stage behind what bp_emit_batch staged (or, a run larger than the staging area, the stream's slot).
// Returns where the stream stands.
template <bool EXC, typename LDS>
__device__ __forceinline__ BpOut bp_last_literals(LDS &S, const uint32_t *bm, uint8_t *out, uint32_t prev_end, uint32_t gop, uint32_t sop, uint32_t lane)
{
    const uint32_t ll = BP_N - prev_end, llx = bp_len_ext(ll);
    BP_FENCE();
    if (sop + 1u + llx + ll > BpCfg<EXC>::STAGE) {
        bp_flush(S.stage + BP_SPARE, out + gop, sop, lane);
        gop += sop;
        sop = 0;
    }
    const bool direct = 1u + llx + ll > BpCfg<EXC>::STAGE;
    auto tail = [&](auto dstp) {
        if (lane == 0) {
            dstp[0] = (uint8_t)((ll < 15u ? ll : 15u) << 4);
            uint32_t r = ll - 15u;
            for (uint32_t k = 0; k < llx; ++k) {
                dstp[1u + k] = (uint8_t)(k + 1u == llx ? r : 255u);
                r -= 255u;
            }
        }
        for (uint32_t k = lane; k < ll; k += 64u)
            dstp[1u + llx + k] = (uint8_t)bp_lit<EXC>(bp_bits(bm, prev_end + k), EXC ? bp_bits(S.xm, prev_end + k) : 0u, 0u);
    };
    if (direct) {
        tail(out + gop);
        gop += 1u + llx + ll;
    } else {
        tail(S.stage + BP_SPARE + sop);
        sop += 1u + llx + ll;
    }
    return BpOut{prev_end, gop, sop};
}

// the end of the stream: what is staged leaves for the stream's slot — or, incompressible, the plane itself does: Blosc
// stores the (shuffled) stream verbatim.  Reads stage (bp_emit_batch, bp_last_literals) or bm (parameter, see above) and xm.  Returns the stream's size.
template <bool EXC, typename LDS>
__device__ __forceinline__ uint32_t bp_finish_stream(LDS &S, const uint32_t *bm, uint8_t *out, BpOut st, uint32_t lane)
{
    uint32_t op = st.gop + st.sop;
    if (op >= BP_N) {
        for (uint32_t k = lane; k < BP_N; k += 64u) out[k] = (uint8_t)bp_lit<EXC>(bp_bits(bm, k), EXC ? bp_bits(S.xm, k) : 0u, 0u);
        op = BP_N;
    } else {
        BP_FENCE();
        bp_flush(S.stage + BP_SPARE, out + st.gop, st.sop, lane);
    }
    return op;
}

// One plane, from its bit map(s) in registers to its stream (or its mark): everything behind the loads.  A plane left to the
// byte-wise kernel gets csize = MARK, and flags[0] = tag says "this call left a mark" to that kernel's scan.
// The BP_SKIP exits (development, timing only) cut the coder short between two phases; `sink` keeps what was computed alive.
template <int DEPTH, bool EXC, bool LAZY, typename LDS>
__device__ __forceinline__ void bp_code_plane(LDS &S, uint32_t wlo, uint32_t whi, uint32_t xlo, uint32_t xhi, bool nonbinary, uint32_t bid,
                                              uint32_t wave, uint32_t lane, uint8_t *__restrict__ scratch, uint64_t slot_bytes,
                                              uint32_t *__restrict__ csize, uint32_t *__restrict__ flags, uint32_t tag)
{
    uint32_t sink = 0;
    // (the shared arrays' addresses, taken here and in this order: see "the plane coder" above)
    uint32_t *bm = S.bm;
    uint16_t *P = S.P;
    uint16_t *wpre = S.wpre;
    uint8_t *flag = S.flag;
    const uint64_t sidx = (uint64_t)bid * 2u + wave;
    uint8_t *out = scratch + sidx * slot_bytes;

    const uint32_t cnt = (uint32_t)__popc(wlo) + (uint32_t)__popc(whi);
    uint32_t m;   // ones in the plane
    const uint32_t incl = wave_scan_sum_dpp(cnt, lane, &m);
    if (nonbinary || m > BpCfg<EXC>::MAXONES) {
        // (the flag: read first — the line sits in the L2 and after the first few marking waves of an XCD it holds the tag)
        if (lane == 0 && flags && flags[0] != tag) flags[0] = tag;
        if (lane == 0) csize[sidx] = 0xFFFFFFFFu;   // left to the byte-wise kernel
        return;
    }
    BP_MARK("scan_done");
    bp_list_ones<EXC>(S, P, wpre, wlo, whi, xlo, xhi, incl, cnt, m, lane);
    if (DEPTH > 0) bp_gap_bytes<EXC>(S, P, m, lane);
    bp_clear_table(S, lane);
    BP_MARK("plist_done");
    if (BP_SKIP >= 4) {
        if (lane == 0) csize[sidx] = P[m] & 1u;
        return;
    }
    BpQueued st{BpOut{0u, 0u, 0u}, 0u};
    int cur = -1;   // next one to be coded (the virtual one in front of the stream first)
    for (int jw = -1; jw < (int)m; jw += 64) {
        BP_MARK("win_begin");
        bp_probe_salu();
        bp_probe_valu();
        const BpOne o = bp_lane_one<DEPTH, EXC>(S, P, jw, m, lane);
        const uint32_t jc1 = bp_table_insert<(DEPTH > 1), EXC>(S, o);
        BP_MARK("hash_done");
        BpMatch mt{false, 0u, 0u, 0u, o.jj, 0u, false};
        if (DEPTH > 0) {
            const BpPick pk = bp_pick<DEPTH, EXC>(S, o.jj, o.c5a, jc1);
            mt = bp_extend_and_price<EXC>(S, P, pk.best >= 0, pk.bjq, pk.bk, pk.a4, o.jj, o.q, o.q1, o.qp1, m);
        }
        BP_MARK("cand_done");
        if (LAZY) mt = bp_lazy_rule(mt.hv, mt.len, mt.nb, mt.c1, mt.a_last, mt.z_last, mt.anycut, o.j, o.q, o.jj, o.q1, o.qn1, m, lane);
        const BpNext nx = bp_next_one(bm, wpre, mt.hv, mt.len, mt.a_last, mt.anycut, o.q, o.jj, m);
        BP_MARK("nxt_done");
        if (BP_SKIP >= 3) {
            sink += nx.nxt + nx.E;
            continue;
        }
        const BpSel sl = bp_select_coded(flag, o.valid, nx.nxt, jw, cur, lane);
        cur = sl.cur;
        BP_MARK("sel_done");
        if (BP_SKIP >= 2) {
            sink += sl.sel ? nx.nxt : 0u;
            continue;
        }
        st = bp_queue_and_drain<EXC>(S, bm, P, out, o.q, o.q1, mt.hv, mt.nb, mt.c1, mt.z_last, mt.anycut, nx.E, nx.nxt, sl.sel, jw, m, st.out.prev_end,
                                     st.out.gop, st.out.sop, st.qn, lane);
        BP_MARK("emit_done");
    }
    BP_MARK("loop_done");
    if (BP_SKIP >= 1) {
        if (lane == 0) csize[sidx] = (st.out.prev_end + sink) & 0xFFFu;
        return;
    }
    uint32_t op = bp_finish_stream<EXC>(S, bm, out, bp_last_literals<EXC>(S, bm, out, st.out.prev_end, st.out.gop, st.out.sop, lane), lane);
    if (BP_SKIP) op = (op & 0xFFFu) + (sink & 1u);
    op = bp_probe_handoff(scratch, sidx, slot_bytes, op, lane);
    if (lane == 0) csize[sidx] = op;
}

// int8 input (the matrix itself): grid = number of 8 KiB blocks; 128 threads: wave w codes byte plane w of the block
// DEPTH = candidates tried per one along the hash chain (1: the table's entry only; 0: no hash matches at all,
// offset-1 runs only — the fastest level)
template <int DEPTH, bool LAZY = false>
__global__ __launch_bounds__(128, BP_WAVES) void k_lz4_bitplanes(const uint8_t *__restrict__ src, PlanesGeom pg, uint32_t n_blocks,
                                                                  uint8_t *__restrict__ scratch, uint64_t slot_bytes, uint32_t *__restrict__ csize,
                                                                  uint32_t *__restrict__ flags, uint32_t tag)
{
    constexpr bool CHAIN = DEPTH > 1;
    __shared__ BpLds<CHAIN, false> lds[2];
    __shared__ uint32_t nonbin[2][2];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const uint32_t bid = blockIdx.x;
    // (a one-trip loop, kept for what it buys in the compiler's schedule.  Without it every instantiation grows — by 1 to 3
    // instructions without the lazy rule at depth >= 2, by 9 to 14 elsewhere — and depths 0 and 1 and the two lazy forms take
    // 66 instead of 64 VGPRs; at depths 0 and 1, where the LDS would allow nine workgroups per SIMD pair, that is 7 instead of
    // 8 waves per SIMD.  Checked per instantiation by tests/test_isa_counts.py.)
    for (int once = 0; once < 1; ++once) {
    const uint8_t *blk = src + (uint64_t)bid * 8192u;

    // ---- phase A: wave r packs the bits of block bytes [4096 r, 4096 r + 4096) for BOTH planes (byte-shuffle fused:
    //      even bytes are plane 0, odd bytes plane 1).  Load k of a lane is the 16 bytes at 1024 k + 16 lane: every load
    //      instruction of the wave covers one contiguous KiB (the first version gave each lane 64 contiguous bytes, i.e.
    //      four instructions that each touched all 64 lines of the half block; FETCH_SIZE is the same either way — the L2
    //      absorbed the repeats — but the step is 1.5 % faster with this form).
    //      16 bytes = 8 positions of each plane = one BYTE of each bit map, at byte 256 r + 64 k + lane.
    {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 *p = reinterpret_cast<const u32x4 *>(blk + 4096u * wave + 16u * lane);
        u32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = __builtin_nontemporal_load(p + 64 * k);   // streamed once
        uint32_t orall = 0;
        uint8_t *bm0 = reinterpret_cast<uint8_t *>(lds[0].bm) + 256u * wave + lane;
        uint8_t *bm1 = reinterpret_cast<uint8_t *>(lds[1].bm) + 256u * wave + lane;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t d[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
            uint32_t acc0 = 0, acc1 = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t x = d[i];
                orall |= x;
                const uint32_t xm = x & 0x01010101u;   // (a byte > 1 in one plane must not leak into the other plane's bits)
                const uint32_t y = xm | (xm >> 15);    // bits 0,1: plane-0 bytes; bits 8,9: plane-1 bytes
                acc0 |= (y & 3u) << (2 * i);
                acc1 |= ((y >> 8) & 3u) << (2 * i);
            }
            bm0[64 * k] = (uint8_t)acc0;
            bm1[64 * k] = (uint8_t)acc1;
        }
        const uint32_t nb0 = orall & 0x00FE00FEu, nb1 = orall & 0xFE00FE00u;   // a byte > 1 somewhere in plane 0 / plane 1
        const unsigned long long b0 = __builtin_amdgcn_ballot_w64(nb0 != 0u), b1 = __builtin_amdgcn_ballot_w64(nb1 != 0u);
        if (lane == 0) {
            nonbin[wave][0] = b0 != 0ull;
            nonbin[wave][1] = b1 != 0ull;
        }
        if (lane < 4u) lds[wave].bm[128u + lane] = 0u;
    }
    __syncthreads();
    const uint32_t wlo = lds[wave].bm[2u * lane], whi = lds[wave].bm[2u * lane + 1u];
    const bool nonbinary = (nonbin[0][wave] | nonbin[1][wave]) != 0u;
    BP_MARK("A_done");
    if (BP_SKIP >= 5) {
        if (lane == 0) csize[(uint64_t)bid * 2u + wave] = lds[wave].bm[5] & 1u;
        return;
    }

    bp_code_plane<DEPTH, false, LAZY>(lds[wave], wlo, whi, 0u, 0u, nonbinary, bid, wave, lane, scratch, slot_bytes, csize, flags, tag);
    }
}

// Bit-plane input (include/hhgt.h, tile-major: common.h; written by k_encode_planes): the wave's bit map is 16 pieces of
// 32 bytes it gathers as they are (one load instruction: lane l takes 8 bytes of tile l / 4).
// Grid: ONE WAVE PER WORKGROUP, one workgroup per plane, two per block (stream 2 block + plane, as ever).  The kernel has no
// barrier and the two planes of a block share nothing; as a pair they shared one LDS allocation, and the wave slot of the
// plane that finished first (a plane runs four or five windows, by its ones) idled until its sibling ended.  Alone, a
// finished plane frees slot, registers and LDS at once.  LDS per workgroup: sizeof(BpBoth) <= BP_PLANE_LDS = 5120 bytes,
// 32 workgroups per CU; the single-wave form compiles to 64 VGPRs (the pair took 70-72), so registers allow those eight
// waves per SIMD as well (seven before: 14 pairs).
// Order: the pieces of four neighbouring sample rows share a 128-byte line, so the planes are dealt to the workgroups in an
// XCD-aware order: of 128 consecutive workgroups the sixteen that land on one XCD (round robin) take both planes of eight
// consecutive blocks — one L2 fetches each line once (the grid is rounded up to whole groups of 128 = 64 blocks; workgroups
// beyond the last block return).
// The plain and the exception-aware coder in ONE launch (round 4): a workgroup looks at its plane's missing-call map and takes
// the one or the other path (both are bp_code_plane, inlined).  The exception-aware path codes planes whose bytes
// are 0, 1 or 0xF7 (missing calls; config 4): the bit map is the map of NONZERO bytes, a second map says which of them are
// 0xF7, every one carries that bit as its class, and two ones only agree if their classes do (tools/sim/gapenc_ref.c states
// the rules).  What this replaced was a plain launch marking every plane that holds a missing call for a second, scanning
// launch — on config 4, where every plane does, 0.4 ms of reading all planes for nothing.  Planes neither path can code (a
// call beyond 0 / 1 / missing, too many nonzero bytes) are marked for the byte-wise kernel (flags[0]).
template <int DEPTH, bool LAZY>
__global__ __launch_bounds__(64, BP_WAVES) void k_lz4_bitplanes_uni(const uint8_t *__restrict__ src, PlanesGeom pg, uint32_t n_blocks,
                                                                     uint8_t *__restrict__ scratch, uint64_t slot_bytes,
                                                                     uint32_t *__restrict__ csize, uint32_t *__restrict__ flags, uint32_t tag, PlanesDiv dv)
{
    constexpr bool CHAIN = DEPTH > 1;
    union BpBoth {
        BpLds<CHAIN, false> p;
        BpLds<CHAIN, true> x;
    };
    static_assert(sizeof(BpBoth) <= BP_PLANE_LDS, "32 planes per CU");
    __shared__ BpBoth lds;
    const uint32_t lane = threadIdx.x;
    uint32_t bid, wave;   // (XCD-aware order, common.h; wave: the byte plane, as before)
    planes_wg_plane(blockIdx.x, &bid, &wave);
    if (bid >= n_blocks) return;
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    // (block -> column, row, block in the row by the launch's reciprocals: the two divisions of planes_block were 32 scalar and 13
    // vector instructions of the 157 in front of the address of the wave's only global load.  dv is the LAST argument on purpose: in
    // front of n_blocks the same code takes 70 VGPRs instead of 64 in every instantiation — the order of the kernel-argument
    // loads moves the register allocation of the whole body; tests/test_lz4_plane_occupancy.py holds the line)
    const u32x2 *pl = reinterpret_cast<const u32x2 *>(src + planes_lane_bytes(pg, dv, bid, wave, lane));
    const u32x2 one = *pl, exc = *(pl + (uint64_t)pg.S_pad * 8ull);
    // (both branches store the bit map of the nonzero bytes, at the same place: stored once in front of the branch, every
    // instantiation but depth 0 takes 72 instead of 70 VGPRs)
    if (__builtin_amdgcn_ballot_w64((exc.x | exc.y) != 0u) == 0ull) {   // no missing call in this plane: the plain coder
        // An empty plane (3.6 % of the flagship's: padded sample rows, columns rounded up to whole chunks) leaves at once with
        // the stream every instantiation's bp_code_plane makes of 4096 zeros — tools/sim/gapenc_ref.c's, at every depth and
        // with the lazy rule: a zero literal, an offset-1 match of 4090 (15 + 15 x 255 + 246 + 4), the last five literals.
        if (BP_SKIP < 6 && __builtin_amdgcn_ballot_w64((one.x | one.y) != 0u) == 0ull) {
            const uint64_t sidx = (uint64_t)bid * 2u + wave;
            const uint32_t v = lane == 0u ? 0x1Fu : lane == 2u ? 1u : lane == 19u ? 0xF6u : lane == 20u ? 0x50u : (lane - 4u < 15u ? 0xFFu : 0u);
            if (lane < BP_EMPTY_BYTES) scratch[sidx * slot_bytes + lane] = (uint8_t)v;
            if (lane == 0) csize[sidx] = BP_EMPTY_BYTES;
            return;
        }
        BpLds<CHAIN, false> &S = lds.p;
        S.bm[2u * lane] = one.x;
        S.bm[2u * lane + 1u] = one.y;
        if (lane < 4u) S.bm[128u + lane] = 0u;
        if (BP_SKIP >= 6) {
            if (lane == 0) csize[(uint64_t)bid * 2u + wave] = S.bm[5] & 1u;
            return;
        }
        bp_code_plane<DEPTH, false, LAZY>(S, one.x, one.y, 0u, 0u, false, bid, wave, lane, scratch, slot_bytes, csize, flags, tag);
    } else {
        BpLds<CHAIN, true> &S = lds.x;
        // (ONE, EXC) = (0, 1): a call beyond 0 / 1 / missing, its byte lives in the int8 matrix — not this coder's
        const bool nonbinary = __builtin_amdgcn_ballot_w64(((exc.x & ~one.x) | (exc.y & ~one.y)) != 0u) != 0ull;
        S.bm[2u * lane] = one.x;
        S.bm[2u * lane + 1u] = one.y;
        if (lane < 4u) S.bm[128u + lane] = 0u;
        S.xm[2u * lane] = exc.x;
        S.xm[2u * lane + 1u] = exc.y;
        if (lane < 4u) S.xm[128u + lane] = 0u;
        if (lane < 24u) S.cls[lane] = 0u;
        if (BP_SKIP >= 6) {
            if (lane == 0) csize[(uint64_t)bid * 2u + wave] = (S.bm[5] ^ S.xm[5]) & 1u;
            return;
        }
        bp_code_plane<DEPTH, true, LAZY>(S, one.x, one.y, exc.x, exc.y, nonbinary, bid, wave, lane, scratch, slot_bytes, csize, flags, tag);
    }
}

// one launch of the coder with D candidates per one and, LZ, the lazy rule: the plane-input kernel (one workgroup per plane,
// its grid rounded up to whole groups of 128 = 64 blocks, for its XCD-aware order) or the int8-input one (one per block)
template <int D, bool LZ>
static void bp_launch(bool planes, const uint8_t *d_src, PlanesGeom pg, uint32_t n_blocks, uint8_t *d_scratch, uint64_t slot_bytes, uint32_t *d_csize,
                      uint32_t *d_flags, uint32_t tag, hipStream_t st)
{
    if (planes)
        hipLaunchKernelGGL((k_lz4_bitplanes_uni<D, LZ>), dim3((n_blocks + 63u) / 64u * 128u), dim3(64), 0, st, d_src, pg, n_blocks, d_scratch,
                           slot_bytes, d_csize, d_flags, tag, planes_div(pg));
    else
        hipLaunchKernelGGL((k_lz4_bitplanes<D, LZ>), dim3(n_blocks), dim3(128), 0, st, d_src, pg, n_blocks, d_scratch, slot_bytes, d_csize, d_flags, tag);
}

// depth: candidates per one; + 0x100: with the lazy rule (instantiated for 12 candidates — clevel 9 — and, for measurements, 2)
int launch_lz4_bitplanes(const uint8_t *d_src, bool planes, PlanesGeom pg, uint64_t n_blocks, uint8_t *d_scratch, size_t slot_bytes, uint32_t *d_csize,
                         int depth, uint32_t *d_flags, uint32_t tag, hipStream_t st)
{
    const bool lazy = (depth & 0x100) != 0;
    depth &= 0xFF;
    if (n_blocks == 0) return HHGT_OK;
    if (2u * n_blocks > 0x7fffff80ull) {   // (the plane-input grid: two workgroups per block, rounded up to whole groups of 128)
        hhgt_set_error("lz4: too many blocks");
        return HHGT_ERR_ARG;
    }
    // (planes_block32's reciprocals are exact for block ids below 2^31 — above — and divisors below 2^31)
    if (planes && (pg.bpr == 0 || (uint64_t)pg.S_pad * pg.bpr == 0 || (uint64_t)pg.S_pad * pg.bpr > 0x7fffffffull)) {
        hhgt_set_error("lz4: a chunk column of the planes must hold between 1 and 2^31 - 1 blocks");
        return HHGT_ERR_ARG;
    }
    const auto launch = lazy ? (depth == 2 ? bp_launch<2, true> : bp_launch<12, true>)
                        : depth <= 0 ? bp_launch<0, false>
                        : depth == 1 ? bp_launch<1, false>
                        : depth == 2 ? bp_launch<2, false>
                        : depth <= 4 ? bp_launch<4, false>
                        : depth <= 8 ? bp_launch<8, false>
                        : depth <= 12 ? bp_launch<12, false>
                                      : bp_launch<16, false>;
    launch(planes, d_src, pg, (uint32_t)n_blocks, d_scratch, (uint64_t)slot_bytes, d_csize, d_flags, tag, st);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
