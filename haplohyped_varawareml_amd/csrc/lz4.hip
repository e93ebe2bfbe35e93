// lz4.hip — Blosc byte-shuffle + LZ4 block encode, one Blosc block per workgroup (gfx950).
//
// Replaces the per-chunk work of the HDF5 filter the reference invokes at
//   create_dataset(..., compression=32001, compression_opts=(2,2,0,0,5,1,2))
//   /root/reference/src/haplohyped/vcf_to_h5.py:134-135
// i.e. c-blosc2's shuffle(typesize) -> split into `typesize` streams -> LZ4 block format per stream.
// The emitted bytes are a valid LZ4 block stream (not byte-identical to liblz4's: the contract is
// "decompresses to identical bytes"; tests/test_gpu_lz4_stream_pins.py holds them to what this coder wrote before).
//
// Workgroup = one block; wave j = stream j (byte plane j of the shuffled block when split).
//   phase A  all waves: coalesced 16 B/lane loads of the block, byte-plane de-interleave in registers
//            (v_perm_b32 for typesize 2), planes stored to LDS  -> shuffle costs no extra HBM traffic
//            (lz4_stage_*: one function per form of the source)
//   phase B  wave j: greedy LZ4 over its plane in LDS, 64 positions (one per lane) per window
//            (lz4_code_stream): every lane verifies and measures its own candidates — the hash table's
//            most recent occurrence and the offset-1 run; the greedy left-to-right choice of non-overlapping
//            matches is the only serial part and runs on the scalar unit; the chosen sequences are queued in LDS
//            and laid out (DPP prefix sum) and written one per lane, 48-64 at a time.
// Algorithmic bytes = blocksize read + compressed bytes written per block; measured: the kernel is bound by
// instruction issue, not by HBM (which also has the coder's history and what was tried and dropped).
#include "common.h"
#include <stdlib.h>

#define LZ_MINMATCH 4u
#define LZ_MFLIMIT 12u
#define LZ_LASTLITERALS 5u
// Shortest offset-1 run / hash match the window encoder takes as a sequence.  LZ4 allows 4; on the genotype workload
// a 4-5 byte match saves 1-2 bytes but ends the literal run and often pre-empts a better match one position later
// (the parse is greedy): measured ratio 4.326 with 4/4, 4.399 with 5/5, **4.410 with 6/6**, 4.352 with 7/7,
// 4.231 with 8/8 — and fewer sequences are less work.  Override with -DLZ_MINRUN= / -DLZ_MINHASH=.
#ifndef LZ_MINRUN
#define LZ_MINRUN 6u
#endif
#ifndef LZ_MINHASH
#define LZ_MINHASH 6u
#endif
#ifndef LZ_BACK_STEPS
#define LZ_BACK_STEPS 1   // backward-extension rounds of the long-run effort
#endif
// Bytes behind the end of every stream in LDS that are ZERO: the window encoder's lanes fetch the 24 bytes at positions
// up to mflimit + 63 = n + 51, i.e. they look at up to 76 bytes past the end of their stream.  Those positions are never
// coded, but what a lane in front of them measures (how far its hash candidate agrees, whether the offset-1 run or the
// hash match is the longer one before both are cut at the stream's match limit) decides between two equally valid
// encodings — with less slack than that the second wave of a workgroup looks at the first wave's live hash table
// there, and streams differ from run to run.
#define LZ_SLACK 96u
// Key length of the hash table.  12 bytes, not LZ4's 4: with a minimum match of 6 the short key only buys candidates that
// die early, and the most recent place where the next TWELVE bytes were the same is far more often the start of a long
// match (genotype planes: ratio 4.41 -> 5.12 and 2 % FASTER; 6 / 8 / 10 / 16 / 20 key bytes: 4.60 / 4.85 / 5.01 / 4.77 / 4.54).
#ifndef LZ_KEY
#define LZ_KEY 12
#endif

// how hard the stream coder looks (from clevel: lz4_effort).  The values only name the kernels: k_lz4_blocks takes the effort as an
// int, so an instantiation keeps the name (k_lz4_blocks<7, 6, false>) that tests/test_isa_guards.py and profiles/ know it by
enum LzEffort : int {
    LZ_RUN_ONLY = 5,   // the offset-1 run candidate only: no hash table, no LDS gathers (like LZ4's acceleration)
    LZ_HASH = 6,       // hash + run candidates: the default
    LZ_LONG_RUN = 7,   // plus the long-run source candidate, the backward extension and every long match finished
};

size_t lz4_slot_bytes(int neblock)
{
    size_t b = (size_t)neblock + (size_t)neblock / 255 + 16;
    return (b + 15) & ~(size_t)15;
}

// ---------------------------------------------------------------------------------------------
// The dynamic LDS of a workgroup, described once for the kernel's pointers, the host's occupancy search and the launch:
//   [data: nwaves streams, sstride apart, + 16][per wave a table of (1 << hashlog) + 2 u16 entries]
//   [8-aligned: per wave a queue of 64 sequences (uint2)]
// (32-bit on both sides: nwaves * sstride is at most an `int` blocksize plus 16 x 111 bytes of slack and alignment, the tables and
//  queues add under 150 KiB, so nothing wraps, and the launch refuses a total above 160 KiB - 64 before it is used)
struct LzLds {
    uint32_t data_bytes, tab_bytes /* per wave */, queue_off, total;
};
static inline __host__ __device__ LzLds lz4_lds_layout(uint32_t nwaves, uint32_t sstride, uint32_t hashlog)
{
    LzLds l;
    l.data_bytes = nwaves * sstride + 16u;
    l.tab_bytes = (2u << hashlog) + 4u;
    l.queue_off = (l.data_bytes + nwaves * l.tab_bytes + 7u) & ~7u;
    l.total = l.data_bytes + nwaves * l.tab_bytes + 8u + nwaves * 512u;   // (+ 8: room for the alignment)
    return l;
}

__device__ __forceinline__ uint32_t lds_load4(const uint8_t *in, uint32_t i)
{
    const uint32_t *w = reinterpret_cast<const uint32_t *>(in);
    uint32_t a = w[i >> 2], b = w[(i >> 2) + 1];
    return __builtin_amdgcn_alignbyte(b, a, i & 3u);
}

__device__ __forceinline__ uint32_t emit_len(uint8_t *out, uint32_t q, uint32_t rem, uint32_t lane)
{
    // LZ4 length extension: rem/255 bytes of 255, then rem%255
    uint32_t nb = rem / 255u + 1u;
    for (uint32_t j = lane; j < nb; j += 64u) out[q + j] = (j == nb - 1u) ? (uint8_t)(rem % 255u) : (uint8_t)255u;
    return q + nb;
}

// ---------------------------------------------------------------------------------------------
// helpers of the window-parallel encoder.
// A lane fetches the 24 bytes at its own position and the 24 bytes at its candidate as aligned dwords
// (ds_read2_b32 x 3 per side) and measures its match up to 20 bytes from registers.
// On unaligned LDS reads: gfx950 accepts ds_read_b32/b64/b128 at any byte address, which would remove every
// v_alignbyte below — but tools/micro/lds_unaligned.hip measures ~57 cycles per unaligned wave-instruction
// (lanes serialised, any width) against 3-5 aligned; the encoder built that way ran 3.3x slower.  Aligned
// dwords + v_alignbyte it is.
struct Own6 {
    uint32_t w[6];
};

__device__ __forceinline__ Own6 lds_load6(const uint8_t *in, uint32_t pos)
{
    const uint32_t *w = reinterpret_cast<const uint32_t *>(in) + (pos >> 2);
    Own6 o;
#pragma unroll
    for (int k = 0; k < 6; ++k) o.w[k] = w[k];
    return o;
}

__device__ __forceinline__ uint32_t div255(uint32_t x) { return (x * 0x8081u) >> 23; }  // exact for x < 65536

#ifdef HHGT_LZ4_STATS
// development build only (tools/lz4_stats.py): event counts of the window loop
//   0 streams  1 windows  2 windows without a candidate  4 matches finished cooperatively  5 ... past their first 64 bytes
//   6 flushes  7 sequences
__device__ unsigned long long g_lz4_stat[8];
#define LZ_STAT(i, v)                                                                \
    do {                                                                             \
        if ((threadIdx.x & 63u) == 0u) atomicAdd(&g_lz4_stat[i], (unsigned long long)(v)); \
    } while (0)
extern "C" int hhgt_debug_lz4_stats(unsigned long long *out8, int reset)
{
    if (out8 && hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_lz4_stat), sizeof(g_lz4_stat)) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[8] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_lz4_stat), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#else
#define LZ_STAT(i, v) ((void)0)
#endif

// Sensitivity probes (development builds only; empty otherwise): 16 extra independent scalar / vector instructions per
// window.  They cost +14 % / +6 % kernel time: a wave's own serial instruction stream is the limit.
__device__ __forceinline__ void lz4_probe_salu()
{
#ifdef LZ_PROBE_SALU
    asm volatile(".rept 16\n\ts_mov_b32 s100, 0\n\t.endr" ::: "s100");
#endif
}
__device__ __forceinline__ void lz4_probe_valu(uint32_t lane)
{
#ifdef LZ_PROBE_VALU
    uint32_t pv = lane;
    asm volatile(".rept 16\n\tv_add_u32 %0, 1, %0\n\t.endr" : "+v"(pv));
#else
    (void)lane;
#endif
}

// v_ffbl_b32: index of the lowest set bit, 0xFFFFFFFF for 0 (kept opaque so that min() folds stay one instruction)
__device__ __forceinline__ uint32_t ffbl(uint32_t x)
{
    uint32_t r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
// number of equal leading bytes (0..4) given x = a ^ b
__device__ __forceinline__ uint32_t eq_bytes(uint32_t x)
{
    const uint32_t t = ffbl(x) >> 3;  // x == 0 -> 0x1FFFFFFF
    return t < 4u ? t : 4u;
}
struct __attribute__((packed)) PackedU32 {
    uint32_t v;
};
__device__ __forceinline__ unsigned long long ballot(bool c) { return __builtin_amdgcn_ballot_w64(c); }
__device__ __forceinline__ bool in_mask(unsigned long long m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
__device__ __forceinline__ uint32_t next_lane(uint32_t v)   // lane + 1's value, 0 for lane 63 (DPP wave_shl:1)
{
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x130, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t lds_addr(const void *p)
{
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)p;
}

// ---------------------------------------------------------------------------------------------
// Emission.  Layout + bytes of the queued sequences, one per lane (lane j = j-th match in stream order).
// queue[j] = (pos | len << 16, offset).  Updates op (output size so far) and anchor (end of the last match).
__device__ __forceinline__ void lz4_flush_queue(const uint8_t *in, uint8_t *__restrict__ out, const uint2 *queue,
                                                uint32_t qn, uint32_t &op, uint32_t &anchor, uint32_t lane)
{
    const bool valid = lane < qn;
    const uint2 e = queue[lane];  // stale entries beyond qn are masked below
    const uint32_t pos = e.x & 0xFFFFu, len = e.x >> 16, off = e.y;
    const uint32_t endp = pos + len;
    const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)endp, 0x138, 0xf, 0xf, false);  // wave_shr:1
    const uint32_t prev_end = lane ? up : anchor;
    const uint32_t ll = valid ? pos - prev_end : 0u, mlc = len - LZ_MINMATCH;
    const uint32_t llx = ll >= 15u ? div255(ll - 15u) + 1u : 0u;
    const uint32_t mlx = (valid && mlc >= 15u) ? div255(mlc - 15u) + 1u : 0u;
    const uint32_t size = valid ? 3u + llx + ll + mlx : 0u;
    uint32_t total;
    const uint32_t so = op + wave_scan_sum_dpp(size, lane, &total) - size;
    if (valid) {
        const uint32_t token = ((ll < 15u ? ll : 15u) << 4) | (mlc < 15u ? mlc : 15u);
        const uint32_t q = so + 1u + llx + ll;
        out[so] = (uint8_t)token;
        out[so + (llx == 1u ? 1u : 0u)] = (uint8_t)(llx == 1u ? ll - 15u : token);
        out[q] = (uint8_t)(off & 0xFFu);
        out[q + 1u] = (uint8_t)(off >> 8);
        out[q + (mlx == 1u ? 2u : 1u)] = (uint8_t)(mlx == 1u ? mlc - 15u : off >> 8);
    }
    if (ballot((llx | mlx) > 1u) != 0ull) {  // rare: 255-runs
        if (valid && (llx | mlx) > 1u) {
            const uint32_t q = so + 1u + llx + ll;
            if (llx > 1u) {
                const uint32_t rem = ll - 15u;
                for (uint32_t k = 0; k < llx; ++k) out[so + 1u + k] = (k == llx - 1u) ? (uint8_t)(rem - 255u * (llx - 1u)) : (uint8_t)255u;
            }
            if (mlx > 1u) {
                const uint32_t rem = mlc - 15u;
                for (uint32_t k = 0; k < mlx; ++k) out[q + 2u + k] = (k == mlx - 1u) ? (uint8_t)(rem - 255u * (mlx - 1u)) : (uint8_t)255u;
            }
        }
    }
    // literals: short runs by their own lane, long runs (> 32 bytes: incompressible stretches) by the whole wave
    const uint32_t lit_dst = so + 1u + llx;
    unsigned long long big = ballot(ll > 32u);
    while (big) {
        const uint32_t j = (uint32_t)__ffsll((long long)big) - 1u;
        big &= big - 1ull;
        const uint32_t n_l = (uint32_t)__builtin_amdgcn_readlane((int)ll, (int)j);
        const uint32_t src = (uint32_t)__builtin_amdgcn_readlane((int)prev_end, (int)j);
        const uint32_t dst = (uint32_t)__builtin_amdgcn_readlane((int)lit_dst, (int)j);
        for (uint32_t k = lane; k < n_l; k += 64u) out[dst + k] = in[src + k];
    }
    // short runs: 4 bytes per step from two aligned LDS dwords; whole dwords go out as one (unaligned) global
    // store, the last 1-3 bytes one by one (the bytes after them belong to other lanes)
    const uint32_t lshort = ll > 32u ? 0u : ll;
    const uint32_t lsh = prev_end & 3u;
    for (uint32_t k = 0; ballot(k < lshort) != 0ull; k += 4u) {
        if (k < lshort) {
            const uint32_t *wsrc = reinterpret_cast<const uint32_t *>(in) + ((prev_end + k) >> 2);
            const uint32_t v = __builtin_amdgcn_alignbyte(wsrc[1], wsrc[0], lsh);
            const uint32_t rem = lshort - k;
            uint8_t *dstp = out + lit_dst + k;
            if (rem >= 4u) {
                reinterpret_cast<PackedU32 *>(dstp)->v = v;
            } else {
                dstp[0] = (uint8_t)v;
                if (rem > 1u) dstp[1] = (uint8_t)(v >> 8);
                if (rem > 2u) dstp[2] = (uint8_t)(v >> 16);
            }
        }
    }
    op += total;
    anchor = (uint32_t)__builtin_amdgcn_readlane((int)endp, (int)(qn - 1u));
}

// Enqueue: the lanes of SEL write their sequence behind the qn already queued, in lane (= stream) order.  Layout and
// emission then happen once per ~12 windows (lz4_flush_queue), one sequence per lane, instead of once per window with 4 of
// 64 lanes busy.  Runs under exec = SEL, set by two scalar moves instead of a per-lane test.
__device__ __forceinline__ void lz4_enqueue(uint32_t queue_lds, uint32_t qn, unsigned long long SEL, uint32_t pos, uint32_t len,
                                            uint32_t off)
{
    const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(SEL >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)SEL, 0u));
    const uint32_t addr = (queue_lds + qn * 8u) + slot * 8u;  // scalar base + lane slot
    const unsigned long long ent = (unsigned long long)(pos | (len << 16)) | ((unsigned long long)off << 32);
    unsigned long long saved;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\tds_write_b64 %2, %3\n\ts_mov_b64 exec, %0"
                 : "=&s"(saved)
                 : "s"(SEL), "v"(addr), "v"(ent)
                 : "memory");
}

// Last literals: everything behind the last match (anchor .. n), as the final sequence without a match.  -> stream size
__device__ __forceinline__ uint32_t lz4_last_literals(const uint8_t *in, uint8_t *__restrict__ out, uint32_t op, uint32_t anchor,
                                                      uint32_t n, uint32_t lane)
{
    const uint32_t ll = n - anchor;
    if (lane == 0) out[op] = (uint8_t)((ll < 15u ? ll : 15u) << 4);
    uint32_t q = op + 1u;
    if (ll >= 15u) q = emit_len(out, q, ll - 15u, lane);
    for (uint32_t k = lane; k < ll; k += 64u) out[q + k] = in[anchor + k];
    return q + ll;
}

// ---------------------------------------------------------------------------------------------
// Search: the phases of one window, in the order lz4_code_stream calls them.  The vector ALU is this kernel's bound (VALU
// issue slots > 85 % busy, LDS and the scalar unit have room: tools/pmc_lz4.sh), so per-lane predicates live as wave masks
// in SGPR pairs (v_cmp writes them for free) and are combined on the scalar unit, and everything wave-uniform (range limits,
// the position-0 exclusion, end-of-stream clipping) is scalar and branched around.  Phases take the window's values as
// plain scalars and hand their results back by value; a predicate never travels as a bool.

// Window advance.  What a lane holds of the window at p (pos = p + lane > 0): its six aligned dwords and the byte in front.
struct LzWindow {
    Own6 own;
    uint32_t pbv;
};
__device__ __forceinline__ LzWindow lz4_window_at(const uint8_t *in, uint32_t pos)
{
    LzWindow w;
    w.own = lds_load6(in, pos);
    w.pbv = (uint32_t)in[pos - 1u];
    return w;
}

// hash of the NB bytes at a lane's position (own = its six aligned dwords, sh = pos & 3, d = the first four bytes)
template <int NB>
__device__ __forceinline__ uint32_t lz4_key_hash(const Own6 &own, uint32_t sh, uint32_t d)
{
    if constexpr (NB <= 4) return d * 2654435761u;
    uint32_t kx = d;
    constexpr int rot[4] = {13, 7, 21, 27};
#pragma unroll
    for (int k = 1; k < (NB + 3) / 4; ++k) {
        uint32_t e = __builtin_amdgcn_alignbyte(own.w[k + 1], own.w[k], sh);
        if (k == (NB + 3) / 4 - 1 && (NB & 3)) e &= (1u << (8 * (NB & 3))) - 1u;   // key ends inside this dword
        kx ^= __builtin_amdgcn_alignbit(e, e, rot[k - 1]);
    }
    return kx * 2246822519u;
}

// Candidates.  Two per position: (a) the hash table's most recent occurrence of the LZ_KEY bytes at the position (not FAST),
// (b) offset 1 — the position continues a run of one byte value.  (b) needs no table and no LDS: E = ballot(byte[pos] ==
// byte[pos-1]) is one compare per window, and a lane's run length is the number of consecutive set bits of E from its own
// bit (exact up to the window end).  On sparse genotype planes (b) roughly halves what a zero run costs, because an
// earlier "0000" copy breaks wherever the EARLIER text had a 1.
// Reads own / pbv / d of the window, reads and updates tab.  Returns, per lane: run, the candidate (hcand, its six dwords cw,
// hsh = hcand & 3); as wave masks: E, Rm (run long enough), Hm (candidate agrees in its first four bytes), M = (Hm | Rm) &
// range_m, range_m (positions that may start a match: not position 0, not past mflimit).
struct LzCand {
    uint32_t run, hcand, hsh;
    Own6 cw;
    unsigned long long E, Rm, Hm, M, range_m;
};
template <bool FAST>
__device__ __forceinline__ LzCand lz4_candidates(const uint8_t *in, uint16_t *tab, uint32_t hshift, const Own6 &own, uint32_t pbv,
                                                 uint32_t d, uint32_t p, uint32_t pos, uint32_t sh, uint32_t lane, uint32_t to_end,
                                                 uint32_t lim63, uint32_t mflimit)
{
    LzCand c;
    c.hcand = 0u;
    c.hsh = 0u;
    c.cw = Own6{};   // (FAST has no candidate dwords; the struct is returned whole)
    if constexpr (!FAST) {
        // positions past mflimit are inserted too: only the last window has them and nothing reads
        // the table after it
        const uint32_t h = lz4_key_hash<LZ_KEY>(own, sh, d) >> hshift;
        c.hcand = (uint32_t)tab[h];
        tab[h] = (uint16_t)pos;
        c.cw = lds_load6(in, c.hcand);
        c.hsh = c.hcand & 3u;
    }
    c.E = ballot((d & 0xFFu) == pbv);
    const unsigned long long r = ~c.E >> lane;  // first set bit = end of this lane's run (none: the window end)
    const uint32_t f_lo = ffbl((uint32_t)r), f_hi = ffbl((uint32_t)(r >> 32)) | 32u;
    const uint32_t f = f_lo < f_hi ? f_lo : f_hi;
    c.run = f < to_end ? f : to_end;
    c.Rm = ballot(c.run >= LZ_MINRUN);
    c.Hm = 0ull;
    if constexpr (!FAST) c.Hm = ballot(d == __builtin_amdgcn_alignbyte(c.cw.w[1], c.cw.w[0], c.hsh));
    // the table starts zeroed, so hcand < pos except at position 0; candidates need no range test:
    // position 0 and lanes past mflimit are taken out of M on the scalar side, in the two windows that have them
    c.M = c.Hm | c.Rm;
    c.range_m = ~0ull;
    if (p - 1u >= lim63) {
        asm volatile("" ::: "memory");  // keep this a (rarely taken) scalar branch
        if (p == 0u) c.range_m &= ~1ull;
        if (p + 63u > mflimit) c.range_m &= ~0ull >> (63u - (mflimit - p));
        c.M &= c.range_m;
    }
    return c;
}

// Measure.  The four xor dwords of bytes 4..19 at the lane's position and at its candidate.  Returns lenh = equal bytes
// (4..20) for the lanes of Hm, 0 for the others, and Zm = lanes whose 20 bytes all agree ("still matching").
struct LzMeasure {
    uint32_t lenh;
    unsigned long long Zm;
};
__device__ __forceinline__ LzMeasure lz4_measure(const Own6 &own, uint32_t sh, const Own6 &cw, uint32_t hsh, unsigned long long Hm)
{
    const uint32_t x1 = __builtin_amdgcn_alignbyte(own.w[2], own.w[1], sh) ^ __builtin_amdgcn_alignbyte(cw.w[2], cw.w[1], hsh);
    const uint32_t x2 = __builtin_amdgcn_alignbyte(own.w[3], own.w[2], sh) ^ __builtin_amdgcn_alignbyte(cw.w[3], cw.w[2], hsh);
    const uint32_t x3 = __builtin_amdgcn_alignbyte(own.w[4], own.w[3], sh) ^ __builtin_amdgcn_alignbyte(cw.w[4], cw.w[3], hsh);
    const uint32_t x4 = __builtin_amdgcn_alignbyte(own.w[5], own.w[4], sh) ^ __builtin_amdgcn_alignbyte(cw.w[5], cw.w[4], hsh);
    // equal bytes of x1..x4: the first non-zero dword decides (all zero: 16 + 4 = 20, still matching)
    const uint32_t t1 = x1 ? x1 : (x2 ? x2 : (x3 ? x3 : x4));
    const uint32_t skip = x1 ? 4u : (x2 ? 8u : (x3 ? 12u : 16u));
    const uint32_t lraw = skip + eq_bytes(t1);
    LzMeasure m;
    m.lenh = in_mask(Hm) ? lraw : 0u;
    m.Zm = ballot((x1 | x2 | x3 | x4) == 0u);
    return m;
}

// The hash-side candidate of a lane as the two LZ_LONG_RUN phases rewrite it: length, source, and the masks that follow it
struct LzHashCand {
    uint32_t lenh, hcand;
    unsigned long long Hm, M, Zm;
};
// the wave's longest extended run of one byte value so far (bytes start .. start + len - 1; byte 0x100: none yet); scalar
struct LzBestRun {
    uint32_t start, len, byte;
};

// Long-run source candidate (LZ_LONG_RUN).  The first byte of a run (it differs from its predecessor, so offset 1 cannot
// cover it) copied together with the run from the LONGEST EARLIER RUN of the same byte value.  The hash table's most recent
// "0000" sits at the end of the previous run, four bytes before the '1' that ends it — a source that dies after 4 bytes;
// LZ4HC's chain search finds the long one, which is why c-blosc's lz4hc (what the reference's compression_opts select)
// packs these planes far tighter than lz4.
// Reads d, r1 (the run behind the lane: lane + 1's lenr), E, Rm, range_m and the best run.  Returns the hash-side candidate
// with the lanes Lm, where the long source beats it, rewritten; those are "still matching" if the run reaches the window
// end and the source run is longer than that.
__device__ __forceinline__ LzHashCand lz4_long_run_source(uint32_t lenh, uint32_t hcand, unsigned long long Hm, unsigned long long M,
                                                          unsigned long long Zm, uint32_t d, uint32_t r1, unsigned long long E,
                                                          unsigned long long Rm, unsigned long long range_m, uint32_t to_end,
                                                          uint32_t best_start, uint32_t best_len, uint32_t best_byte)
{
    const unsigned long long Lm0 = ballot((d & 0xFFu) == best_byte) & ~E & (Rm >> 1) & range_m;
    if (Lm0 != 0ull) {
        const uint32_t want = r1 + 1u;                                    // this byte + the run behind it
        const uint32_t lenl = want < best_len ? want : best_len;
        const unsigned long long Lm = Lm0 & ballot(lenl > lenh);
        const bool isl = in_mask(Lm);
        lenh = isl ? lenl : lenh;
        hcand = isl ? best_start : hcand;
        Hm |= Lm;
        M |= Lm;
        Zm = (Zm & ~Lm) | (Lm & ballot(want == to_end) & ballot(best_len > want));
    }
    return LzHashCand{lenh, hcand, Hm, M, Zm};
}

// Backward extension (LZ_LONG_RUN, LZ_BACK_STEPS rounds).  Every candidate is tried one byte to the left as its left
// neighbour's candidate (LZ4HC's backward extension, lane-parallel): if the byte in front of lane + 1's source equals this
// lane's byte, this lane has a match one byte longer from one byte earlier.  That turns "1, then 0 0 0 ... from the long
// run" into one match with no literal, and lengthens ordinary hash matches found one position late.
// Reads d, range_m and one byte of the text per round.  Returns the hash-side candidate with the lanes Bm rewritten.
__device__ __forceinline__ LzHashCand lz4_extend_back(const uint8_t *in, uint32_t lenh, uint32_t hcand, unsigned long long Hm,
                                                      unsigned long long M, unsigned long long Zm, uint32_t d, unsigned long long range_m)
{
#pragma unroll
    for (int step = 0; step < LZ_BACK_STEPS; ++step) {
        const uint32_t nh = next_lane(hcand);   // lane+1's source
        const uint32_t nl = next_lane(lenh);    // ... and length
        const uint32_t pbyte = (uint32_t)in[nh ? nh - 1u : 0u];
        const unsigned long long Bm = ballot(nl + 1u > lenh) & ballot(nh != 0u) & ballot((d & 0xFFu) == pbyte) & (Hm >> 1) & range_m;
        if (Bm != 0ull) {
            const bool isb = in_mask(Bm);
            lenh = isb ? nl + 1u : lenh;
            hcand = isb ? nh - 1u : hcand;
            Hm |= Bm;
            M |= Bm;
            Zm = (Zm & ~Bm) | (Bm & (Zm >> 1));
        }
    }
    return LzHashCand{lenh, hcand, Hm, M, Zm};
}

// Run-dominance rule and minimum hash length.  A hash match that starts 1 or 2 bytes before a run and ends inside it is a bad
// buy: "match, then the rest of the run" is two sequences (>= 6 bytes) where "1-2 literals, then the whole run" is one
// (<= 5).  On sparse genotype planes that is every '1' followed by zeros (the typical window): such candidates are
// dropped, and with them the reason to measure hash matches past 20 bytes.
// Reads lenh, r1 / r2 (the runs that start one / two lanes on), Rm.  Returns Hm without the dominated and the too short,
// M without those of them that have no run of their own, lenh zeroed outside the new Hm.
struct LzKept {
    uint32_t lenh;
    unsigned long long Hm, M;
};
__device__ __forceinline__ LzKept lz4_drop_dominated(uint32_t lenh, unsigned long long Hm, unsigned long long M, unsigned long long Rm,
                                                     uint32_t r1, uint32_t r2)
{
    const unsigned long long DOMm = (ballot(r1 + 1u > lenh) & (Rm >> 1)) | (ballot(r2 + 2u > lenh) & (Rm >> 2));  // Rm >> k: lane + k starts a run
    const unsigned long long drop = Hm & (DOMm | ballot(lenh < LZ_MINHASH)) & ~Rm;  // lanes with a run of their own stay candidates
    Hm &= ~(DOMm | ballot(lenh < LZ_MINHASH));
    M &= ~drop;
    return LzKept{in_mask(Hm) ? lenh : 0u, Hm, M};
}

// Choice.  Per lane the longer of run and hash match; ties go to the run (offset 1: the cheaper continuation, and the one
// lz4_long_run_source learns from).  Returns len and off per lane; RFm = chosen runs that reach the window end; LNG = RFm and
// the hash matches alive after 20 bytes ("still matching": finished cooperatively if selected), both clipped where the
// stream ends.
struct LzChoice {
    uint32_t len, off;
    unsigned long long RFm, LNG;
};
__device__ __forceinline__ LzChoice lz4_choose(uint32_t lenr, uint32_t lenh, uint32_t hcand, unsigned long long Hm, unsigned long long Zm,
                                               uint32_t p, uint32_t pos, uint32_t to_end, uint32_t matchlimit)
{
    LzChoice c;
    const unsigned long long URm = ballot(lenr >= lenh);
    c.len = lenr > lenh ? lenr : lenh;
    c.off = in_mask(URm) ? 1u : pos - hcand;
    c.RFm = URm & ballot(lenr == to_end);
    const unsigned long long MOREm = Hm & Zm & ~URm;
    c.LNG = c.RFm | MOREm;
    if (p + 100u > matchlimit) {  // only the last windows of a stream can reach the end-of-block limits
        asm volatile("" ::: "memory");
        const uint32_t maxlen = matchlimit - pos;  // lanes past matchlimit are not in M
        c.LNG &= ballot(c.len < maxlen);           // clipped at the end of the stream: not "long"
        c.len = c.len < maxlen ? c.len : maxlen;
    }
    return c;
}

// ---------------------------------------------------------------------------------------------
// Parse.  The greedy left-to-right choice of non-overlapping matches among the lanes of M: the only serial part, on the
// scalar unit (8 scalar instructions + one v_readlane per match).  Starts at the first lane of mrest, adds lanes to SEL, and
// stops at the match that ends past the window or (STOP_AT_LNG) at a selected lane of LNG.  Writes SEL, mrest, last = the lane
// it stopped on and lcur = where that lane's match ends (window-relative) in the caller's variables: handed back as a struct,
// the selection loop of the long-run effort had three scalar instructions more per finished match and the stage ran 2.4 % slower.
// ("+&s": the loop rewrites m while it still needs M — without the early-clobber mark the two, equal on entry, may be given
//  the same register pair)
#define LZ_PARSE_LOOP(AT_LNG)                      \
    "1:\n\t"                                       \
    "s_ff1_i32_b64 %[last], %[m]\n\t"              \
    "s_bitset1_b64 %[sel], %[last]\n\t"            \
    "v_readlane_b32 %[lcur], %[len], %[last]\n\t"  \
    "s_add_i32 %[lcur], %[lcur], %[last]\n\t"      \
    AT_LNG                                         \
    "s_cmp_gt_u32 %[lcur], 63\n\t"                 \
    "s_cbranch_scc1 2f\n\t"                        \
    "s_lshl_b64 %[m], -1, %[lcur]\n\t"             \
    "s_and_b64 %[m], %[m], %[M]\n\t"               \
    "s_cbranch_scc1 1b\n"                          \
    "2:"
#define LZ_PARSE_STOP_AT_LNG "s_bitcmp1_b64 %[lng], %[last]\n\ts_cbranch_scc1 2f\n\t"
template <bool STOP_AT_LNG>
__device__ __forceinline__ void lz4_greedy_parse(unsigned long long &SEL, unsigned long long &mrest, uint32_t &last, uint32_t &lcur,
                                                 unsigned long long M, uint32_t len, unsigned long long LNG)
{
    if constexpr (STOP_AT_LNG)
        asm volatile(LZ_PARSE_LOOP(LZ_PARSE_STOP_AT_LNG)
                     : [sel] "+&s"(SEL), [m] "+&s"(mrest), [last] "=&s"(last), [lcur] "=&s"(lcur)
                     : [M] "s"(M), [len] "v"(len), [lng] "s"(LNG)
                     : "scc");
    else
        asm volatile(LZ_PARSE_LOOP("")
                     : [sel] "+&s"(SEL), [m] "+&s"(mrest), [last] "=&s"(last), [lcur] "=&s"(lcur)
                     : [M] "s"(M), [len] "v"(len)
                     : "scc");
}

// Cooperative finish of a selected match that is still matching after ml bytes (ps = its position, c = its source; room
// to matchlimit > 0: a match that reached it is not in LNG).  Most tails are short: first the next 64 bytes, one per lane;
// a long run then goes on in steps of 256, four bytes per lane.  -> the match's whole length
__device__ __forceinline__ uint32_t lz4_finish_match(const uint8_t *in, uint32_t ps, uint32_t c, uint32_t ml, uint32_t lane,
                                                     uint32_t matchlimit)
{
    const uint32_t kb = ml + lane;
    const uint32_t room = matchlimit - (ps + ml);
    const unsigned long long neb = ballot(in[ps + kb] != in[c + kb]) | (room < 64u ? ~0ull << room : 0ull);
    if (neb != 0ull) {
        ml += (uint32_t)__ffsll((long long)neb) - 1u;
    } else {
        LZ_STAT(5, 1);
        ml += 64u;
        for (;;) {
            const uint32_t k = ml + 4u * lane;
            uint32_t nm = 0u;
            if (ps + k < matchlimit) {
                nm = eq_bytes(lds_load4(in, ps + k) ^ lds_load4(in, c + k));
                const uint32_t room = matchlimit - (ps + k);
                nm = nm < room ? nm : room;
            }
            const unsigned long long stop = ballot(nm < 4u);
            if (stop == 0ull) {
                ml += 256u;
                continue;
            }
            const uint32_t f2 = (uint32_t)__ffsll((long long)stop) - 1u;
            ml += 4u * f2 + (uint32_t)__builtin_amdgcn_readlane((int)nm, (int)f2);
            break;
        }
    }
    return ml;   // (one exit: with an early return behind the 64-byte look every instantiation has 3 scalar instructions more)
}

// Selection of a window's sequences: the parse, and the finish of what it stops on.  A match that is still matching after
// its per-lane cap is finished cooperatively: in the default mode only the window's last selected match (the parse ends
// on it), under LONGRUN every selected one — a capped match is NOT followed by its own continuation (the next candidate is
// the most recent place with the next 12 bytes, usually somewhere else), so each cut costs a sequence (+3.9 % ratio for
// +15 % time).  Under LONGRUN a finished run that is the wave's longest becomes `best`.
// Returns SEL, the lengths with the finished ones in their lanes, and lcur = the end of the last match (window-relative).
struct LzSelected {
    unsigned long long SEL;
    uint32_t len, lcur;
    LzBestRun best;
};
template <bool LONGRUN>
__device__ __forceinline__ LzSelected lz4_select(const uint8_t *in, unsigned long long M, unsigned long long LNG, unsigned long long RFm,
                                                 uint32_t len, uint32_t off, uint32_t d, uint32_t p, uint32_t lane, uint32_t matchlimit,
                                                 uint32_t best_start, uint32_t best_len, uint32_t best_byte)
{
    unsigned long long SEL = 0ull, mrest = M;
    uint32_t lcur, last;
    LzBestRun best = {best_start, best_len, best_byte};
    for (;;) {
        lz4_greedy_parse<LONGRUN>(SEL, mrest, last, lcur, M, len, LNG);
        if (!((LNG >> last) & 1ull)) break;
        LZ_STAT(4, 1);
        const uint32_t at = p + last;
        const uint32_t ml = lz4_finish_match(in, at, at - (uint32_t)__builtin_amdgcn_readlane((int)off, (int)last), lcur - last, lane, matchlimit);
        len = lane == last ? ml : len;
        lcur = last + ml;
        if (LONGRUN && ((RFm >> last) & 1ull) && ml + 1u > best.len) {  // a longer run of one byte value: bytes at-1 .. at+ml-1
            best.len = ml + 1u;
            best.start = at - 1u;
            best.byte = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)last) & 0xFFu;
        }
        if (!LONGRUN || lcur >= 64u) break;   // (default mode: that was the window's last match)
        mrest = M & (~0ull << lcur);
        if (mrest == 0ull) break;
    }
    return LzSelected{SEL, len, lcur, best};
}

// ---------------------------------------------------------------------------------------------
// One stream: in[0 .. n) in LDS (LZ_SLACK zero bytes behind it) -> LZ4 block format at out.  -> compressed size
// tab: this wave's hash table; queue: its 64 sequence slots.  The driver: table clear, the windows' phases in order,
// the final flush, the last literals.
template <LzEffort EFFORT>
__device__ __forceinline__ uint32_t lz4_code_stream(const uint8_t *in, uint32_t n, uint16_t *tab, uint32_t hashlog,
                                                    uint8_t *__restrict__ out, uint2 *queue)
{
    constexpr bool FAST = EFFORT == LZ_RUN_ONLY, LONGRUN = EFFORT == LZ_LONG_RUN;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t i = lane; i < (1u << hashlog) / 2u + 1u; i += 64u) reinterpret_cast<uint32_t *>(tab)[i] = 0u;
    const uint32_t to_end = 64u - lane;
    const uint32_t queue_lds = lds_addr(queue);
    uint32_t op = 0, anchor = 0, qn = 0;
    if (n > LZ_MFLIMIT) {
        const uint32_t mflimit = n - LZ_MFLIMIT, matchlimit = n - LZ_LASTLITERALS;
        const uint32_t hshift = 32u - hashlog;
        const uint32_t lim63 = mflimit - 63u;  // p - 1 >= lim63 (unsigned) <=> p == 0 or p + 63 > mflimit
        uint32_t p = 0;
        LzWindow w;
        w.own = lds_load6(in, lane);
        w.pbv = lane ? (uint32_t)in[lane - 1u] : 0x100u;   // 0x100 = "none": position 0 continues no run
        LzBestRun best = {0u, 0u, 0x100u};
        LZ_STAT(0, 1);
        while (p <= mflimit) {
            LZ_STAT(1, 1);
            const uint32_t pos = p + lane;
            const uint32_t sh = pos & 3u;
            const uint32_t d = __builtin_amdgcn_alignbyte(w.own.w[1], w.own.w[0], sh);
            const LzCand c = lz4_candidates<FAST>(in, tab, hshift, w.own, w.pbv, d, p, pos, sh, lane, to_end, lim63, mflimit);
            unsigned long long M = c.M;
            if (M == 0ull) {
                LZ_STAT(2, 1);
                p += 64u;
                w = lz4_window_at(in, p + lane);
                continue;
            }
            uint32_t lenh = 0u, hcand = c.hcand;
            unsigned long long Hm = c.Hm, Zm = 0ull;
            if constexpr (!FAST) {
                const LzMeasure m = lz4_measure(w.own, sh, c.cw, c.hsh, Hm);
                lenh = m.lenh;
                Zm = m.Zm;
            }
            const uint32_t lenr = in_mask(c.Rm) ? c.run : 0u;
            if constexpr (!FAST) {
                const uint32_t r1 = next_lane(lenr), r2 = next_lane(r1);
                if constexpr (LONGRUN) {
                    const LzHashCand l = lz4_long_run_source(lenh, hcand, Hm, M, Zm, d, r1, c.E, c.Rm, c.range_m, to_end, best.start,
                                                             best.len, best.byte);
                    const LzHashCand b = lz4_extend_back(in, l.lenh, l.hcand, l.Hm, l.M, l.Zm, d, c.range_m);
                    lenh = b.lenh, hcand = b.hcand, Hm = b.Hm, M = b.M, Zm = b.Zm;
                }
                const LzKept k = lz4_drop_dominated(lenh, Hm, M, c.Rm, r1, r2);
                lenh = k.lenh, Hm = k.Hm, M = k.M;
                if (M == 0ull) {
                    p += 64u;
                    w = lz4_window_at(in, p + lane);
                    continue;
                }
            }
            const LzChoice ch = lz4_choose(lenr, lenh, hcand, Hm, Zm, p, pos, to_end, matchlimit);
            const LzSelected s = lz4_select<LONGRUN>(in, M, ch.LNG, ch.RFm, ch.len, ch.off, d, p, lane, matchlimit, best.start, best.len, best.byte);
            best = s.best;
            // the next window's own bytes are requested here and consumed after the enqueue
            const uint32_t np = p + (s.lcur > 64u ? s.lcur : 64u);
            lz4_probe_salu();
            lz4_probe_valu(lane);
            const LzWindow nw = lz4_window_at(in, np + lane);
            lz4_enqueue(queue_lds, qn, s.SEL, pos, s.len, ch.off);
            qn += (uint32_t)__popcll(s.SEL);
            LZ_STAT(7, __popcll(s.SEL));
            if (qn > 48u) {
                LZ_STAT(6, 1);
                lz4_flush_queue(in, out, queue, qn, op, anchor, lane);
                qn = 0u;
            }
            p = np;
            w = nw;
        }
    }
    if (qn) lz4_flush_queue(in, out, queue, qn, op, anchor, lane);
    return lz4_last_literals(in, out, op, anchor, n, lane);
}

// ---------------------------------------------------------------------------------------------
// Staging (phase A): the block's bytes, shuffled, into LDS — plane j at data + j * pstride.  One function per form of
// the source; all threads of the workgroup take part.

// the block exists as bit planes (include/hhgt.h "Bit-plane form"; typesize 2, 8 KiB blocks): the shuffled byte
// planes are generated from the bits; bytes of calls beyond 0 / 1 / missing come from their place in the int8 block blk
__device__ __forceinline__ void lz4_stage_planes(const uint8_t *__restrict__ planes, const PlanesGeom &pg, uint32_t bid, bool have_bytes,
                                                 const uint8_t *blk, uint8_t *data, uint32_t pstride)
{
    uint64_t pcol;
    uint32_t prow, pbi;
    planes_block(pg, bid, &pcol, &prow, &pbi);
    const uint64_t kst = (uint64_t)pg.S_pad * 32ull;   // bytes between the kind-planes of a tile
    for (uint32_t i = threadIdx.x; i < 512u; i += blockDim.x) {   // byte i of each plane = variants 8 i .. 8 i + 7
        const uint8_t *pl = planes + planes_piece(pg, pcol, pbi * 16u + (i >> 5), 0u, prow) + (i & 31u);
        const uint32_t o[2] = {pl[0], pl[kst]}, e[2] = {pl[2ull * kst], pl[3ull * kst]};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            uint32_t w[2] = {0u, 0u};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                uint32_t v = (o[h] >> k) & 1u;
                if ((e[h] >> k) & 1u) v = v ? 0xF7u : (have_bytes ? (uint32_t)blk[(8u * i + (uint32_t)k) * 2u + (uint32_t)h] : 0u);
                w[k >> 2] |= v << (8 * (k & 3));
            }
            *reinterpret_cast<uint2 *>(data + (uint32_t)h * pstride + 8u * i) = make_uint2(w[0], w[1]);
        }
    }
}

// typesize 1: a copy, 16 bytes per lane where source and size allow
__device__ __forceinline__ void lz4_stage_bytes(const uint8_t *blk, uint32_t bsize, uint8_t *data)
{
    for (uint32_t i = threadIdx.x * 16u; i < bsize; i += blockDim.x * 16u) {
        if (i + 16u <= bsize && ((reinterpret_cast<uintptr_t>(blk + i) & 15u) == 0))
            *reinterpret_cast<uint4 *>(data + i) = *reinterpret_cast<const uint4 *>(blk + i);
        else
            for (uint32_t j = i; j < bsize && j < i + 16u; ++j) data[j] = blk[j];
    }
}

// typesize 2, whole 16-byte pieces from an aligned source: eight elements per lane, de-interleaved by v_perm_b32
__device__ __forceinline__ void lz4_stage_pairs(const uint8_t *blk, uint32_t bsize, uint8_t *data, uint32_t pstride)
{
    for (uint32_t i = threadIdx.x * 16u; i < bsize; i += blockDim.x * 16u) {
        uint4 v = *reinterpret_cast<const uint4 *>(blk + i);
        uint32_t p0a = __builtin_amdgcn_perm(v.y, v.x, 0x06040200u), p0b = __builtin_amdgcn_perm(v.w, v.z, 0x06040200u);
        uint32_t p1a = __builtin_amdgcn_perm(v.y, v.x, 0x07050301u), p1b = __builtin_amdgcn_perm(v.w, v.z, 0x07050301u);
        *reinterpret_cast<uint2 *>(data + (i >> 1)) = make_uint2(p0a, p0b);
        *reinterpret_cast<uint2 *>(data + pstride + (i >> 1)) = make_uint2(p1a, p1b);
    }
}

// any typesize: byte by byte; the bytes behind the last whole element follow the last plane
__device__ __forceinline__ void lz4_stage_shuffle(const uint8_t *blk, uint32_t bsize, uint32_t typesize, uint32_t nelem, uint8_t *data,
                                                  uint32_t pstride)
{
    const uint32_t body = nelem * typesize;
    for (uint32_t i = threadIdx.x; i < bsize; i += blockDim.x) {
        uint8_t v = blk[i];
        if (i < body) {
            uint32_t e = i / typesize, j = i - e * typesize;
            data[j * pstride + e] = v;
        } else
            data[(typesize - 1u) * pstride + nelem + (i - body)] = v;  // tail after the last plane
    }
}

// LZ_SLACK: what the lanes see behind the end of a stream is zeros, not a neighbour's table or a previous block
__device__ __forceinline__ void lz4_clear_slack(uint8_t *data, uint32_t nstreams, uint32_t pstride, uint32_t neblock)
{
    const uint32_t w_ = threadIdx.x >> 6;
    if (w_ < nstreams)
        for (uint32_t k = threadIdx.x & 63u; k < LZ_SLACK; k += 64u) data[(size_t)w_ * pstride + neblock + k] = 0;
}

// Scan mode: which of the 64 blocks from b0 still hold a stream the bit-plane coder (lz4bits.hip) left marked
// (csize == 0xFFFFFFFF).  Every wave of the workgroup reads the same sizes and gets the same mask.
__device__ __forceinline__ unsigned long long lz4_marked_blocks(const uint32_t *__restrict__ csize, uint32_t b0, uint32_t n_total,
                                                                uint32_t nwaves)
{
    const uint32_t bb = b0 + (threadIdx.x & 63u);
    bool any = false;
    if (bb < n_total)
        for (uint32_t j = 0; j < nwaves; ++j) any = any || csize[(uint64_t)bb * nwaves + j] == 0xFFFFFFFFu;
    return __builtin_amdgcn_ballot_w64(any);
}

// grid = n_chunks * nblocks (scan mode: a fixed grid); block = 64 * nwaves (nwaves = typesize when blocks are split, else 1)
// dynamic LDS: lz4_lds_layout
// MW = minimum waves per SIMD the register allocator must leave room for (0: no constraint, workgroups of up
// to 16 waves for typesize 16).  The common genotype case (typesize 2 -> 2-wave workgroups) is latency bound,
// so it is compiled for 7 resident waves per SIMD (8 at the fastest effort, <= 64 VGPRs).
// PLANES: the blocks exist as bit planes (phase A generates the bytes); a template parameter so that the int8
// instantiations keep their registers (the default one sits at the 72-register line of 7 waves per SIMD)
// Two modes.  Direct (mark_flag == nullptr): workgroup = block blockIdx.x, every stream is coded.  Scan (mark_flag set): the
// bit-plane coder ran first; its word says whether it left anything (it holds this call's tag if so), and only the streams
// it left marked are coded: the grid scans the stream sizes, 64 blocks per load, and works on the blocks that still hold one.
template <int MW, int EFFORT, bool PLANES>
__global__ __launch_bounds__(MW ? 128 : 1024, MW ? MW : 1) void k_lz4_blocks(const uint8_t *__restrict__ src, uint32_t nblocks,
                                                     uint64_t chunk_nbytes, uint32_t typesize, uint32_t blocksize,
                                                     uint32_t split, uint32_t sstride, uint32_t hashlog,
                                                     uint8_t *__restrict__ scratch, uint64_t slot_bytes,
                                                     uint32_t *__restrict__ csize, uint32_t n_total, const uint8_t *__restrict__ planes,
                                                     PlanesGeom pg, const uint32_t *__restrict__ mark_flag, uint32_t tag)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t nwaves = blockDim.x >> 6;
    const bool scan = mark_flag != nullptr;
    if (scan && __builtin_nontemporal_load(mark_flag) != tag) return;
    for (uint32_t b0 = scan ? blockIdx.x * 64u : blockIdx.x; b0 < (scan ? n_total : blockIdx.x + 1u); b0 += scan ? gridDim.x * 64u : 1u) {
        unsigned long long todo = scan ? lz4_marked_blocks(csize, b0, n_total, nwaves) : 1ull;   // direct: the one block
        while (todo != 0ull) {   // (workgroup-uniform)
            const uint32_t bid = scan ? b0 + (uint32_t)__builtin_ctzll(todo) : b0;
            todo &= todo - 1ull;
            // wave index through readfirstlane: everything derived from it (stream base, output slot) stays in SGPRs,
            // so the byte stores below use the SGPR-base + 32-bit-offset addressing form
            const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
            const uint64_t chunk = bid / nblocks;
            const uint32_t b = bid - (uint32_t)(chunk * nblocks);
            const uint64_t boff = (uint64_t)b * blocksize;
            const uint32_t bsize = (uint32_t)(chunk_nbytes - boff < blocksize ? chunk_nbytes - boff : blocksize);
            const bool leftover = bsize != blocksize;
            const uint32_t nstreams = (split && !leftover) ? typesize : 1u;
            const uint32_t nelem = bsize / typesize;
            const uint32_t neblock = bsize / nstreams;
            // plane stride in LDS: split streams are padded apart; a single stream keeps Blosc's contiguous
            // shuffled image [plane 0 | plane 1 | ... | tail]
            const uint32_t pstride = nstreams > 1u ? sstride : nelem;
            const LzLds L = lz4_lds_layout(nwaves, sstride, hashlog);
            uint8_t *data = smem;
            const uint8_t *blk = src + chunk * chunk_nbytes + boff;

            // ---- phase A: load + byte-shuffle into LDS
            if (PLANES)
                lz4_stage_planes(planes, pg, bid, src != nullptr, blk, data, pstride);
            else if (typesize == 1u)
                lz4_stage_bytes(blk, bsize, data);
            else if (typesize == 2u && (bsize & 15u) == 0u && (pstride & 7u) == 0u && ((reinterpret_cast<uintptr_t>(blk) & 15u) == 0))
                lz4_stage_pairs(blk, bsize, data, pstride);
            else
                lz4_stage_shuffle(blk, bsize, typesize, nelem, data, pstride);
            lz4_clear_slack(data, nstreams, pstride, neblock);
            __syncthreads();

            // ---- phase B: one wave per stream
            // (the stream index is formed in each branch, not once in front of them: hoisted, the PLANES instantiations code
            //  every block 0.3 % slower, profiles/r10_lz4_isa.txt)
            if (scan && csize[(uint64_t)bid * nwaves + wave] != 0xFFFFFFFFu) {
                // this stream of the block was coded by the bit-plane encoder
            } else if (wave < nstreams) {
                const uint8_t *in = data + (size_t)wave * pstride;
                const uint64_t sidx = (uint64_t)bid * nwaves + wave;
                uint8_t *out = scratch + sidx * slot_bytes;
                uint16_t *tab = reinterpret_cast<uint16_t *>(smem + L.data_bytes + wave * L.tab_bytes);
                uint2 *queue = reinterpret_cast<uint2 *>(smem + L.queue_off) + wave * 64u;   // (offset arithmetic keeps the LDS address space)
                uint32_t cs = lz4_code_stream<(LzEffort)EFFORT>(in, neblock, tab, hashlog, out, queue);
                if (cs >= neblock) {  // incompressible: Blosc stores the (shuffled) stream verbatim
                    for (uint32_t k = lane; k < neblock; k += 64u) out[k] = in[k];
                    cs = neblock;
                }
                if (lane == 0) csize[sidx] = cs;
            } else if (lane == 0) {
                csize[(uint64_t)bid * nwaves + wave] = 0u;
            }
            if (scan) __syncthreads();   // the next marked block reuses the LDS
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Launch.

static LzEffort lz4_effort(int clevel)   // clevel 1-2 / 3-6 (the default 5) / 7-9
{
    return clevel <= 2 ? LZ_RUN_ONLY : clevel >= 7 ? LZ_LONG_RUN : LZ_HASH;
}

// The bit-plane encoder (lz4bits.hip) takes the case the path is built for — typesize 2, 8 KiB blocks — and marks the
// streams it cannot code (calls beyond 0 / 1 / missing, with int8 input any byte > 1, very dense planes); k_lz4_blocks then
// only runs those.  HHGT_LZ4_BITPLANES=0 keeps everything on the byte-wise encoder.
static bool lz4_bitplanes_take(const uint8_t *d_src, const uint8_t *d_planes, uint64_t chunk_nbytes, int typesize, int blocksize,
                               size_t slot_bytes)
{
    static const bool bp_env = !(getenv("HHGT_LZ4_BITPLANES") && atoi(getenv("HHGT_LZ4_BITPLANES")) == 0);
    return bp_env && typesize == 2 && blocksize == 8192 && chunk_nbytes % 8192 == 0 &&
           (d_planes || (reinterpret_cast<uintptr_t>(d_src) & 15u) == 0) && slot_bytes >= 4128;
}

// The bit-plane coder's effort argument: candidates tried per one along the hash chain (clevel 1-2: none, offset-1 runs
// only; HHGT_LZ4_DEPTH overrides).  clevel 9 — what the file-writing paths run at — also parses lazily (+ 0x100;
// HHGT_LZ4_LAZY=0 / 1 overrides: 1 at the default depth is the measurement of what the rule costs the bench)
static int lz4_bitplanes_depth(int clevel)
{
    static const int depth_env = getenv("HHGT_LZ4_DEPTH") ? atoi(getenv("HHGT_LZ4_DEPTH")) : -1;
    static const int lazy_env = getenv("HHGT_LZ4_LAZY") ? atoi(getenv("HHGT_LZ4_LAZY")) : -1;
    int depth = depth_env >= 0 ? depth_env : (clevel <= 2 ? 0 : clevel <= 4 ? 1 : clevel <= 6 ? 2 : clevel == 7 ? 4 : clevel == 8 ? 8 : 12);
    if ((lazy_env < 0 ? clevel >= 9 && depth == 12 : lazy_env != 0) && (depth == 2 || depth == 12)) depth |= 0x100;
    return depth;
}

// Workgroup geometry: blocks are split into `typesize` streams (one wave each) as Blosc splits them; sstride = a stream's
// bytes + LZ_SLACK zero bytes for the lanes' lookahead, 16-byte aligned.
struct LzGeom {
    uint32_t split, nwaves, nblocks, sstride;
};
static LzGeom lz4_geometry(uint64_t chunk_nbytes, int typesize, int blocksize)
{
    LzGeom g;
    g.split = (typesize >= 2 && typesize <= 16 && blocksize / typesize >= 128) ? 1u : 0u;
    g.nwaves = g.split ? (uint32_t)typesize : 1u;
    g.nblocks = (uint32_t)((chunk_nbytes + blocksize - 1) / blocksize);
    const uint32_t max_stream = g.split ? (uint32_t)blocksize / (uint32_t)typesize : (uint32_t)blocksize;
    g.sstride = (max_stream + LZ_SLACK + 15u) & ~15u;
    if (g.split && chunk_nbytes % blocksize) {
        // a leftover block is compressed as ONE stream laid out contiguously over the data area
        uint32_t need = ((uint32_t)(chunk_nbytes % blocksize) + LZ_SLACK + 15u) & ~15u;
        if (need > g.sstride * g.nwaves) g.sstride = (need + g.nwaves - 1) / g.nwaves;
        g.sstride = (g.sstride + 15u) & ~15u;
    }
    return g;
}

// Hash table size: the kernel is latency/issue bound, so resident waves matter more than table reach.  The largest table
// (<= 4096 entries) that does not cost a resident workgroup relative to the smallest one (512 entries); 160 KiB LDS and 32
// waves per CU.  (On genotype planes the ratio is the same with 64 .. 512 entries.)
static uint32_t lz4_hashlog(uint32_t nwaves, uint32_t sstride)
{
    auto occ = [&](uint32_t hl) {
        size_t by_lds = (160 * 1024) / (size_t)lz4_lds_layout(nwaves, sstride, hl).total, by_waves = 32 / nwaves;
        return by_lds < by_waves ? by_lds : by_waves;
    };
    uint32_t hashlog = 12;
    while (hashlog > 9 && occ(hashlog) < occ(9)) --hashlog;
    return hashlog;
}

// The instantiations: two-wave workgroups are compiled for 8 (run only) or 7 waves per SIMD, larger ones without a bound;
// from bit planes the workgroup always has two waves.
using LzKernelFn = decltype(&k_lz4_blocks<0, LZ_HASH, false>);   // the nine have one signature
struct LzKernel {
    int mw;
    LzEffort effort;
    bool planes;
    LzKernelFn fn;
};
template <int MW, LzEffort EFFORT, bool PLANES>
static LzKernel lz4_kernel()
{
    return LzKernel{MW, EFFORT, PLANES, k_lz4_blocks<MW, (int)EFFORT, PLANES>};
}
static const LzKernel lz4_kernels[] = {
    lz4_kernel<0, LZ_RUN_ONLY, false>(), lz4_kernel<8, LZ_RUN_ONLY, false>(), lz4_kernel<0, LZ_HASH, false>(),
    lz4_kernel<7, LZ_HASH, false>(),     lz4_kernel<0, LZ_LONG_RUN, false>(), lz4_kernel<7, LZ_LONG_RUN, false>(),
    lz4_kernel<8, LZ_RUN_ONLY, true>(),  lz4_kernel<7, LZ_HASH, true>(),      lz4_kernel<7, LZ_LONG_RUN, true>(),
};

int launch_lz4_blocks(const uint8_t *d_src, const uint8_t *d_planes, PlanesGeom pg, uint64_t n_chunks, uint64_t chunk_nbytes, int typesize,
                      int blocksize, uint8_t *d_scratch, size_t slot_bytes, uint32_t *d_csize, int clevel, uint32_t *d_flags, uint32_t tag,
                      hipStream_t st)
{
    if (d_planes && (typesize != 2 || blocksize != 8192 || chunk_nbytes % 8192 || (reinterpret_cast<uintptr_t>(d_planes) & 15u))) {
        hhgt_set_error("lz4: bit planes stand for typesize 2, 8 KiB blocks, chunks of whole blocks, 16-byte aligned");
        return HHGT_ERR_ARG;
    }
    const bool bitplanes = lz4_bitplanes_take(d_src, d_planes, chunk_nbytes, typesize, blocksize, slot_bytes);
    if (bitplanes) {
        const int rc = launch_lz4_bitplanes(d_planes ? d_planes : d_src, d_planes != nullptr, pg, n_chunks * (chunk_nbytes / 8192), d_scratch,
                                            slot_bytes, d_csize, lz4_bitplanes_depth(clevel), d_flags, tag, st);
        if (rc != HHGT_OK) return rc;
    }
    const LzGeom g = lz4_geometry(chunk_nbytes, typesize, blocksize);
    const uint32_t hashlog = lz4_hashlog(g.nwaves, g.sstride);
    const size_t lds = lz4_lds_layout(g.nwaves, g.sstride, hashlog).total;
    if (lds > 160 * 1024 - 64) {
        hhgt_set_error("lz4: block of %d bytes x typesize %d does not fit LDS", blocksize, typesize);
        return HHGT_ERR_ARG;
    }
    static size_t attr_lds = 64 * 1024;  // dynamic LDS above 64 KiB needs an explicit opt-in
    if (lds > attr_lds) {
        for (const LzKernel &k : lz4_kernels) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_lds = lds;
    }
    uint64_t grid = n_chunks * g.nblocks;
    if (grid == 0) return HHGT_OK;
    // scan mode: a fixed grid (enough workgroups to fill the chip) scans the stream sizes, 64 blocks per workgroup and step
    if (bitplanes) grid = (grid + 63) / 64 < 256u * 14u ? (grid + 63) / 64 : 256u * 14u;
    if (grid > 0x7fffffffull) {
        hhgt_set_error("lz4: too many blocks");
        return HHGT_ERR_ARG;
    }
    const LzEffort effort = lz4_effort(clevel);
    const int mw = (d_planes || g.nwaves <= 2) ? (effort == LZ_RUN_ONLY ? 8 : 7) : 0;
    const LzKernel *k = nullptr;
    for (const LzKernel &c : lz4_kernels)
        if (c.mw == mw && c.effort == effort && c.planes == (d_planes != nullptr)) {
            k = &c;
            break;
        }
    if (!k) {
        hhgt_set_error("lz4: no kernel for %d waves per SIMD at effort %d", mw, (int)effort);
        return HHGT_ERR_ARG;
    }
    const uint32_t *mark_flag = bitplanes ? d_flags : nullptr;   // scan mode: where the bit-plane coder says whether it left marks
    hipLaunchKernelGGL(k->fn, dim3((uint32_t)grid), dim3(64u * g.nwaves), lds, st, d_src, g.nblocks, chunk_nbytes, (uint32_t)typesize,
                       (uint32_t)blocksize, g.split, g.sstride, hashlog, d_scratch, (uint64_t)slot_bytes, d_csize,
                       (uint32_t)(n_chunks * g.nblocks), d_planes, pg, mark_flag, tag);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
