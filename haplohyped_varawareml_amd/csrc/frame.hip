// frame.hip — Blosc chunk framing: header | bstarts | per block, per stream: int32 csize + bytes.
//
// Produces what c-blosc2 hands back to the HDF5 filter pipeline for a dataset written through filter 32001
// (shuffle + LZ4-format codec): a self-describing chunk whose header says typesize / nbytes / blocksize / cbytes and whose
// bstarts[] give each block's offset, so a reader can decode one block (= one sample row of the
// genotype chunk) without touching the others.  Layout restated in oracle/codec_oracle.c, pinned
// there against c-blosc 1.21 for the 16-byte header form.
//
// k_frame_sizes : one workgroup per chunk; block sizes -> bstarts (exclusive scan), chunk cbytes,
//                 "memcpyed" decision (compressed form larger than nbytes + header).
// k_scan_u64    : chunk offsets (single workgroup; O(chunks)).
// k_frame_write : one WAVE per block; copies the stream bytes from the LZ4 scratch slots to their final (byte-aligned)
//                 position, 16 bytes per lane.  A wave moves about 1.3 KB and is a chain of memory round trips, so the
//                 kernel is written around what one wave waits for:
//                   1. everything the wave must know about its block — the chunk's two offsets and flag, the block's bstart,
//                      its stream sizes — is requested together, by scalar loads from wave-uniform addresses, and costs ONE
//                      wait; the decisions on those values (capacity, memcpyed) come behind that wait;
//                   2. on the genotype path (two streams per block) the first 512 bytes of both streams are requested WITH
//                      the metadata — a slot's address depends on the block index alone — and only the rest, [512, 1024) of
//                      a stream, waits for the sizes;
//                   3. no store stands between a load and its wait: header, bstarts entry, size prefixes and payload are
//                      all written behind the last payload wait (the memory counter counts stores too).
#include "common.h"

#define BLOSC_DOSHUFFLE 0x1u
#define BLOSC_MEMCPYED 0x2u
#define BLOSC_DOBITSHUFFLE 0x4u
#define BLOSC_DONT_SPLIT 0x10u

struct FrameParams {
    uint32_t nblocks, typesize, blocksize, split, nwaves, format, hl;
    uint64_t chunk_nbytes, slot_bytes;
};

__device__ __forceinline__ uint32_t frame_wave_incl_scan(uint32_t v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_frame_sizes(FrameParams P, const uint32_t *__restrict__ csize,
                                                     uint32_t *__restrict__ bstart,
                                                     unsigned long long *__restrict__ chunk_csize,
                                                     uint32_t *__restrict__ chunk_flags)
{
    __shared__ uint32_t sm[8];
    const uint64_t chunk = blockIdx.x;
    uint32_t carry = P.hl + 4u * P.nblocks;
    for (uint32_t b0 = 0; b0 < P.nblocks; b0 += 256u) {
        const uint32_t b = b0 + threadIdx.x;
        uint32_t sz = 0;
        if (b < P.nblocks) {
            const uint64_t boff = (uint64_t)b * P.blocksize;
            const bool leftover = P.chunk_nbytes - boff < P.blocksize;
            const uint32_t ns = (P.split && !leftover) ? P.typesize : 1u;
            const uint32_t *cs = csize + (chunk * P.nblocks + b) * P.nwaves;
            for (uint32_t j = 0; j < ns; ++j) sz += 4u + cs[j];
        }
        uint32_t inc = frame_wave_incl_scan(sz);
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        if (lane == 63) sm[w] = inc;
        __syncthreads();
        uint32_t base = 0, tot = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t x = sm[i];
            if (i < w) base += x;
            tot += x;
        }
        __syncthreads();
        if (b < P.nblocks) bstart[chunk * P.nblocks + b] = carry + base + inc - sz;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        uint32_t flags = 0;
        unsigned long long cb = carry;
        if (cb > P.chunk_nbytes + P.hl) {
            flags = 1u;
            cb = P.chunk_nbytes + P.hl;
        }
        chunk_csize[chunk] = cb;
        chunk_flags[chunk] = flags;
    }
}

// single workgroup exclusive scan of uint64 (chunk sizes -> chunk offsets); out[n] = total
__global__ __launch_bounds__(256) void k_scan_u64(const unsigned long long *__restrict__ in, uint64_t n,
                                                  unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long sm[4];
    unsigned long long carry = 0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (uint64_t i0 = 0; i0 < n; i0 += 256u) {
        const uint64_t i = i0 + threadIdx.x;
        unsigned long long v = i < n ? in[i] : 0ull, inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            unsigned long long t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63) sm[w] = inc;
        __syncthreads();
        unsigned long long base = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned long long x = sm[k];
            if (k < w) base += x;
            tot += x;
        }
        __syncthreads();
        if (i < n) out[i] = carry + base + inc - v;
        carry += tot;
    }
    if (threadIdx.x == 0) out[n] = carry;
}

// Copies by one wave, src 16-byte aligned (an LZ4 scratch slot), dst at any byte: 16 bytes per lane — one load instruction per
// KiB — stored where they belong with byte-aligned stores (round 4; the first version moved dwords, two loads per dword and a
// funnel shift to reach dword-aligned destinations: 8 load instructions per KiB).
typedef uint32_t u32x4_fr __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_fr_unaligned __attribute__((ext_vector_type(4), aligned(1)));
typedef uint64_t u64_fr_unaligned __attribute__((aligned(1)));
typedef uint32_t u32_fr_unaligned __attribute__((aligned(1)));
typedef uint16_t u16_fr_unaligned __attribute__((aligned(1)));

__device__ __forceinline__ u32x4_fr wave_get16(const uint8_t *__restrict__ s)
{
    return *reinterpret_cast<const u32x4_fr *>(s);
}

__device__ __forceinline__ void put_u32(uint8_t *__restrict__ d, uint32_t v)
{
    *reinterpret_cast<u32_fr_unaligned *>(d) = v;
}

// the first `left` (>= 1) bytes of v to d: one 16-byte store, or — the last piece of a stream, 1-15 bytes — at most four
// stores of 8, 4, 2 and 1 bytes by the bits of `left`
__device__ __forceinline__ void wave_put16(uint8_t *__restrict__ d, const u32x4_fr &v, uint32_t left)
{
    if (left >= 16u) {
        *reinterpret_cast<u32x4_fr_unaligned *>(d) = v;
        return;
    }
    uint64_t w = (uint64_t)v.x | ((uint64_t)v.y << 32);
    if (left & 8u) {
        *reinterpret_cast<u64_fr_unaligned *>(d) = w;
        d += 8;
        w = (uint64_t)v.z | ((uint64_t)v.w << 32);
    }
    if (left & 4u) {
        put_u32(d, (uint32_t)w);
        d += 4;
        w >>= 32;
    }
    if (left & 2u) {
        *reinterpret_cast<u16_fr_unaligned *>(d) = (uint16_t)w;
        d += 2;
        w >>= 16;
    }
    if (left & 1u) *d = (uint8_t)w;
}

// bytes [1024, n) of a stream (streams longer than 1 KiB): 4 KiB per pass with the loads in flight together.  (a slot is padded
// to 16 bytes: the last piece may read past n, and stores only what is left)
__device__ __forceinline__ void wave_copy_rest(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t n)
{
    const uint32_t o = (threadIdx.x & 63u) * 16u;
    for (uint32_t base = 1024u; base < n; base += 4096u) {
        u32x4_fr v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t q = base + (uint32_t)k * 1024u + o;
            v[k] = u32x4_fr{0u, 0u, 0u, 0u};
            if (q < n) v[k] = wave_get16(src + q);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t q = base + (uint32_t)k * 1024u + o;
            if (q < n) wave_put16(dst + q, v[k], n - q);
        }
    }
}

__device__ __forceinline__ void wg_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t n)
{
    const uint32_t o = (threadIdx.x & 63u) * 16u;
    if (o < n) wave_put16(dst + o, wave_get16(src + o), n - o);
    wave_copy_rest(dst, src, n);
}

// header bytes of a chunk (see oracle/codec_oracle.c write_header), by the first hl lanes of the wave that frames block 0
__device__ __forceinline__ void frame_header(const FrameParams &P, uint8_t *__restrict__ cdst, uint32_t cbytes, uint32_t memcpyed)
{
    const uint32_t i = threadIdx.x & 63u;
    if (i >= P.hl) return;
    const uint32_t split_flag = P.split ? 0u : BLOSC_DONT_SPLIT;
    uint32_t flags = (1u << 5) | (P.typesize > 1u ? BLOSC_DOSHUFFLE : 0u) | split_flag | (memcpyed ? BLOSC_MEMCPYED : 0u);
    uint8_t v = 0;
    if (P.format == HHGT_BLOSC2) {
        if (i == 0) v = 5;
        else if (i == 1) v = 1;
        else if (i == 2) v = (uint8_t)(flags | BLOSC_DOSHUFFLE | BLOSC_DOBITSHUFFLE);
        else if (i == 3) v = (uint8_t)P.typesize;
        else if (i == 16 + 5) v = (flags & BLOSC_DOSHUFFLE) ? 1 : 0;
    } else {
        if (i == 0) v = 2;
        else if (i == 1) v = 1;
        else if (i == 2) v = (uint8_t)flags;
        else if (i == 3) v = (uint8_t)P.typesize;
    }
    if (i >= 4 && i < 8) v = (uint8_t)((uint32_t)P.chunk_nbytes >> ((i - 4) * 8));
    if (i >= 8 && i < 12) v = (uint8_t)(P.blocksize >> ((i - 8) * 8));
    if (i >= 12 && i < 16) v = (uint8_t)(cbytes >> ((i - 12) * 8));
    cdst[i] = v;
}

// verbatim copy of source block b behind the header of a memcpyed chunk (rare: an incompressible chunk)
__device__ __forceinline__ void frame_block_memcpyed(const FrameParams &P, const uint8_t *__restrict__ src, uint8_t *__restrict__ cdst,
                                                     uint64_t chunk, uint32_t b, uint64_t gb, const uint8_t *__restrict__ planes,
                                                     const PlanesGeom &pg)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t boff = (uint64_t)b * P.blocksize;
    const uint32_t bsize = (uint32_t)(P.chunk_nbytes - boff < P.blocksize ? P.chunk_nbytes - boff : P.blocksize);
    // (source is 16-byte aligned per block only when blocksize is; the byte loop takes what wg_copy's contract does not)
    const uint8_t *s = src + chunk * P.chunk_nbytes + boff;
    uint8_t *d = cdst + P.hl + boff;
    if (planes) {   // the block exists as bit planes (hhgt.h "Bit-plane form"): its bytes are generated
        uint64_t pcol;
        uint32_t prow, pbi;
        planes_block(pg, gb, &pcol, &prow, &pbi);
        const uint64_t kst = (uint64_t)pg.S_pad * 32ull;   // bytes between the kind-planes of a tile
        for (uint32_t i = lane; i < 4096u; i += 64u) {
            const uint8_t *pl = planes + planes_piece(pg, pcol, pbi * 16u + (i >> 8), 0u, prow) + ((i & 255u) >> 3);
#pragma unroll
            for (uint32_t h = 0; h < 2u; ++h) {
                uint32_t v = (pl[h * kst] >> (i & 7u)) & 1u;
                if ((pl[(2ull + h) * kst] >> (i & 7u)) & 1u) v = v ? 0xF7u : (src ? (uint32_t)s[2u * i + h] : 0u);
                d[2u * i + h] = (uint8_t)v;
            }
        }
    } else if ((reinterpret_cast<uintptr_t>(s) & 15u) == 0 && (bsize & 15u) == 0) wg_copy(d, s, bsize);
    else for (uint32_t i = lane; i < bsize; i += 64u) d[i] = s[i];
}

#define FRAME_WAVES 4u   // waves (= Blosc blocks) per workgroup of k_frame_write

// what a wave must know about its block.  chunk * nblocks + b == gb, so the block's bstart and sizes are indexed by gb alone;
// only the chunk's offsets and flag need the division.
struct BlockMeta {
    uint64_t chunk;
    unsigned long long coff, cend;
    uint32_t b, bs, memcpyed;
};

// The metadata of block gb in ONE level: scalar loads (gb is wave-uniform) of inputs that earlier launches wrote, all
// requested before the first of them is used.  The caller takes the values with frame_meta_take, after it has requested
// whatever else it wants in flight beside them.
__device__ __forceinline__ BlockMeta frame_meta_load(const FrameParams &P, const uint32_t *__restrict__ bstart,
                                                     const unsigned long long *__restrict__ chunk_off,
                                                     const uint32_t *__restrict__ chunk_flags, uint64_t gb)
{
    BlockMeta m;
    m.bs = bstart[gb];
    m.chunk = gb / P.nblocks;
    m.b = (uint32_t)(gb - m.chunk * P.nblocks);
    m.coff = chunk_off[m.chunk];
    m.cend = chunk_off[m.chunk + 1];
    m.memcpyed = chunk_flags[m.chunk];
    return m;
}

// (the values are taken here, all of them: the compiler otherwise moves each load down to its first use, behind the branches
// on the others, and the wave pays a round trip per value)
#define frame_meta_take(m, x0, x1) asm volatile("" : "+s"((m).bs), "+s"((m).coff), "+s"((m).cend), "+s"((m).memcpyed), "+s"(x0), "+s"(x1))

// The genotype path: block gb of a two-stream geometry (typesize 2, split blocks) whose slots hold 512 bytes or more, by ONE
// wave — lanes 0-31 work on stream 0, lanes 32-63 on stream 1.  -> false: the block is not for this path (memcpyed chunk,
// leftover block) and nothing was written.
//
// It stands in a function of its own, called FIRST by the kernel, and has one exit: the compiler's wait insertion merges what
// is pending over all paths that lead into a block.  With the other paths inlined beside it (they were, at first) their loops'
// pending loads count as pending here, and every write to a register they use waits for all memory operations of the wave —
// the early load before the second piece is requested, the stores of the size prefixes before the payload stores.
__device__ __forceinline__ bool frame_wave_genotype(const FrameParams &P, const uint8_t *__restrict__ scratch,
                                                    const uint32_t *__restrict__ csize, const uint32_t *__restrict__ bstart,
                                                    const unsigned long long *__restrict__ chunk_off,
                                                    const uint32_t *__restrict__ chunk_flags, uint8_t *__restrict__ dst,
                                                    uint64_t dst_cap, uint64_t gb)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t half = lane >> 5, o = (lane & 31u) * 16u;
    const uint8_t *s0 = scratch + 2u * gb * P.slot_bytes;
    const uint8_t *sl = s0 + (half ? (uint32_t)P.slot_bytes : 0u);
    // bytes [0, 512) of both streams, before anything is known about them: the address depends on gb alone, and what lies
    // behind a stream's end is never stored.  (The caller has checked slot_bytes >= 512: the load stays inside the scratch.)
    u32x4_fr va = wave_get16(sl + o);
    BlockMeta m = frame_meta_load(P, bstart, chunk_off, chunk_flags, gb);
    uint32_t cs0 = csize[2u * gb], cs1 = csize[2u * gb + 1u];
    frame_meta_take(m, cs0, cs1);
    // bytes [512, 1024), exactly, ahead of every decision on the metadata.  A size is at most the slot; the second test keeps
    // the load inside the allocation whatever a size says.
    const uint32_t n = half ? cs1 : cs0;
    const bool more = 512u + o < n && 528u + o <= P.slot_bytes;
    u32x4_fr vb = u32x4_fr{0u, 0u, 0u, 0u};
    if (more) vb = wave_get16(sl + 512u + o);
    // the one payload wait; every store of the wave comes behind it (a store issued before it would be waited for as well)
    asm volatile("" : "+v"(va), "+v"(vb));
    bool taken = true;
    if (m.cend <= dst_cap) {   // capacity error is reported by the host from chunk_off[n]
        const bool leftover = P.chunk_nbytes - (uint64_t)m.b * P.blocksize < P.blocksize;
        if (m.memcpyed || leftover) taken = false;
        else {
            uint8_t *cdst = dst + m.coff;
            // where this lane's stream goes: any byte.  (Round 4, a timing-only build with these rounded down to 16 bytes ran
            // the stage in the same time: the alignment of the stores is not what the kernel waits for.)
            uint8_t *dl = cdst + m.bs + 4u + (half ? cs0 + 4u : 0u);
            if (m.b == 0) frame_header(P, cdst, (uint32_t)(m.cend - m.coff), 0u);
            if (lane == 0) put_u32(cdst + P.hl + 4u * m.b, m.bs);
            if ((lane & 31u) == 0) put_u32(dl - 4u, n);
            if (o < n) wave_put16(dl + o, va, n - o);
            if (more) wave_put16(dl + 512u + o, vb, n - 512u - o);
            if (cs0 > 1024u || cs1 > 1024u) {   // rare on genotype planes: the rest by the whole wave, stream after stream
                uint8_t *d0 = cdst + m.bs + 4u;
                wave_copy_rest(d0, s0, cs0);
                wave_copy_rest(d0 + cs0 + 4u, s0 + P.slot_bytes, cs1);
            }
        }
    }
    return taken;
}

// Every other block, by ONE wave: any number of streams (lane j holds the size of stream j, nwaves <= 16) copied one after
// the other, leftover blocks, memcpyed chunks.
__device__ __forceinline__ void frame_wave_any(const FrameParams &P, const uint8_t *__restrict__ scratch, const uint32_t *__restrict__ csize,
                                               const uint8_t *__restrict__ src, const uint32_t *__restrict__ bstart,
                                               const unsigned long long *__restrict__ chunk_off, const uint32_t *__restrict__ chunk_flags,
                                               uint8_t *__restrict__ dst, uint64_t dst_cap, uint64_t gb, const uint8_t *__restrict__ planes,
                                               const PlanesGeom &pg)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t sidx0 = gb * P.nwaves;
    const uint32_t cs_l = lane < P.nwaves ? csize[sidx0 + lane] : 0u;
    BlockMeta m = frame_meta_load(P, bstart, chunk_off, chunk_flags, gb);
    frame_meta_take(m, m.b, m.chunk);
    if (m.cend > dst_cap) return;  // capacity error is reported by the host from chunk_off[n]
    uint8_t *cdst = dst + m.coff;
    if (m.b == 0) frame_header(P, cdst, (uint32_t)(m.cend - m.coff), m.memcpyed);
    if (m.memcpyed) {
        frame_block_memcpyed(P, src, cdst, m.chunk, m.b, gb, planes, pg);
        return;
    }
    const bool leftover = P.chunk_nbytes - (uint64_t)m.b * P.blocksize < P.blocksize;
    const uint32_t ns = (P.split && !leftover) ? P.typesize : 1u;
    if (lane == 0) put_u32(cdst + P.hl + 4u * m.b, m.bs);
    uint32_t q = m.bs;
    for (uint32_t j = 0; j < ns; ++j) {
        const uint32_t cs = (uint32_t)__builtin_amdgcn_readlane((int)cs_l, (int)j);
        if (lane == 0) put_u32(cdst + q, cs);
        wg_copy(cdst + q + 4u, scratch + (sidx0 + j) * P.slot_bytes, cs);
        q += 4u + cs;
    }
}

__global__ __launch_bounds__(64 * FRAME_WAVES) void k_frame_write(FrameParams P, const uint8_t *__restrict__ scratch,
                                                                  const uint32_t *__restrict__ csize,
                                                                  const uint8_t *__restrict__ src,
                                                                  const uint32_t *__restrict__ bstart,
                                                                  const unsigned long long *__restrict__ chunk_off,
                                                                  const uint32_t *__restrict__ chunk_flags,
                                                                  uint8_t *__restrict__ dst, uint64_t dst_cap,
                                                                  uint64_t n_total_blocks, const uint8_t *__restrict__ planes, PlanesGeom pg)
{
    // one wave per Blosc block (blocks are a few KiB after compression: a whole workgroup per block idles).  (Round 4: a
    // wave per PAIR of blocks, the four streams in flight together, was slower — 2.05 against 1.76 ms per 3 M x 2504 step
    // alone, 5.5 against 2.8 ms beside the encode chain: the kernel lives on the number of waves in flight.)
    // The wave's index through readfirstlane: the block index, and with it every metadata address, is uniform for the compiler.
    const uint64_t gb = (uint64_t)blockIdx.x * FRAME_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (gb >= n_total_blocks) return;
    bool done = false;
    if (P.nwaves == 2u && P.slot_bytes >= 512u) done = frame_wave_genotype(P, scratch, csize, bstart, chunk_off, chunk_flags, dst, dst_cap, gb);
    if (!done) frame_wave_any(P, scratch, csize, src, bstart, chunk_off, chunk_flags, dst, dst_cap, gb, planes, pg);
}

int launch_frame(const uint8_t *d_scratch, size_t slot_bytes, const uint32_t *d_csize, const uint8_t *d_src, const uint8_t *d_planes,
                 PlanesGeom pg, uint64_t n_chunks, uint64_t chunk_nbytes, int typesize, int blocksize, int format,
                 uint32_t *d_bstart, uint64_t *d_chunk_csize, uint8_t *d_dst, uint64_t dst_cap,
                 uint64_t *d_chunk_off, uint32_t *d_chunk_flags, hipStream_t st)
{
    if (n_chunks == 0) return HHGT_OK;
    FrameParams P;
    P.nblocks = (uint32_t)((chunk_nbytes + blocksize - 1) / blocksize);
    P.typesize = (uint32_t)typesize;
    P.blocksize = (uint32_t)blocksize;
    P.split = (typesize >= 2 && typesize <= 16 && blocksize / typesize >= 128) ? 1u : 0u;
    P.nwaves = P.split ? (uint32_t)typesize : 1u;
    P.format = (uint32_t)format;
    P.hl = format == HHGT_BLOSC2 ? 32u : 16u;
    P.chunk_nbytes = chunk_nbytes;
    P.slot_bytes = slot_bytes;
    // (a one-launch form — a ticket per workgroup, a decoupled look-back over the chunk totals, 8 blocks per wave — was built
    // and measured in round 4: framing 2.97 against 1.83 ms per 3 M x 2504 step; removed, git history has it)
    hipLaunchKernelGGL(k_frame_sizes, dim3((uint32_t)n_chunks), dim3(256), 0, st, P, d_csize, d_bstart,
                       reinterpret_cast<unsigned long long *>(d_chunk_csize), d_chunk_flags);
    hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(256), 0, st,
                       reinterpret_cast<const unsigned long long *>(d_chunk_csize), n_chunks,
                       reinterpret_cast<unsigned long long *>(d_chunk_off));
    const uint64_t n_total_blocks = n_chunks * P.nblocks;
    hipLaunchKernelGGL(k_frame_write, dim3((uint32_t)((n_total_blocks + FRAME_WAVES - 1) / FRAME_WAVES)), dim3(64 * FRAME_WAVES), 0, st, P,
                       d_scratch, d_csize, d_src, d_bstart, reinterpret_cast<const unsigned long long *>(d_chunk_off),
                       d_chunk_flags, d_dst, dst_cap, n_total_blocks, d_planes, pg);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
