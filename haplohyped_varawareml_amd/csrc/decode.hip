// decode.hip — Blosc chunk decode (LZ4 block decode + byte-unshuffle) on gfx950.
//
// Read-side counterpart of lz4.hip/frame.hip: what the HDF5 filter 32001 does when the reference's
// reader pulls a dataset (/root/reference/src/utils/h5_reader.py:37-41) — and the device-side half of
// the encode -> compress -> decode round-trip property used by the full-size parity tests.
// Workgroup = one block; wave j decodes stream j in place: compressed bytes staged at the end of its LDS
// plane buffer, decoded bytes written from the start; the workgroup then un-shuffles the planes straight into HBM with 16 B stores.
// k_decode_blocks decodes whole chunks; k_decode_sel (hhgt_decompress_blocks) decodes one selected block per workgroup
// and writes only a byte range of it — the read of a hyperslab.  Both run the same header check, stream walk, in-place
// LZ4 decode and un-shuffle (the __device__ functions below).
#include "common.h"

#define BLOSC_DOSHUFFLE 0x1u
#define BLOSC_MEMCPYED 0x2u
#define BLOSC_DOBITSHUFFLE 0x4u
#define BLOSC_DONT_SPLIT 0x10u

typedef uint32_t u32_unaligned __attribute__((aligned(1)));
// little-endian u32 at any byte address of GLOBAL memory (one unaligned dword load, not four byte loads)
__device__ __forceinline__ uint32_t ld32u(const uint8_t *p) { return *reinterpret_cast<const u32_unaligned *>(p); }

// a value every lane holds identically, moved to an SGPR: everything derived from it (ip, op, lengths, the
// branches on them) then compiles to scalar code instead of exec-masked vector code
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// LZ4 length extension starting at cin[ip]: returns added length, advances ip. wave-uniform.
__device__ __forceinline__ bool read_ext(const uint8_t *cin, uint32_t csize, uint32_t &ip, uint32_t &len)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (;;) {
        const uint32_t i = ip + lane;
        const uint32_t b = i < csize ? cin[i] : 0u;
        const unsigned long long stop = __ballot(b != 255u);
        if (stop == 0ull) {
            len += 255u * 64u;
            ip += 64u;
            if (ip >= csize) return false;
            continue;
        }
        const uint32_t j = (uint32_t)__builtin_ctzll(stop);
        if (ip + j >= csize) return false;
        len += 255u * j + (uint32_t)__builtin_amdgcn_readlane((int)b, (int)j);
        ip += j + 1u;
        return true;
    }
}

// out[op, op + ml) = the ml bytes starting `off` back (all arguments but lane wave-uniform, off >= 1)
__device__ __forceinline__ void lz4_match_copy(uint8_t *out, uint32_t op, uint32_t off, uint32_t ml, uint32_t lane)
{
    // byte k of the match is byte (k mod off) of the `off` bytes before op once the match overlaps itself, byte k of
    // them otherwise; one straight-line step serves the first 64 bytes of every case (a 64-byte step never reads a
    // byte written in the same step), the loop behind it is only entered by matches longer than that
    const uint8_t *pat = out + op - off;
    uint32_t ph = lane, step = 0u;
    if ((ml < 64u ? ml : 64u) > off) {  // off < 64 and ml > off: the match overlaps itself within a step
        if ((off & (off - 1u)) == 0u) {  // runs of a byte / pair / quad: the usual case, no division
            ph = lane & (off - 1u);
        } else {
            ph = lane % off;
            step = 64u % off;
        }
    }
    if (lane < ml) out[op + lane] = pat[ph];
    if (ml > 64u) {
        asm volatile("" ::: "memory");  // keep the (scalar) length test: the loop guard alone would cost every sequence
        if (off < 64u) {
            for (uint32_t k = lane + 64u; k < ml; k += 64u) {
                ph += step;
                if (ph >= off) ph -= off;
                out[op + k] = pat[ph];
            }
        } else {
            for (uint32_t k = lane + 64u; k < ml; k += 64u) out[op + k] = pat[k];
        }
    }
}

// decode cin[0, csize) (LDS) -> out[0, n) (LDS). returns true on success. wave-cooperative.
__device__ __forceinline__ bool lz4_wave_decode(const uint8_t *cin, uint32_t csize, uint8_t *out, uint32_t n)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t ip = 0, op = 0;
    for (;;) {
        // Fast path (nearly every sequence of a genotype plane): token, up to 13 literals, the offset and one match-length
        // extension byte all sit in the 19 bytes at ip.  Lane k (k <= 15) gathers the two aligned dwords around byte
        // ip + k and forms the 32-bit window starting there, so every header field is one readlane away: the token
        // from lane 0, offset + extension byte from lane ll + 1; byte 1 of lane k's window is literal k.  The kernel
        // is bound by scalar-ALU issue (the SQ counters show 1.0 scalar op per cycle per SIMD), so the point of this
        // shape is few scalar instructions per sequence.  (cin has >= 24 readable bytes past csize.)
        {
            const uint32_t q = ip + (lane < 15u ? lane : 15u);
            const uint32_t *w = reinterpret_cast<const uint32_t *>(cin) + (q >> 2);
            const uint32_t v = __builtin_amdgcn_alignbyte(w[1], w[0], q & 3u);         // bytes ip + lane .. + 3
            const uint32_t t = uni(v);
            const uint32_t ll = (t >> 4) & 15u, mlt = t & 15u;
            if (ll <= 13u) {
                const uint32_t s3 = (uint32_t)__builtin_amdgcn_readlane((int)v, (int)(ll + 1u));
                const uint32_t off = s3 & 0xFFFFu;
                // lengths 19..273 carry one extension byte (255 there = longer still: general path below); branch-free
                const uint32_t is15 = (mlt + 1u) >> 4;
                const uint32_t e1 = ((s3 >> 16) & 0xFFu) * is15;
                const uint32_t ml = mlt + 4u + e1, adv = ll + 3u + is15;
                // whole sequence inside the stream (so this is not the literal-only last one), output fits, offset
                // reaches no further back than the first byte; anything else is sorted out by the general path
                if (e1 != 255u && ip + adv <= csize && ll + ml <= n - op && off - 1u < op + ll) {
                    if (lane < ll) out[op + lane] = (uint8_t)(v >> 8);
                    op += ll;
                    lz4_match_copy(out, op, off, ml, lane);
                    op += ml;
                    ip += adv;
                    continue;
                }
            }
        }
        if (ip >= csize) return false;  // (the fast path cannot pass its own bounds check from here either)
        const uint32_t token = uni(cin[ip++]);
        uint32_t ll = token >> 4;
        if (ll == 15u && !read_ext(cin, csize, ip, ll)) return false;
        if (ll > csize - ip || ll > n - op) return false;
        for (uint32_t k = lane; k < ll; k += 64u) out[op + k] = cin[ip + k];
        op += ll;
        ip += ll;
        if (ip == csize) break;  // last sequence carries literals only
        if (csize - ip < 2u) return false;
        const uint32_t off = uni((uint32_t)cin[ip] | ((uint32_t)cin[ip + 1u] << 8));
        ip += 2u;
        if (off == 0u || off > op) return false;
        uint32_t ml = token & 15u;
        if (ml == 15u && !read_ext(cin, csize, ip, ml)) return false;
        ml += 4u;
        if (ml > n - op) return false;
        lz4_match_copy(out, op, off, ml, lane);
        op += ml;
    }
    return op == n;
}

// ---- the decoder body, shared by k_decode_blocks (whole chunks) and k_decode_sel (block ranges) -----------------------

// what the header of one framed chunk says, once validated against the dataset's parameters
struct BloscHdr {
    uint32_t hl;          // header bytes: 16 (Blosc1) or 32 (Blosc2 extended header)
    uint32_t flags;
    uint32_t doshuffle;   // byte-shuffled
    uint32_t dont_split;  // one stream per block
};

// validates the header of the chunk ck[0, avail) (either format); false = bad chunk.  Every thread computes the same.
__device__ __forceinline__ bool blosc_header(const uint8_t *ck, uint32_t avail, uint64_t chunk_nbytes, uint32_t typesize,
                                             uint32_t blocksize, BloscHdr &h)
{
    h.hl = 16;
    h.flags = 0;
    h.doshuffle = 0;
    h.dont_split = 1;
    if (avail < 16u) return false;
    bool bad = false;
    const uint32_t version = ck[0];
    const uint32_t flags = ck[2];
    const uint32_t ts = ck[3], nbytes = ld32u(ck + 4), bs = ld32u(ck + 8), cbytes = ld32u(ck + 12);
    const bool extended = (flags & BLOSC_DOSHUFFLE) && (flags & BLOSC_DOBITSHUFFLE);
    h.flags = flags;
    h.doshuffle = (flags & BLOSC_DOSHUFFLE) ? 1u : 0u;
    if (extended) {
        h.hl = 32;
        bad = version < 3u || avail < 32u;
        h.doshuffle = 0;
        if (!bad)
            for (int k = 0; k < 6; ++k) {
                uint32_t f = ck[16 + k];
                if (f == 1u) h.doshuffle = 1u;
                else if (f != 0u) bad = true;
            }
    } else if (flags & BLOSC_DOBITSHUFFLE)
        bad = true;
    h.dont_split = (flags & BLOSC_DONT_SPLIT) ? 1u : 0u;
    bad = bad || ts != typesize || nbytes != (uint32_t)chunk_nbytes || cbytes != avail;
    if (flags & BLOSC_MEMCPYED) bad = bad || avail != chunk_nbytes + h.hl;
    else bad = bad || bs != blocksize || ((flags >> 5) & 7u) != 1u;
    return !bad;
}

// streams of a block of bsize bytes (the short last block of a chunk is always one stream)
__device__ __forceinline__ uint32_t block_streams(const BloscHdr &h, uint32_t bsize, uint32_t blocksize, uint32_t typesize)
{
    return (!h.dont_split && bsize == blocksize) ? typesize : 1u;
}

// block b of a valid, compressed chunk -> its byte planes in LDS: wave j decodes stream j in place (plane j at
// smem + j * sstride when the block is split, the whole block at smem otherwise).  Workgroup-cooperative, holds a barrier;
// returns false (the same in every thread) when the block's stream table or a stream is corrupt.
__device__ __forceinline__ bool decode_block_lds(const uint8_t *ck, uint32_t avail, uint32_t hl, uint32_t b, uint32_t bsize,
                                                 uint32_t nstreams, uint32_t sstride, uint8_t *smem, uint32_t *s_bad)
{
    const uint32_t nwaves = blockDim.x >> 6;
    const uint32_t wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63u;  // SGPR: stream sizes and LDS bases follow
    const uint32_t neblock = bsize / nstreams;
    // bytes of LDS the stream of this wave owns: its plane, or the whole area when the block is one stream
    const uint32_t cap = nstreams > 1u ? sstride : nwaves * sstride;
    // stream table of this block: walk the csize words (nstreams <= 16, serial by every thread)
    bool sbad = hl + 4u * b + 4u > avail;
    uint32_t sp = sbad ? 0u : ld32u(ck + hl + 4u * b), my_sp = 0, my_cs = 0;
    for (uint32_t j = 0; j < nstreams && !sbad; ++j) {
        if (sp + 4u > avail) {
            sbad = true;
            break;
        }
        const uint32_t cs = ld32u(ck + sp);
        if (cs == 0u || cs > neblock || sp + 4u + cs > avail) {
            sbad = true;
            break;
        }
        if (j == wave) {
            my_sp = sp + 4u;
            my_cs = cs;
        }
        sp += 4u + cs;
    }
    if (!sbad && wave < nstreams) {
        uint8_t *plane = smem + (size_t)wave * sstride;   // (one stream: wave 0 only)
        if (my_cs == neblock) {
            for (uint32_t k = lane; k < neblock; k += 64u) plane[k] = ck[my_sp + k];
        } else {
            // In-place decode (lz4.h's LZ4_DECOMPRESS_INPLACE_MARGIN scheme): the compressed bytes are staged at the
            // END of the plane's own buffer and the decoder writes from its start.  In a valid block the bytes still to
            // read never exceed the bytes still to write by more than 2 + n/255, so with a margin of (n >> 8) + 32 the
            // write head stays behind the read head; a malformed block can only garble its own output, every access
            // stays inside [plane, plane + cap).  Halves the LDS per workgroup -> 16 instead of 9 workgroups per CU.
            if (neblock + (neblock >> 8) + 60u > cap) sbad = true;
            uint8_t *cin = plane + ((cap - 24u - my_cs) & ~3u);   // dword-aligned; 24 readable bytes behind the stream
            const uint32_t nd = my_cs >> 2;       // whole dwords (unaligned global loads), then the last 1-3 bytes
            if (!sbad) {
                for (uint32_t k = lane; k < nd; k += 64u) reinterpret_cast<uint32_t *>(cin)[k] = ld32u(ck + my_sp + 4u * k);
                if (lane < (my_cs & 3u)) cin[4u * nd + lane] = ck[my_sp + 4u * nd + lane];
            }
            if (sbad || !lz4_wave_decode(cin, my_cs, plane, neblock)) sbad = true;
        }
    }
    if (sbad) atomicOr(s_bad, 1u);
    __syncthreads();
    return *s_bad == 0u;
}

// decoded bytes [lo, hi) of the block whose planes decode_block_lds left in LDS -> out[0, hi - lo) (HBM), un-shuffled.
// 16-byte stores when lo, hi and out are 16-byte aligned (the whole block of k_decode_blocks), a byte loop otherwise.
__device__ __forceinline__ void unshuffle_range(const uint8_t *planes, uint32_t doshuffle, uint32_t typesize, uint32_t nstreams,
                                                uint32_t bsize, uint32_t sstride, uint32_t lo, uint32_t hi, uint8_t *out)
{
    const uint32_t nelem = bsize / typesize;
    const uint32_t pstride = nstreams > 1u ? sstride : nelem;
    if ((!doshuffle || typesize == 1u) && nstreams == 1u) {
        for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) out[i - lo] = planes[i];
    } else if (!doshuffle) {
        // split but not shuffled (c-blosc 1.21 writes this for shuffle 0): stream j holds bytes [j neblock, (j + 1)
        // neblock) of the block and sits at planes + j * sstride
        const uint32_t neblock = bsize / nstreams;
        for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
            const uint32_t j = i / neblock;
            out[i - lo] = planes[j * sstride + (i - j * neblock)];
        }
    } else if (typesize == 2u && nstreams == 2u && ((lo | hi) & 15u) == 0u &&
               ((reinterpret_cast<uintptr_t>(out) & 15u) == 0)) {
        for (uint32_t i = lo + threadIdx.x * 16u; i < hi; i += blockDim.x * 16u) {
            uint2 a = *reinterpret_cast<const uint2 *>(planes + (i >> 1));
            uint2 c = *reinterpret_cast<const uint2 *>(planes + pstride + (i >> 1));
            uint4 v;
            v.x = __builtin_amdgcn_perm(c.x, a.x, 0x05010400u);
            v.y = __builtin_amdgcn_perm(c.x, a.x, 0x07030602u);
            v.z = __builtin_amdgcn_perm(c.y, a.y, 0x05010400u);
            v.w = __builtin_amdgcn_perm(c.y, a.y, 0x07030602u);
            *reinterpret_cast<uint4 *>(out + (i - lo)) = v;
        }
    } else {
        const uint32_t body = nelem * typesize;
        for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
            uint8_t v;
            if (i < body) {
                uint32_t e = i / typesize, j = i - e * typesize;
                v = planes[j * pstride + e];
            } else
                v = planes[(typesize - 1u) * pstride + nelem + (i - body)];
            out[i - lo] = v;
        }
    }
}

// grid = n_chunks * nblocks; block = 64 * nwaves; dynamic LDS = nwaves * sstride + 16
__global__ __launch_bounds__(1024) void k_decode_blocks(const uint8_t *__restrict__ src,
                                                        const unsigned long long *__restrict__ chunk_off,
                                                        uint32_t nblocks, uint64_t chunk_nbytes, uint32_t typesize,
                                                        uint32_t blocksize, uint32_t sstride,
                                                        uint8_t *__restrict__ dst, unsigned long long *n_bad)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ uint32_t s_bad;
    const uint32_t nwaves = blockDim.x >> 6;
    const uint64_t chunk = blockIdx.x / nblocks;
    const uint32_t b = blockIdx.x - (uint32_t)(chunk * nblocks);
    const uint8_t *ck = src + chunk_off[chunk];
    const uint32_t avail = (uint32_t)(chunk_off[chunk + 1] - chunk_off[chunk]);
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    BloscHdr h;
    const bool ok = blosc_header(ck, avail, chunk_nbytes, typesize, blocksize, h);
    const uint64_t boff = (uint64_t)b * blocksize;
    const uint32_t bsize = (uint32_t)(chunk_nbytes - boff < blocksize ? chunk_nbytes - boff : blocksize);
    uint8_t *out_blk = dst + chunk * chunk_nbytes + boff;
    // a bad header counts once per chunk, a corrupt block once per block
    if (!ok) {
        if (threadIdx.x == 0 && b == 0) atomicAdd(n_bad, 1ull);
        return;
    }
    if (h.flags & BLOSC_MEMCPYED) {
        for (uint32_t i = threadIdx.x; i < bsize; i += blockDim.x) out_blk[i] = ck[h.hl + boff + i];
        return;
    }
    const uint32_t nstreams = block_streams(h, bsize, blocksize, typesize);
    if (nstreams > nwaves) {  // header asks for a split this launch was not sized for
        if (threadIdx.x == 0 && b == 0) atomicAdd(n_bad, 1ull);
        return;
    }
    if (!decode_block_lds(ck, avail, h.hl, b, bsize, nstreams, sstride, smem, &s_bad)) {
        if (threadIdx.x == 0) atomicAdd(n_bad, 1ull);
        return;
    }
    unshuffle_range(smem, h.doshuffle, typesize, nstreams, bsize, sstride, 0u, bsize, out_blk);
}

// grid = n_sel, one selection per workgroup; block and dynamic LDS as k_decode_blocks.  Selection i: decoded bytes
// [lo, hi) of Blosc block `block` of the chunk at src_ptr -> dst + dst_off.  A bad selection counts once.
__global__ __launch_bounds__(1024) void k_decode_sel(const hhgt_block_sel *__restrict__ sel, uint64_t chunk_nbytes,
                                                     uint32_t typesize, uint32_t blocksize, uint32_t sstride,
                                                     uint8_t *__restrict__ dst, unsigned long long *n_bad)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ uint32_t s_bad;
    const uint32_t nwaves = blockDim.x >> 6;
    const hhgt_block_sel *s = sel + blockIdx.x;
    const uint8_t *ck = reinterpret_cast<const uint8_t *>(s->src_ptr);
    const uint64_t src_bytes = s->src_bytes;
    const uint32_t b = s->block, lo = s->lo, hi = s->hi;
    uint8_t *out = dst + s->dst_off;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const uint32_t avail = src_bytes > 0xffffffffull ? 0u : (uint32_t)src_bytes;   // (too large: fails the header)
    BloscHdr h;
    bool ok = blosc_header(ck, avail, chunk_nbytes, typesize, blocksize, h);
    const uint32_t nblocks = (uint32_t)((chunk_nbytes + blocksize - 1) / blocksize);
    ok = ok && b < nblocks;
    const uint64_t boff = (uint64_t)b * blocksize;
    const uint32_t bsize = ok ? (uint32_t)(chunk_nbytes - boff < blocksize ? chunk_nbytes - boff : blocksize) : 0u;
    ok = ok && lo < hi && hi <= bsize;
    if (!ok) {
        if (threadIdx.x == 0) atomicAdd(n_bad, 1ull);
        return;
    }
    if (h.flags & BLOSC_MEMCPYED) {
        const uint8_t *from = ck + h.hl + boff;
        for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) out[i - lo] = from[i];
        return;
    }
    const uint32_t nstreams = block_streams(h, bsize, blocksize, typesize);
    if (nstreams > nwaves || !decode_block_lds(ck, avail, h.hl, b, bsize, nstreams, sstride, smem, &s_bad)) {
        if (threadIdx.x == 0) atomicAdd(n_bad, 1ull);
        return;
    }
    unshuffle_range(smem, h.doshuffle, typesize, nstreams, bsize, sstride, lo, hi, out);
}

// ---- the row walk of the four query kernels (hhgt_count_alleles, hhgt_count_samples, hhgt_genotype_planes, hhgt_gather_calls)
//
// Each runs one selection per workgroup (grid = n_sel; block = 64 * nwaves and dynamic LDS as decode_geometry says for
// typesize 2: two waves): a chunk, the Blosc block `part` of its sample rows, the rows of row_mask and the variants [lo, hi)
// of that block.  Thread t owns variants [g, g + 16) of the block for g = 16 (t + k blockDim), k = 0, 1 (blockDim * 32 >=
// blocksize / 2 for every block size served), over every selected row: stage_row leaves the row's block in LDS, for_calls16
// hands the thread its 2 x 16 calls four at a time.  What a kernel does with four calls (count4, tally4, planes4, classes4), at the
// end of a row and with its totals is its own; so are the checks of its outputs.

// a bad selection counts once, whatever made it bad
__device__ __forceinline__ void bad_selection(unsigned long long *n_bad)
{
    if (threadIdx.x == 0) atomicAdd(n_bad, 1ull);
}

// a chunk lies in global memory: said through the address space, its loads are global_load, not flat_load
__device__ __forceinline__ const uint8_t *global_chunk(uint64_t src_ptr)
{
    return (const uint8_t *)(const __attribute__((address_space(1))) uint8_t *)src_ptr;
}

struct RowWalk {
    const uint8_t *ck;    // the framed chunk
    uint32_t avail;       // its stored bytes
    BloscHdr h;
    uint64_t mask;        // the selected rows
    uint32_t part, lo, hi;
    uint32_t blocksize, vb, parts, mwords;   // variants per block, blocks per row, variant-mask words per block
    uint32_t nstreams, neblock;              // streams of a block as it lies in LDS, bytes of each
    bool memcpyed;        // the chunk is stored, not compressed
    bool shuffled;        // the block in LDS is byte-shuffled: allele j of variant v at byte j * vb + v, else at 2 v + j
    bool planes16;        // the fast form: both planes of a shuffled block split into two streams, 16-byte aligned

    // fills the walk from the fields every selection struct shares, clears *s_bad (holds a barrier) and validates what
    // the three kernels validate alike: the header, part, [lo, hi), the row bits, the split against the launch
    template <typename Sel>
    __device__ __forceinline__ bool init(const uint8_t *chunk, const Sel *s, uint32_t sc, uint32_t vc, uint32_t bs,
                                         uint32_t *s_bad)
    {
        ck = chunk;
        const uint64_t src_bytes = s->src_bytes;
        mask = s->row_mask;
        part = s->part, lo = s->lo, hi = s->hi;
        if (threadIdx.x == 0) *s_bad = 0;
        __syncthreads();
        avail = src_bytes > 0xffffffffull ? 0u : (uint32_t)src_bytes;   // (too large: fails the header)
        blocksize = bs;
        vb = bs >> 1, parts = vc * 2u / bs, mwords = (vb + 31u) >> 5;
        bool ok = blosc_header(ck, avail, (uint64_t)sc * vc * 2u, 2u, bs, h);
        ok = ok && part < parts && lo < hi && hi <= vb && (sc >= 64u || (mask >> sc) == 0ull);
        nstreams = block_streams(h, bs, bs, 2u);   // (every block of such a chunk is whole)
        memcpyed = (h.flags & BLOSC_MEMCPYED) != 0u;
        shuffled = h.doshuffle && !memcpyed;
        planes16 = shuffled && nstreams == 2u && (vb & 15u) == 0u;
        neblock = memcpyed ? bs : bs / nstreams;   // (a stored row is staged as one stream)
        return ok && nstreams <= (blockDim.x >> 6);
    }
};

// the lowest row of the mask (mlo, mhi: its halves, wave-uniform, not both 0), which leaves the mask
__device__ __forceinline__ uint32_t next_row(uint32_t &mlo, uint32_t &mhi)
{
    const uint32_t r = mlo ? (uint32_t)__builtin_ctz(mlo) : 32u + (uint32_t)__builtin_ctz(mhi);
    if (mlo) mlo &= mlo - 1u;
    else mhi &= mhi - 1u;
    return r;
}

// block `part` of row r -> LDS: decode_block_lds' planes, or, of a memcpyed chunk, the stored row as one stream, so that
// the calls are read from one address space whatever the chunk.  Workgroup-cooperative, ends in a barrier; the caller
// holds another before the next row goes over this one.  false (in every thread): the row's stream is corrupt.
__device__ __forceinline__ bool stage_row(const RowWalk &W, uint32_t r, uint8_t *smem, uint32_t sstride, uint32_t *s_bad)
{
    const uint32_t b = r * W.parts + W.part;
    if (!W.memcpyed) return decode_block_lds(W.ck, W.avail, W.h.hl, b, W.blocksize, W.nstreams, sstride, smem, s_bad);
    const uint8_t *stored = W.ck + W.h.hl + (uint64_t)b * W.blocksize;
    const uint32_t nd = W.blocksize >> 2;
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < nd; i += blockDim.x) reinterpret_cast<uint32_t *>(smem)[i] = ld32u(stored + 4u * i);
    if (threadIdx.x < (W.blocksize & 3u)) smem[4u * nd + threadIdx.x] = stored[4u * nd + threadIdx.x];
    __syncthreads();
    return true;
}

// the calls of variants [v0, v0 + 4) of the block stage_row left at smem, in any layout -> a, c (first and second alleles,
// one call per byte; -9 beyond the block: counts nothing).  The block is cut into streams of neblock bytes, stream j at
// smem + j * sstride (typesize 2: at most two streams).  The slow path of for_calls16.
__device__ __forceinline__ void gather4(const RowWalk &W, const uint8_t *smem, uint32_t sstride, uint32_t v0, uint32_t &a,
                                        uint32_t &c)
{
    a = 0xF7F7F7F7u, c = 0xF7F7F7F7u;
#pragma unroll 1
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t v = v0 + j;
        if (v < W.vb) {
            const uint32_t p0 = W.shuffled ? v : 2u * v, p1 = W.shuffled ? W.vb + v : 2u * v + 1u;
            const uint32_t sh = 8u * j;
            a = (a & ~(0xFFu << sh)) | ((uint32_t)smem[p0 < W.neblock ? p0 : sstride + (p0 - W.neblock)] << sh);
            c = (c & ~(0xFFu << sh)) | ((uint32_t)smem[p1 < W.neblock ? p1 : sstride + (p1 - W.neblock)] << sh);
        }
    }
}

// f(a, b, w), w = 0..3, for the calls of variants [g + 4 w, g + 4 w + 4), g = 16 (t + k blockDim): a, b hold the two
// alleles, one call per byte.  Two 16-byte loads of the planes (planes16), gather4 otherwise; no f past the block.
template <typename F>
__device__ __forceinline__ void for_calls16(const RowWalk &W, const uint8_t *smem, uint32_t sstride, uint32_t k, F f)
{
    const uint32_t g = 16u * (threadIdx.x + blockDim.x * k);
    if (W.planes16) {
        if (g >= W.vb) return;
        const uint4 A = *reinterpret_cast<const uint4 *>(smem + g);
        const uint4 B = *reinterpret_cast<const uint4 *>(smem + sstride + g);
        f(A.x, B.x, 0);
        f(A.y, B.y, 1);
        f(A.z, B.z, 2);
        f(A.w, B.w, 3);
    } else {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            uint32_t a, c;
            gather4(W, smem, sstride, g + 4u * (uint32_t)w, a, c);
            if (g < W.vb) f(a, c, w);   // (past the block gather4 gives calls that count nothing)
        }
    }
}

// bits 0..3 of n -> 0x80 in bytes 0..3 (the four copies of n sit 7 bits apart, so the products never carry into each other)
__device__ __forceinline__ uint32_t bits_to_bytes(uint32_t n)
{
    return (((n & 0xFu) * 0x00204081u) & 0x01010101u) << 7;
}

// which of a thread's variants count — the range [lo, hi) and the block's bits of vmask (nullptr: all) — is the same for
// every row, so it is expanded once: take[k][w] has 0x80 in byte j iff variant g + 4 w + j is counted
__device__ __forceinline__ void expand_take(uint32_t lo, uint32_t hi, const uint32_t *vmask, uint64_t mask_word,
                                            uint32_t take[2][4])
{
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint32_t g = 16u * (threadIdx.x + blockDim.x * (uint32_t)k);
        uint32_t bits = 0u;
        if (g < hi && g + 16u > lo) {
            const uint32_t b0 = lo > g ? lo - g : 0u, b1 = hi - g < 16u ? hi - g : 16u;   // [b0, b1) of the 16: 0 <= b0 < b1
            bits = ((1u << b1) - 1u) & ~((1u << b0) - 1u);
            if (vmask != nullptr) bits &= vmask[mask_word + (g >> 5)] >> (g & 16u);
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) take[k][w] = bits_to_bytes(bits >> (4 * w));
    }
}

// classifies 4 calls: a, b hold the two alleles of the calls, one call per byte -> 0x80 in the byte of a call whose allele
// is called (pa, pb), is 1 (ea, eb), whose alleles differ (ne)
__device__ __forceinline__ void classify4(uint32_t a, uint32_t b, uint32_t &pa, uint32_t &pb, uint32_t &ea, uint32_t &eb,
                                          uint32_t &ne)
{
    const uint32_t H = 0x80808080u, L7 = 0x7F7F7F7Fu;
    pa = ~a & H, pb = ~b & H;                              // 0x80 where the allele is >= 0
    const uint32_t xa = a ^ 0x01010101u, xb = b ^ 0x01010101u;
    ea = ~(((xa & L7) + L7) | xa) & H;                     // 0x80 where the allele is 1 (zero-byte test without carries)
    eb = ~(((xb & L7) + L7) | xb) & H;
    const uint32_t d = a ^ b;
    ne = (((d & L7) + L7) | d) & H;                        // 0x80 where the alleles differ
}

// ---- allele counts straight out of LDS (hhgt_count_alleles) ------------------------------------------------------------

// adds the counters of 4 calls to 4 packed byte counters.  After 64 rows no byte exceeds 128, so the packed adds never
// carry into the next byte.
__device__ __forceinline__ void count4(uint32_t a, uint32_t b, uint32_t &an, uint32_t &ac, uint32_t &het, uint32_t &hom)
{
    uint32_t pa, pb, ea, eb, ne;
    classify4(a, b, pa, pb, ea, eb, ne);
    an += (pa >> 7) + (pb >> 7);
    ac += (ea >> 7) + (eb >> 7);
    het += (pa & pb & ne) >> 7;
    hom += (ea & eb) >> 7;
}

// The row walk above with dynamic LDS = the larger of decode_geometry's and 64 * blockDim + 16.  The thread counts its
// variants in registers over every selected row.  Then the counters go through LDS once, variant-major, and out with one
// agent-scope add per (variant, counter) and consecutive lanes on consecutive words.
__global__ __launch_bounds__(128) void k_count_alleles(const hhgt_count_sel *__restrict__ sel, uint32_t sc, uint32_t vc,
                                                       uint32_t blocksize, uint32_t sstride, uint32_t *__restrict__ counts,
                                                       uint64_t n_out, unsigned long long *n_bad)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ uint32_t s_bad;
    const hhgt_count_sel *s = sel + blockIdx.x;
    const uint64_t out_row = s->out_row;
    RowWalk W;
    // (a generic chunk pointer, not global_chunk: with that one the compiler batches the decoder's global loads and the
    // 32 counters no longer fit five waves per SIMD — tests/test_isa_counts.py)
    bool ok = W.init(reinterpret_cast<const uint8_t *>(s->src_ptr), s, sc, vc, blocksize, &s_bad);
    const uint32_t lo = W.lo, hi = W.hi;
    ok = ok && out_row <= n_out && hi - lo <= n_out - out_row;
    if (!ok) return bad_selection(n_bad);
    uint32_t acc[2][4][4];   // [k][counter][word]: byte j of word w = variant g + 4 w + j
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int w = 0; w < 4; ++w) acc[k][c][w] = 0u;
    uint32_t mlo = uni((uint32_t)W.mask), mhi = uni((uint32_t)(W.mask >> 32));
    bool bad = false;
    while ((mlo | mhi) != 0u) {
        const uint32_t r = next_row(mlo, mhi);
        if (!stage_row(W, r, smem, sstride, &s_bad)) {
            bad = true;
            break;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k)
            for_calls16(W, smem, sstride, (uint32_t)k, [&](uint32_t a, uint32_t b, int w) {
                count4(a, b, acc[k][0][w], acc[k][1][w], acc[k][2][w], acc[k][3][w]);
            });
        __syncthreads();   // the block is read before the next row goes over it
    }
    if (bad) return bad_selection(n_bad);
    // flush, in two passes of 16 * blockDim variants: the packed counters -> LDS as [variant][AN, AC, HET, HOM] bytes (the
    // order of d_counts), then word i of the pass -> d_counts, skipping zeros
    uint32_t *out = counts + out_row * 4u;           // variant v of the block, v in [lo, hi): out + 4 (v - lo)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint32_t pass0 = 16u * blockDim.x * (uint32_t)k, pass1 = pass0 + 16u * blockDim.x;
        const uint32_t v0 = lo > pass0 ? lo : pass0, v1 = hi < pass1 ? hi : pass1;
        if (v0 >= v1) continue;   // (uniform)
        uint32_t wd[16];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t an = acc[k][0][w], ac = acc[k][1][w], het = acc[k][2][w], hom = acc[k][3][w];
            const uint32_t p01 = __builtin_amdgcn_perm(ac, an, 0x05010400u), q01 = __builtin_amdgcn_perm(hom, het, 0x05010400u);
            const uint32_t p23 = __builtin_amdgcn_perm(ac, an, 0x07030602u), q23 = __builtin_amdgcn_perm(hom, het, 0x07030602u);
            wd[4 * w + 0] = __builtin_amdgcn_perm(q01, p01, 0x05040100u);
            wd[4 * w + 1] = __builtin_amdgcn_perm(q01, p01, 0x07060302u);
            wd[4 * w + 2] = __builtin_amdgcn_perm(q23, p23, 0x05040100u);
            wd[4 * w + 3] = __builtin_amdgcn_perm(q23, p23, 0x07060302u);
        }
        __syncthreads();   // LDS is free: the last row's planes (or the previous pass) have been read
        uint4 *dst = reinterpret_cast<uint4 *>(smem + 64u * threadIdx.x);
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[q] = make_uint4(wd[4 * q], wd[4 * q + 1], wd[4 * q + 2], wd[4 * q + 3]);
        __syncthreads();
        for (uint32_t i = 4u * (v0 - pass0) + threadIdx.x; i < 4u * (v1 - pass0); i += blockDim.x) {
            const uint32_t x = smem[i];
            if (x) __hip_atomic_fetch_add(out + (4u * (pass0 - lo) + i), x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- per-sample counts straight out of LDS (hhgt_count_samples) --------------------------------------------------------

// adds the counters of the calls of a, b (count4's classes) that m selects (0x80 in the byte of a counted call)
__device__ __forceinline__ void tally4(uint32_t a, uint32_t b, uint32_t m, uint32_t &an, uint32_t &ac, uint32_t &het,
                                       uint32_t &hom)
{
    uint32_t pa, pb, ea, eb, ne;
    classify4(a, b, pa, pb, ea, eb, ne);
    pa &= m;
    ea &= m;
    an += (uint32_t)__builtin_popcount(pa) + (uint32_t)__builtin_popcount(pb & m);
    ac += (uint32_t)__builtin_popcount(ea) + (uint32_t)__builtin_popcount(eb & m);
    het += (uint32_t)__builtin_popcount(pa & pb & ne);
    hom += (uint32_t)__builtin_popcount(ea & eb);
}

// sum of x over the wave, the same in every lane: an inclusive scan along each row of 16 lanes (DPP row_shr 1, 2, 4, 8;
// lanes without a source add 0), then the four row totals read from the last lane of each row
__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 15) + (uint32_t)__builtin_amdgcn_readlane((int)x, 31) +
           (uint32_t)__builtin_amdgcn_readlane((int)x, 47) + (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// The row walk above under expand_take's mask.  Per selected row the thread classifies its calls (count4's classes), masks,
// popcounts; the four totals of the row travel as two words of 16-bit fields (a block has at most 2 x 4096 alleles, so no
// field carries) through a DPP reduction to one LDS slot per wave and row.  At the end thread r adds row r's counters to
// d_counts: at most 4 atomics per row and selection, zeros skipped.
__global__ __launch_bounds__(128, 8) void k_count_samples(const hhgt_sample_sel *__restrict__ sel, uint32_t sc, uint32_t vc,
                                                       uint32_t blocksize, uint32_t sstride,
                                                       const uint32_t *__restrict__ vmask, uint64_t vmask_words,
                                                       uint32_t *__restrict__ counts, uint64_t n_out,
                                                       unsigned long long *n_bad)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ uint32_t s_bad;
    __shared__ uint2 s_rows[2][64];   // [wave][row]: (AN | AC << 16, HET | HOM_ALT << 16) of the wave's variants
    const uint32_t nwaves = blockDim.x >> 6;
    const uint32_t wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const hhgt_sample_sel *s = sel + blockIdx.x;
    const uint64_t out_row = s->out_row, mask_word = s->mask_word;
    RowWalk W;
    bool ok = W.init(global_chunk(s->src_ptr), s, sc, vc, blocksize, &s_bad);
    const uint64_t mask = W.mask;
    const uint32_t top = mask ? 63u - (uint32_t)__builtin_clzll(mask) : 0u;      // the highest selected row
    ok = ok && nwaves <= 2u && (mask == 0ull || (out_row < n_out && top < n_out - out_row)) &&
         (vmask == nullptr || (mask_word <= vmask_words && W.mwords <= vmask_words - mask_word));
    if (!ok) return bad_selection(n_bad);
    uint32_t take[2][4];
    expand_take(W.lo, W.hi, vmask, mask_word, take);
    uint32_t mlo = uni((uint32_t)mask), mhi = uni((uint32_t)(mask >> 32));
    while ((mlo | mhi) != 0u) {
        const uint32_t r = next_row(mlo, mhi);
        if (!stage_row(W, r, smem, sstride, &s_bad)) return bad_selection(n_bad);
        uint32_t an = 0u, ac = 0u, het = 0u, hom = 0u;
#pragma unroll
        for (int k = 0; k < 2; ++k)
            for_calls16(W, smem, sstride, (uint32_t)k,
                        [&](uint32_t a, uint32_t b, int w) { tally4(a, b, take[k][w], an, ac, het, hom); });
        const uint32_t t0 = wave_sum(an | (ac << 16)), t1 = wave_sum(het | (hom << 16));
        if (lane == 0u) s_rows[wave][r] = make_uint2(t0, t1);
        __syncthreads();   // the block is read before the next row goes over it; every wave's slot is written
    }
    if (threadIdx.x < 64u && ((mask >> threadIdx.x) & 1ull)) {
        uint2 t = s_rows[0][threadIdx.x];
        if (nwaves > 1u) {
            const uint2 u = s_rows[1][threadIdx.x];
            t.x += u.x;
            t.y += u.y;
        }
        uint32_t *out = counts + (out_row + threadIdx.x) * 4u;
        const uint32_t v[4] = {t.x & 0xFFFFu, t.x >> 16, t.y & 0xFFFFu, t.y >> 16};
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (v[c]) __hip_atomic_fetch_add(out + c, v[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- genotype bit planes straight out of LDS (hhgt_genotype_planes) ----------------------------------------------------

// 0x80 in the bytes of m that have it -> bits 0..3 (byte j -> bit j; the four shifted copies never meet below bit 28)
__device__ __forceinline__ uint32_t bytes_to_bits(uint32_t m)
{
    return (((m >> 7) * 0x01020408u) >> 24) & 0xFu;
}

// classifies 4 calls (a, b as classify4 takes them) that m selects and adds their bits, at `sh`, to the three planes: a call
// is complete iff both alleles are 0 or 1, and then HET (0/1, 1/0), HOM_REF (0/0) or HOM_ALT (1/1)
__device__ __forceinline__ void planes4(uint32_t a, uint32_t b, uint32_t m, uint32_t sh, uint32_t &het, uint32_t &ref,
                                        uint32_t &alt)
{
    const uint32_t H = 0x80808080u, L7 = 0x7F7F7F7Fu;
    const uint32_t xa = a ^ 0x01010101u, xb = b ^ 0x01010101u;
    const uint32_t za = ~(((a & L7) + L7) | a) & H, zb = ~(((b & L7) + L7) | b) & H;        // 0x80 where the allele is 0
    const uint32_t ea = ~(((xa & L7) + L7) | xa) & H, eb = ~(((xb & L7) + L7) | xb) & H;    // 0x80 where the allele is 1
    het |= bytes_to_bits(((za & eb) | (ea & zb)) & m) << sh;
    ref |= bytes_to_bits(za & zb & m) << sh;
    alt |= bytes_to_bits(ea & eb & m) << sh;
}

// The row walk above under expand_take's mask.  Per selected row the thread turns its 16 calls into 16 bits of each plane;
// lanes 2 i and 2 i + 1 hold the halves of word (t + k blockDim) / 2 of the block, the odd lane's half crosses over with one
// DPP quad_perm, and the even lane stores the word of each plane — plain vector stores: a (row, block) belongs to one
// workgroup.  A stream that turns out corrupt after some rows were written gets those rows' words zeroed again (the caller's
// buffer was zero there), so a bad selection leaves nothing behind.
__global__ __launch_bounds__(128, 8) void k_genotype_planes(const hhgt_plane_sel *__restrict__ sel, uint32_t sc, uint32_t vc,
                                                            uint32_t blocksize, uint32_t sstride,
                                                            const uint32_t *__restrict__ vmask, uint64_t vmask_words,
                                                            uint32_t *__restrict__ planes, uint64_t n_rows,
                                                            uint64_t row_words, unsigned long long *n_bad)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ uint32_t s_bad;
    const uint32_t nwaves = blockDim.x >> 6;
    const hhgt_plane_sel *s = sel + blockIdx.x;
    const uint64_t out_row = s->out_row, mask_word = s->mask_word, out_word = s->out_word;
    RowWalk W;
    bool ok = W.init(global_chunk(s->src_ptr), s, sc, vc, blocksize, &s_bad);
    const uint64_t mask = W.mask;
    const uint32_t mwords = W.mwords;
    const uint32_t top = mask ? 63u - (uint32_t)__builtin_clzll(mask) : 0u;      // the highest selected row
    ok = ok && nwaves <= 2u && (mask == 0ull || (out_row < n_rows && top < n_rows - out_row)) &&
         out_word <= row_words && mwords <= row_words - out_word &&
         (vmask == nullptr || (mask_word <= vmask_words && mwords <= vmask_words - mask_word));
    if (!ok) return bad_selection(n_bad);
    uint32_t take[2][4];
    expand_take(W.lo, W.hi, vmask, mask_word, take);
    const uint64_t plane_words = n_rows * row_words;
    uint32_t mlo = uni((uint32_t)mask), mhi = uni((uint32_t)(mask >> 32));
    uint32_t bad_row = 64u;   // the row whose stream was corrupt
    while ((mlo | mhi) != 0u) {
        const uint32_t r = next_row(mlo, mhi);
        if (!stage_row(W, r, smem, sstride, &s_bad)) {
            bad_row = r;
            break;
        }
        uint32_t *row = planes + (out_row + r) * row_words + out_word;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t t = threadIdx.x + blockDim.x * (uint32_t)k;
            uint32_t het = 0u, ref = 0u, alt = 0u;
            for_calls16(W, smem, sstride, (uint32_t)k, [&](uint32_t a, uint32_t b, int w) {
                planes4(a, b, take[k][w], 4u * (uint32_t)w, het, ref, alt);
            });
            // the neighbour's 16 bits of each plane (quad_perm [1, 0, 3, 2]); every lane of the wave is here
            const uint32_t hr = het | (ref << 16);
            const uint32_t nhr = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hr, 0xB1, 0xf, 0xf, false);
            const uint32_t nalt = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)alt, 0xB1, 0xf, 0xf, false);
            const uint32_t w = t >> 1;
            if (!(t & 1u) && w < mwords) {
                row[w] = het | (nhr << 16);
                row[plane_words + w] = ref | (nhr & 0xFFFF0000u);
                row[2u * plane_words + w] = alt | (nalt << 16);
            }
        }
        __syncthreads();   // the block is read before the next row goes over it
    }
    if (bad_row < 64u) {
        // rows below the corrupt one were written: back to the zeros the caller put there
        __syncthreads();
        for (uint32_t r = 0; r < bad_row; ++r) {
            if (!((mask >> r) & 1ull)) continue;
            uint32_t *row = planes + (out_row + r) * row_words + out_word;
            for (uint32_t w = threadIdx.x; w < mwords; w += blockDim.x) row[w] = row[plane_words + w] = row[2u * plane_words + w] = 0u;
        }
        bad_selection(n_bad);
    }
}

// ---- selected variants as dense columns straight out of LDS (hhgt_gather_calls) -----------------------------------------

// the classes of 4 calls (a, b as classify4 takes them), one per byte: 0 HOM_REF, 1 HET, 2 HOM_ALT, 3 not complete
// (planes4's definitions)
__device__ __forceinline__ uint32_t classes4(uint32_t a, uint32_t b)
{
    const uint32_t H = 0x80808080u, L7 = 0x7F7F7F7Fu;
    const uint32_t xa = a ^ 0x01010101u, xb = b ^ 0x01010101u;
    const uint32_t za = ~(((a & L7) + L7) | a) & H, zb = ~(((b & L7) + L7) | b) & H;        // 0x80 where the allele is 0
    const uint32_t ea = ~(((xa & L7) + L7) | xa) & H, eb = ~(((xb & L7) + L7) | xb) & H;    // 0x80 where the allele is 1
    const uint32_t het = (za & eb) | (ea & zb), alt = ea & eb;
    const uint32_t nc = ~((za & zb) | het | alt) & H;
    return ((het | nc) >> 7) | ((alt | nc) >> 6);
}

// dst[i] = get(i), i < n, by the whole workgroup, consecutive lanes on consecutive elements; elements narrower than a dword
// go out as whole dwords wherever dst's alignment allows (the same bytes either way)
template <typename T, typename Get>
__device__ __forceinline__ void store_elements(T *dst, uint32_t n, Get get)
{
    constexpr uint32_t PER = sizeof(T) < 4u ? 4u / (uint32_t)sizeof(T) : 1u;
    if constexpr (PER == 1u) {
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) dst[i] = get(i);
        return;
    }
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);      // (a multiple of sizeof(T))
    uint32_t head = mis ? (4u - mis) / (uint32_t)sizeof(T) : 0u;
    if (head > n) head = n;
    const uint32_t body = (n - head) / PER, tail = head + body * PER;
    if (threadIdx.x < head) dst[threadIdx.x] = get(threadIdx.x);
    uint32_t *d32 = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t q = threadIdx.x; q < body; q += blockDim.x) {
        uint32_t v = 0u;
#pragma unroll
        for (uint32_t e = 0; e < PER; ++e) v |= (uint32_t)get(head + q * PER + e) << (8u * (uint32_t)sizeof(T) * e);
        d32[q] = v;
    }
    if (tail + threadIdx.x < n) dst[tail + threadIdx.x] = get(tail + threadIdx.x);    // (fewer than PER <= blockDim)
}

// a row's gathered calls, their classes in `codes` (LDS), as elements of T: element j = values[class j][col0 + j]
template <typename T>
__device__ __forceinline__ void store_classes(void *out, uint64_t first, const void *values, uint64_t n_cols, uint64_t col0,
                                              const uint8_t *codes, uint32_t n)
{
    const T *tab = static_cast<const T *>(values) + col0;
    store_elements(static_cast<T *>(out) + first, n, [&](uint32_t j) { return tab[(uint64_t)codes[j] * n_cols + j]; });
}

// The row walk above under expand_take's mask, which also says where a thread's calls go: the gathered variants before
// the thread's own (its popcounts through one workgroup scan, once per selection: pass 0's 16-variant groups come before pass
// 1's).  Per selected row the thread classifies its calls (classes4) and puts the gathered ones' classes — raw mode: their
// allele pairs — at those places of a row buffer in LDS behind the decoder's area; after a barrier consecutive lanes turn
// consecutive entries into output elements (table mode: one opaque element of d_values per entry, read through L2) with
// plain vector stores: an (output row, column) belongs to one workgroup.  Dynamic LDS: decode_geometry's, rounded up to 16,
// plus blocksize / 2 entries of one byte (table) or two (raw): 12.5 KiB at 8 KiB blocks, twelve workgroups a CU — six waves a
// SIMD, which the second launch bound asks of the registers too (80 VGPRs, no spill; unbounded the compiler takes 109 and
// four waves, measured 20 % slower).  The table is not staged in LDS: that was measured slower.
__global__ __launch_bounds__(128, 6) void k_gather_calls(const hhgt_gather_sel *__restrict__ sel, uint32_t sc, uint32_t vc,
                                                      uint32_t blocksize, uint32_t sstride, const uint32_t *__restrict__ vmask,
                                                      uint64_t vmask_words, const uint32_t *__restrict__ row_map, uint64_t n_map,
                                                      const void *__restrict__ values, uint32_t elem_bytes, void *out,
                                                      uint64_t n_rows, uint64_t n_cols, uint64_t row_stride,
                                                      unsigned long long *n_bad)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ uint32_t s_bad;
    __shared__ uint32_t s_tot[2];      // per wave: gathered variants of pass 0 | pass 1 << 16
    __shared__ uint32_t s_past;        // a selected row lies past the output
    __shared__ uint64_t s_row[64];     // the output row of every selected chunk row
    const uint32_t nwaves = blockDim.x >> 6;
    const uint32_t wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const hhgt_gather_sel *s = sel + blockIdx.x;
    const uint64_t out_row = s->out_row, mask_word = s->mask_word, out_col = s->out_col;
    if (threadIdx.x == 0) s_past = 0u;
    RowWalk W;
    bool ok = W.init(global_chunk(s->src_ptr), s, sc, vc, blocksize, &s_bad);      // (holds the barrier behind s_past = 0)
    const uint64_t mask = W.mask;
    const uint32_t top = mask ? 63u - (uint32_t)__builtin_clzll(mask) : 0u;      // the highest selected row
    const uint64_t n_in = row_map != nullptr ? n_map : n_rows;                    // what out_row + r must stay below
    ok = ok && nwaves <= 2u && (mask == 0ull || (out_row < n_in && top < n_in - out_row)) &&
         (vmask == nullptr || (mask_word <= vmask_words && W.mwords <= vmask_words - mask_word));
    if (!ok) return bad_selection(n_bad);
    uint32_t take[2][4];
    expand_take(W.lo, W.hi, vmask, mask_word, take);
    // where the thread's gathered variants go, and how many the selection gathers
    uint32_t mine = 0u;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int w = 0; w < 4; ++w) mine += (uint32_t)__builtin_popcount(take[k][w]) << (16 * k);
    uint32_t incl = mine;
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t below = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += below;
    }
    if (lane == 63u) s_tot[wave] = incl;
    if (threadIdx.x < 64u && ((mask >> threadIdx.x) & 1ull)) {
        const uint64_t R = row_map != nullptr ? (uint64_t)row_map[out_row + threadIdx.x] : out_row + threadIdx.x;
        s_row[threadIdx.x] = R;
        if (R >= n_rows) atomicOr(&s_past, 1u);
    }
    __syncthreads();
    const uint32_t tot0 = s_tot[0], tot1 = nwaves > 1u ? s_tot[1] : 0u;
    const uint32_t n0 = (tot0 & 0xFFFFu) + (tot1 & 0xFFFFu), total = n0 + (tot0 >> 16) + (tot1 >> 16);
    const uint32_t before = wave ? tot0 : 0u, excl = incl - mine;
    const uint32_t place[2] = {(before & 0xFFFFu) + (excl & 0xFFFFu), n0 + (before >> 16) + (excl >> 16)};
    if (s_past != 0u || out_col > n_cols || total > n_cols - out_col) return bad_selection(n_bad);
    if (total == 0u) return;
    const bool raw = values == nullptr;
    uint8_t *codes = smem + (((size_t)nwaves * sstride + 16u + 15u) & ~(size_t)15u);      // the row buffer
    uint16_t *pairs = reinterpret_cast<uint16_t *>(codes);
    uint32_t mlo = uni((uint32_t)mask), mhi = uni((uint32_t)(mask >> 32));
    while ((mlo | mhi) != 0u) {
        const uint32_t r = next_row(mlo, mhi);
        if (!stage_row(W, r, smem, sstride, &s_bad)) return bad_selection(n_bad);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            uint32_t A[4] = {0u, 0u, 0u, 0u}, B[4] = {0u, 0u, 0u, 0u};
            for_calls16(W, smem, sstride, (uint32_t)k, [&](uint32_t a, uint32_t b, int w) { A[w] = a, B[w] = b; });
            uint32_t pos = place[k];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t cw = classes4(A[w], B[w]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!((take[k][w] >> (8 * j + 7)) & 1u)) continue;
                    if (raw) pairs[pos] = (uint16_t)(((A[w] >> (8 * j)) & 0xFFu) | (((B[w] >> (8 * j)) & 0xFFu) << 8));
                    else codes[pos] = (uint8_t)(cw >> (8 * j));
                    ++pos;
                }
            }
        }
        __syncthreads();   // the row buffer is whole; the block is read before the next row goes over it
        const uint64_t first = s_row[r] * row_stride + out_col;
        if (raw) store_elements(static_cast<uint16_t *>(out) + first, total, [&](uint32_t j) { return pairs[j]; });
        else if (elem_bytes == 1u) store_classes<uint8_t>(out, first, values, n_cols, out_col, codes, total);
        else if (elem_bytes == 2u) store_classes<uint16_t>(out, first, values, n_cols, out_col, codes, total);
        else if (elem_bytes == 4u) store_classes<uint32_t>(out, first, values, n_cols, out_col, codes, total);
        else store_classes<uint64_t>(out, first, values, n_cols, out_col, codes, total);
        // (the next row's stage_row holds a barrier before anybody writes the row buffer again)
    }
}

// launch shape shared by both kernels: waves per workgroup, the per-stream LDS stride, dynamic LDS bytes
static int decode_geometry(int typesize, int blocksize, uint32_t *nwaves, uint32_t *sstride, size_t *lds)
{
    // one wave per stream of a split header: typesize 2..16 always, also for blocks of fewer than 128 elements, which
    // our encoder and c-blosc store unsplit but another writer may split (the split is the header's word, not ours)
    const uint32_t split = (typesize >= 2 && typesize <= 16) ? 1u : 0u;
    *nwaves = split ? (uint32_t)typesize : 1u;
    const uint32_t max_stream = split ? (uint32_t)blocksize / (uint32_t)typesize : (uint32_t)blocksize;
    // per-stream buffer = decoded plane + in-place margin ((n >> 8) + 32) + alignment slack (4) + read-ahead (24)
    uint32_t ss = (max_stream + (max_stream >> 8) + 60u + 15u) & ~15u;
    {   // a block decoded as ONE stream (no-split header, or the short last block of a chunk) owns the whole area
        const uint32_t whole = (uint32_t)blocksize + ((uint32_t)blocksize >> 8) + 60u;
        if (whole > ss * *nwaves) ss = ((whole + *nwaves - 1) / *nwaves + 15u) & ~15u;
    }
    *sstride = ss;
    *lds = (size_t)*nwaves * ss + 16u;
    if (*lds > 160 * 1024 - 64) {
        hhgt_set_error("decode: block of %d bytes x typesize %d does not fit LDS", blocksize, typesize);
        return HHGT_ERR_ARG;
    }
    return HHGT_OK;
}

int launch_decode(const uint8_t *d_src, const uint64_t *d_chunk_off, uint64_t n_chunks, uint64_t chunk_nbytes,
                  int typesize, int blocksize, uint8_t *d_dst, unsigned long long *d_bad, hipStream_t st)
{
    if (n_chunks == 0) return HHGT_OK;
    uint32_t nwaves, sstride;
    size_t lds;
    if (int rc = decode_geometry(typesize, blocksize, &nwaves, &sstride, &lds)) return rc;
    const uint32_t nblocks = (uint32_t)((chunk_nbytes + blocksize - 1) / blocksize);
    static size_t attr_lds = 64 * 1024;  // dynamic LDS above 64 KiB needs an explicit opt-in
    if (lds > attr_lds) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_decode_blocks),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_lds = lds;
    }
    const uint64_t grid = n_chunks * nblocks;
    if (grid > 0x7fffffffull) {
        hhgt_set_error("decode: too many blocks");
        return HHGT_ERR_ARG;
    }
    hipLaunchKernelGGL(k_decode_blocks, dim3((uint32_t)grid), dim3(64u * nwaves), lds, st, d_src,
                       reinterpret_cast<const unsigned long long *>(d_chunk_off), nblocks, chunk_nbytes,
                       (uint32_t)typesize, (uint32_t)blocksize, sstride, d_dst, d_bad);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

int launch_decode_sel(const hhgt_block_sel *d_sel, uint32_t n_sel, uint64_t chunk_nbytes, int typesize, int blocksize,
                      uint8_t *d_dst, unsigned long long *d_bad, hipStream_t st)
{
    if (n_sel == 0) return HHGT_OK;
    uint32_t nwaves, sstride;
    size_t lds;
    if (int rc = decode_geometry(typesize, blocksize, &nwaves, &sstride, &lds)) return rc;
    static size_t attr_lds = 64 * 1024;
    if (lds > attr_lds) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_decode_sel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_lds = lds;
    }
    if (n_sel > 0x7fffffffu) {
        hhgt_set_error("decode: too many selections");
        return HHGT_ERR_ARG;
    }
    hipLaunchKernelGGL(k_decode_sel, dim3(n_sel), dim3(64u * nwaves), lds, st, d_sel, chunk_nbytes, (uint32_t)typesize,
                       (uint32_t)blocksize, sstride, d_dst, d_bad);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

// the launch of a row-walk kernel: one workgroup per selection, decode_geometry's shape for typesize 2 (blocksize <= 8192:
// at most 8.4 KiB of LDS, no opt-in needed), at least lds_floor bytes of dynamic LDS; args follow sstride in the kernel's list
template <typename Kernel, typename Sel, typename... Args>
static int launch_row_kernel(const char *who, Kernel kernel, size_t lds_floor, hipStream_t st, const Sel *d_sel, uint32_t n_sel,
                             uint32_t sc, uint32_t vc, int blocksize, Args... args)
{
    if (n_sel == 0) return HHGT_OK;
    uint32_t nwaves, sstride;
    size_t lds;
    if (int rc = decode_geometry(2, blocksize, &nwaves, &sstride, &lds)) return rc;
    if (lds < lds_floor) lds = lds_floor;
    if (n_sel > 0x7fffffffu) {
        hhgt_set_error("%s: too many selections", who);
        return HHGT_ERR_ARG;
    }
    hipLaunchKernelGGL(kernel, dim3(n_sel), dim3(64u * nwaves), lds, st, d_sel, sc, vc, (uint32_t)blocksize, sstride, args...);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

int launch_count_alleles(const hhgt_count_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc, int blocksize,
                         uint32_t *d_counts, uint64_t n_out, unsigned long long *d_bad, hipStream_t st)
{
    const size_t flush = 64u * 64u * 2u + 16u;   // one pass of the flush: 16 variants x 4 counter bytes per thread, two waves
    return launch_row_kernel("count_alleles", k_count_alleles, flush, st, d_sel, n_sel, sc, vc, blocksize, d_counts, n_out,
                             d_bad);
}

int launch_count_samples(const hhgt_sample_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc, int blocksize,
                         const uint32_t *d_vmask, uint64_t vmask_words, uint32_t *d_counts, uint64_t n_out,
                         unsigned long long *d_bad, hipStream_t st)
{
    return launch_row_kernel("count_samples", k_count_samples, 0, st, d_sel, n_sel, sc, vc, blocksize, d_vmask, vmask_words,
                             d_counts, n_out, d_bad);
}

int launch_genotype_planes(const hhgt_plane_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc, int blocksize,
                           const uint32_t *d_vmask, uint64_t vmask_words, uint32_t *d_planes, uint64_t n_rows,
                           uint64_t row_words, unsigned long long *d_bad, hipStream_t st)
{
    return launch_row_kernel("genotype_planes", k_genotype_planes, 0, st, d_sel, n_sel, sc, vc, blocksize, d_vmask,
                             vmask_words, d_planes, n_rows, row_words, d_bad);
}

int launch_gather_calls(const hhgt_gather_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc, int blocksize,
                        const uint32_t *d_vmask, uint64_t vmask_words, const uint32_t *d_row_map, uint64_t n_map,
                        const void *d_values, int elem_bytes, void *d_out, uint64_t n_rows, uint64_t n_cols,
                        uint64_t row_stride, unsigned long long *d_bad, hipStream_t st)
{
    uint32_t nwaves, sstride;
    size_t lds;
    if (int rc = decode_geometry(2, blocksize, &nwaves, &sstride, &lds)) return rc;
    // the row buffer behind the decoder's area: one entry per variant of a block, a class byte or an allele pair
    const size_t row_buffer = (size_t)(blocksize / 2) * (d_values ? 1u : 2u);
    return launch_row_kernel("gather_calls", k_gather_calls, ((lds + 15u) & ~(size_t)15u) + row_buffer, st, d_sel, n_sel, sc,
                             vc, blocksize, d_vmask, vmask_words, d_row_map, n_map, d_values, (uint32_t)elem_bytes, d_out,
                             n_rows, n_cols, row_stride, d_bad);
}
