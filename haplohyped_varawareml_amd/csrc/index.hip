// index.hip — line framing and fixed-column parse on device-resident VCF text (gfx950).
//
// Replaces, for a whole block of text at once, what the reference does one record at a time:
//   tbx_itr_next -> raw text line                 /root/reference/cpp/vcfpp.h:1468
//   vcf_parse1: CHROM POS ID REF ALT ... FORMAT   /root/reference/cpp/vcfpp.h:1471  (htslib)
//   BcfRecord::isSNP filter                       /root/reference/cpp/vcfpp.h:990-1000
//   Start()/End()/REF()/ALT()                     /root/reference/cpp/vcfpp.h:1118-1133,1142-1151
//   region restriction (tabix contig[:beg-end])   /root/reference/cpp/vcfpp.h:1424-1451
//
// Stage 1 (k_index_newlines): ONE streaming read of the text, 16 B per lane, coalesced; each wave
//   owns a 16 KiB region and records the newline positions it finds in a private slot array.
//   HBM bound: algorithmic bytes = nbytes read + 4 B per line written.
// Stage 2 (k_compact_newlines): prefix over per-region counts -> dense nl[] array (O(lines)).  No scan launch: stage 1
//   leaves a total per 256 regions, every workgroup sums the totals in front of it (common.h, CHAIN_GROUP).
// Stage 3 (k_parse_fixed): one lane per line walks the 9 fixed columns (O(F) bytes per line,
//   F ~ 60-300 B, versus the ~10 KB sample region that only the encode stage reads).
// Stage 4 (k_compact_kept): kept records are compacted (exclusive scan of keep flags: stage 3's totals per 256 lines
//   and a scan inside the workgroup) and the per-record table (start, stop, ref, alt) is written at v_base + k.
#include "common.h"

typedef uint32_t u32x4_unaligned __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t eq_mask4(uint32_t x, uint32_t c4)
{
    // exact per-byte "== c" -> bit k set for byte k (c4 = the byte in all four positions)
    const uint32_t t = x ^ c4;
    const uint32_t z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);  // 0x80 where byte == 0
    return (((z >> 7) * 0x01020408u) >> 24) & 0xFu;
}

__device__ __forceinline__ uint32_t eq_mask16(const u32x4_t &v, uint32_t c4)
{
    return eq_mask4(v.x, c4) | (eq_mask4(v.y, c4) << 4) | (eq_mask4(v.z, c4) << 8) | (eq_mask4(v.w, c4) << 12);
}

// "Is there a newline in these 16 bytes": the exact mask (bit k set for byte k) ...
__device__ __forceinline__ uint32_t nl_mask16(const u32x4_t &v) { return eq_mask16(v, 0x0A0A0A0Au); }

// ... and, where only a flag is needed, the cheap test (three operations per dword where the exact mask takes seven)
__device__ __forceinline__ uint32_t nl_any16(const u32x4_t &v)
{
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
    uint32_t f = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t t = d[q] ^ 0x0A0A0A0Au;
        f |= (t - 0x01010101u) & ~t & 0x80808080u;   // non-zero iff one of the four bytes is '\n'
    }
    return f;
}

// the 16 bytes at g0 (<= n) where fewer than 16 are left of the text: assembled byte by byte, blanks behind the end, and
// with `virt` position n holds the virtual newline
__device__ __forceinline__ u32x4_t tail_window16(const uint8_t *__restrict__ text, uint64_t n, bool virt, uint64_t g0)
{
    uint32_t d0 = 0x20202020u, d1 = d0, d2 = d0, d3 = d0;
#pragma unroll 1   // (once per text: kept a loop, the callers unroll around it)
    for (int j = 15; j >= 0; --j) {   // from the last byte down: each one is shifted in at the bottom
        const uint64_t g = g0 + (uint32_t)j;
        uint32_t ch = 0x20u;
        if (g < n) ch = text[g];
        else if (g == n && virt) ch = 0x0Au;
        d3 = (d3 << 8) | (d2 >> 24);
        d2 = (d2 << 8) | (d1 >> 24);
        d1 = (d1 << 8) | (d0 >> 24);
        d0 = (d0 << 8) | ch;
    }
    return u32x4_t{d0, d1, d2, d3};
}

// grid: ceil(n_regions / 4) blocks of 256 threads; wave w of block b scans region 4b + w.
__global__ __launch_bounds__(256) void k_index_newlines(const uint8_t *__restrict__ text, uint64_t n,
                                                        uint32_t *__restrict__ slots,
                                                        uint32_t *__restrict__ counts, uint32_t *__restrict__ region_tot,
                                                        uint32_t n_regions, DevCounters *cnt)
{
    HHGT_WAVE_PRIO();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= n_regions) return;
    // a text that does not end in '\n' gets a virtual newline at position n
    const bool virt = n > 0 && text[n - 1] != '\n';
    const uint64_t rbase = (uint64_t)r * INDEX_REGION;
    uint32_t *my = slots + (size_t)r * INDEX_CAP;
    uint32_t wcount = 0;
    bool overflow = false;
    uint32_t masks[INDEX_REGION / 1024];
    // issue all loads first (16 independent 16 B loads per lane), then resolve
#pragma unroll
    for (int it = 0; it < (int)(INDEX_REGION / 1024); ++it) {
        uint64_t g0 = rbase + (uint64_t)it * 1024u + lane * 16u;
        uint32_t m = 0;
        if (g0 + 16 <= n) {
            const u32x4_t v4 = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(text + g0));  // streamed once
            m = nl_mask16(v4);
        } else if (g0 <= n) {
            for (int j = 0; j < 16; ++j) {
                uint64_t g = g0 + j;
                if (g < n) {
                    if (text[g] == '\n') m |= 1u << j;
                } else if (g == n && virt)
                    m |= 1u << j;
            }
        }
        masks[it] = m;
    }
#pragma unroll
    for (int it = 0; it < (int)(INDEX_REGION / 1024); ++it) {
        uint32_t m = masks[it];
        if (__ballot(m != 0) == 0ull) continue;  // wave-uniform: long lines mostly skip
        uint32_t c = __popc(m);
        uint32_t inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            uint32_t t = __shfl_up(inc, d, 64);
            if (lane >= (uint32_t)d) inc += t;
        }
        uint32_t idx = wcount + inc - c;
        uint32_t g0 = (uint32_t)(rbase + (uint64_t)it * 1024u + lane * 16u);
        while (m) {
            int j = __ffs(m) - 1;
            m &= m - 1;
            if (idx < INDEX_CAP) my[idx] = g0 + (uint32_t)j;
            else overflow = true;
            ++idx;
        }
        wcount += __shfl(inc, 63, 64);
    }
    if (__ballot(overflow) != 0ull && lane == 0) atomicAdd(&cnt->err_density, 1ull);
    if (lane == 0) {
        const uint32_t c = wcount < INDEX_CAP ? wcount : INDEX_CAP;
        counts[r] = c;
        if (c) atomicAdd(&region_tot[r / CHAIN_GROUP], c);   // (k_compact_newlines sums these instead of a scan of counts[])
    }
}

// ---------------------------------------------------------------------------------------------
// k_index_hop<U, WALK>: the same index for text whose lines cannot be shorter than `skip` bytes — a record with S sample
// columns has at least 2 S + 17 bytes in front of its newline, so behind every line start that many bytes need not be
// looked at.  A wave owns HOP_K (<= 64, the launcher's choice) consecutive regions and walks them line by line, appending
// every newline to the slot list of the region it lies in (same slots / counts layout as k_index_newlines: everything
// downstream is unchanged).  The first newline of a wave's range is found by plain scanning, so ranges need no hand-over.
//
// WALK = false (round 2, HHGT_INDEX_MODE=1): from `pos` the wave loads U KiB (16 B per lane, all loads in flight
// together), takes the first newline, looks at the first byte of the next line ('#' header lines and empty lines are
// short: no skip behind them) and hops by the bound — for the 1000G shape (lines of 4 S + 58 bytes) it reads half of
// the text.
//
// WALK = true (round 4, the default): behind a newline the wave loads the HEAD of the next line — 1 KiB, 16 B per lane,
// starting 15 bytes in front of the line so that lane 0 holds the newline itself — ranks the tabs in it (one 16-bit mask
// per lane, a DPP prefix count, two ballots) and thereby knows where the sample columns start.  If FORMAT is exactly
// "GT", a record of S diploid calls "a|b" has its newline at soff + 4 S - 1: the next head is loaded THERE, and when its
// byte 15 is the newline the line has cost one load of 1 KiB instead of a search through U KiB (and nothing of the
// sample columns was read: the index pass reads ~1.1 KB per 10 KB line).  Anything else — another FORMAT, a byte that
// is not a newline, a '\r' in front of it, fewer than nine tabs in the head (an INFO column of more than ~900 bytes), a
// newline inside the head, the last KiB of the text — falls back to the search, from the tighter bound soff + 2 S - 1
// where the head gave one.  What the walk does NOT look at are sample columns, exactly like the hop: a line that is
// shorter than its head claims is malformed either way; when its newline falls into a hop it merges with the next line,
// and the newline is found where the merged line is read: by the encoders inside the sample columns of a KEPT record
// (every field is matched against "a|b\t", encode.hip), by k_parse_fixed in the skipped bytes of a record the filters
// DROP (nobody else reads those) — the same error, one record later.
//
// The kernel is a loop over phases (below; each header: what it reads, what it changes in HopState, which phase follows).
// A step finds ONE newline — check_candidate or search_newline — records it, and asks the line behind it about the next:
// read_head (WALK), else plain_hop.  WALK, while candidates hold: walk_batch (batch_heads, batch_chain) does four lines.

// byte `off` (wave-uniform, < 1024) of a head window held 16 bytes per lane
__device__ __forceinline__ uint32_t head_byte(const u32x4_t &v, uint32_t off)
{
    const uint32_t q = (off >> 2) & 3u;
    const uint32_t d = q == 0u ? v.x : (q == 1u ? v.y : (q == 2u ? v.z : v.w));
    return ((uint32_t)__builtin_amdgcn_readlane((int)d, (int)(off >> 4)) >> (8u * (off & 3u))) & 0xFFu;
}

// offset of the k-th (1-based) set bit of the wave's 1024-bit mask (16 bits per lane, lane order), given the exclusive
// prefix count `cum` of the lanes' popcounts; the caller knows that there are at least k
__device__ __forceinline__ uint32_t head_kth(uint32_t m16, uint32_t cum, uint32_t k)
{
    const unsigned long long b = __builtin_amdgcn_ballot_w64(cum < k && cum + (uint32_t)__popc(m16) >= k);
    const int l = __builtin_ctzll(b);
    uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)m16, l);
    const uint32_t r = k - (uint32_t)__builtin_amdgcn_readlane((int)cum, l);
    for (uint32_t i = 1; i < r; ++i) m &= m - 1u;
    return 16u * (uint32_t)l + (uint32_t)__builtin_ctz(m);
}

// What a wave of k_index_hop was given (wave-uniform but for `lane`).  For the compiler's sake the phases take this and the
// state by reference and are inlined: every member stays the scalar register it was as a local of the kernel (lz4bits.hip
// found the bools of structs passed by value in VGPRs).
struct HopRange {
    const uint8_t *__restrict__ text;
    uint64_t n, endw;     // positions [beg, endw) are this wave's; position n counts
    uint64_t last_term;   // the terminator of the text's last line (n: the virtual newline)
    bool virt;            // a text that does not end in '\n' gets a virtual newline at n
    uint32_t S, skip, lane, r_first;
    uint32_t *__restrict__ slots;
};

// what survives a step of the wave (wave-uniform but for cntv)
struct HopState {
    uint32_t cntv;   // lane i: newlines found in region r_first + i
    bool overflow;   // ... more than a slot list holds
    uint64_t pos;    // the cursor: search_newline starts here
    // WALK: the position the head of the last line says its newline is at (have_cand), and where to search if it is not
    uint64_t cand, fb;
    bool have_cand;
    // WALK: the length of the last line, the batch's guess for the next ones.  (Two head windows in flight per wave, the
    // second one placed by this length, were measured in round 4 at 2.78 against 2.40 ms for the index stage and taken out.)
    uint64_t est_len;
    // A batch reads 256 bytes of a head where the one-line path reads 1 KiB — and a record that is too short for its S
    // samples but ends inside that KiB is recognised there (its newline is IN the head).  So a candidate that came out of
    // a batch and turns out not to be a newline sends the wave back to the head it came from, once, with the wide window.
    uint64_t head_p;   // the (verified) newline in front of the line whose head produced `cand`
    bool cand_batch;   // ... and that head was read by a batch
    bool rehead;       // this step reads the head behind head_p again: its newline is recorded already
    // the batch governor: the first link of a chain that does not hold hands over to the one-line path (no_batch: for one
    // step); two steps in a row that get nowhere switch the batches off for the rest of the wave's range (bat_off)
    bool no_batch, bat_off;
    uint32_t bat_fail;
};

// appends newline q (< endw) to the slot list of its region
__device__ __forceinline__ void record(const HopRange &r, HopState &st, uint64_t q)
{
    const uint32_t rr = (uint32_t)(q / INDEX_REGION), local = rr - r.r_first;
    const uint32_t have = (uint32_t)__builtin_amdgcn_readlane((int)st.cntv, (int)local);
    if (have < INDEX_CAP) {
        if (r.lane == 0) r.slots[(size_t)rr * INDEX_CAP + have] = (uint32_t)q;
    } else
        st.overflow = true;
    st.cntv += r.lane == local ? 1u : 0u;
}

// what check_candidate / search_newline hand to read_head and plain_hop: the newline of this step
struct HopLine {
    uint64_t p;        // where it is
    u32x4_t hd;        // WALK: the head window [p - 15, p + 1009), 16 bytes per lane (have_head)
    bool have_head;
    uint32_t nb_reg;   // the byte behind the newline, where it came with the same 16 bytes (nb_have)
    bool nb_have;
};
constexpr uint32_t HEAD_NL = 15u;   // offset of the newline inside a head window: lane 0 holds it

// ---- WALK, four lines per step: the walk is bound by the ~300 instructions a wave issues per line, not by the latency of
// its one load (two windows in flight changed nothing) — so the same instructions serve FOUR lines:
// 16 lanes x 16 bytes each look at a 256-byte window where the newline of line k + g should be if the lines are of one
// length (40 bytes in front of the guess), find the newline, rank the tabs behind it (row-wise DPP scan), and the lane
// that holds the ninth tab checks "\tGT\t" and says where the NEXT newline must be.  Then the chain is verified on the
// scalar side: group g's newline must sit exactly where group g - 1 said (group 0: where the candidate is).  The first
// link that does not hold — another width, another FORMAT, a '\r', a head of more than ~190 bytes, a '#' line — hands
// over to the one-line path below, which decides with its 1 KiB head or a search; two steps in a row that get nowhere
// switch the batches off for the rest of the wave's range.

// what the four windows of a batch hold
struct BatchHeads {
    u32x4_t v;                // the lane's 16 bytes: lanes 16 g .. 16 g + 15 hold the window of line g
    uint32_t og[4];           // per group (wave-uniform): offset of the first newline in its window ...
    bool vg[4];               // ... and whether there is one
    unsigned long long nl2;   // lanes that hold a second newline: the line ends inside its head
    unsigned long long b9;    // lanes that hold the ninth tab behind the newline with "\tGT" in front of it
    uint32_t t9;              // per lane: the offset of that tab in the group's window
};

// Batch, vector side.  Reads the four 256-byte windows at cand - 40 + g L0; changes nothing in the state.  -> batch_chain.
__device__ __forceinline__ BatchHeads batch_heads(const HopRange &r, uint64_t cand, uint64_t L0)
{
    BatchHeads h;
    const uint32_t g = r.lane >> 4, li = r.lane & 15u;
    const uint8_t *wbase = r.text + (cand - 40ull);
    const uint64_t voff = (uint64_t)g * L0 + 16ull * li;
    const u32x4_t v = *reinterpret_cast<const u32x4_unaligned *>(wbase + voff);
    const uint32_t nlm = nl_mask16(v), tbm = eq_mask16(v, 0x09090909u);
    const unsigned long long nlb = __builtin_amdgcn_ballot_w64(nlm != 0u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t mg = (uint32_t)(nlb >> (16 * k)) & 0xFFFFu;
        h.vg[k] = mg != 0u;
        const int fl = 16 * k + __builtin_ctz(mg | 0x10000u);
        h.og[k] = 16u * ((uint32_t)fl & 15u) + (uint32_t)__builtin_ctz((uint32_t)__builtin_amdgcn_readlane((int)nlm, fl & 63) | 0x10000u);
    }
    const uint32_t o = g == 0u ? h.og[0] : (g == 1u ? h.og[1] : (g == 2u ? h.og[2] : h.og[3]));
    const uint32_t l0 = 16u * li;
    const uint32_t keep = l0 > o ? 0xFFFFu : (l0 + 15u <= o ? 0u : (0xFFFFu << (o - l0 + 1u)) & 0xFFFFu);
    h.nl2 = __builtin_amdgcn_ballot_w64((nlm & keep) != 0u);
    const uint32_t tk = tbm & keep, tc = (uint32_t)__popc(tk);
    uint32_t incl = tc;   // inclusive count inside the row of 16 lanes
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xf, 0xf, false);
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xf, 0xf, false);
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xf, 0xf, false);
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xf, 0xf, false);
    const uint32_t cum = incl - tc;
    const bool has9 = cum < 9u && incl >= 9u;
    // in the lane of the ninth tab: its offset, "\tGT" in front of it, the next newline
    uint32_t m9 = tk;
    const uint32_t r1 = 8u - cum;   // lower tabs of this lane to step over (has9: 0 .. 8)
#pragma unroll
    for (uint32_t i = 0; i < 8u; ++i) m9 = i < r1 ? (m9 & (m9 - 1u)) : m9;
    const uint32_t j9 = (uint32_t)__builtin_ctz(m9 | 0x10000u) & 15u;   // byte of the lane
    const uint32_t pw = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.w, 0x111, 0xf, 0xf, false);      // previous lane's last dword
    const uint32_t ptb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)tbm, 0x111, 0xf, 0xf, false);    // ... and its tab mask
    const uint32_t tb20 = (tbm << 4) | (ptb >> 12);           // tab bits of the 20 bytes [previous lane's last four | own 16]
    const bool tab8 = ((tb20 >> (j9 + 1u)) & 1u) != 0u;       // byte j9 - 3 of the lane
    const uint32_t ix = j9 + 2u, di = ix >> 2;                // bytes j9 - 2, j9 - 1 in the 20-byte array
    const uint32_t w0 = di == 0u ? pw : (di == 1u ? v.x : (di == 2u ? v.y : (di == 3u ? v.z : v.w)));
    const uint32_t w1 = di == 0u ? v.x : (di == 1u ? v.y : (di == 2u ? v.z : v.w));
    const uint32_t gt2 = __builtin_amdgcn_alignbyte(w1, w0, ix & 3u) & 0xFFFFu;
    const bool ok9 = has9 && tab8 && gt2 == 0x5447u;           // 'G' | 'T' << 8
    h.v = v;
    h.t9 = l0 + j9;
    h.b9 = __builtin_amdgcn_ballot_w64(ok9);
    return h;
}

// Batch, scalar side: the chain.  Reads what batch_heads found; records every newline that sits where its predecessor
// said and whose head is of the shape, and moves est_len along with them.  Changes the candidate (cand, fb, have_cand,
// head_p, cand_batch: the next one, unverified), the governor, and `pos` where a link hands over without a candidate.
// -> false: the chain reached the end of the wave's range, the walk is over.  -> true: the next step is a batch again
// (no_batch clear), check_candidate (a link did not hold) or search_newline (no candidate left: see below).
__device__ __forceinline__ bool batch_chain(const HopRange &r, HopState &st, const BatchHeads &h, uint64_t L0)
{
    const uint64_t cand = st.cand;
    uint64_t expected = cand, fbx = st.fb, exp_head = st.head_p;
    bool exp_batch = st.cand_batch;
    bool stop = false, handed = false;
    uint32_t advanced = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (stop || handed) continue;
        const uint64_t nlpos = cand - 40ull + (uint64_t)k * L0 + h.og[k];
        const bool cr = h.vg[k] && h.og[k] != 0u && head_byte(h.v, 256u * (uint32_t)k + h.og[k] - 1u) == '\r';
        if (!h.vg[k] || nlpos != expected || cr) {   // not where it should be (or a CRLF text): the one-line path decides
            handed = true;
            continue;
        }
        exp_head = expected;
        exp_batch = true;
        if (expected >= r.endw) {
            stop = true;
            continue;
        }
        const uint32_t bits = (uint32_t)(h.b9 >> (16 * k)) & 0xFFFFu;
        if (bits == 0u || ((h.nl2 >> (16 * k)) & 0xFFFFull) != 0ull) {
            // the newline is there, the head behind it is not of this shape: found again (and recorded) by the search
            st.have_cand = false;
            st.pos = expected;
            handed = true;
            expected = ~0ull;
            continue;
        }
        record(r, st, expected);
        ++advanced;
        const int l9 = 16 * k + __builtin_ctz(bits);
        const uint32_t t9s = (uint32_t)__builtin_amdgcn_readlane((int)h.t9, l9);
        const uint64_t soff = cand - 40ull + (uint64_t)k * L0 + t9s + 1ull;
        const uint64_t nxt = soff + 4ull * r.S - 1ull;
        st.est_len = nxt - expected;
        expected = nxt;
        fbx = soff + 2ull * r.S - 17ull;
    }
    if (stop) return false;
    if (expected != ~0ull) {   // the next candidate (unverified), for the next step or for the one-line path
        if (expected > r.last_term) {   // (a line that claims to reach past the text: the search decides)
            st.have_cand = false;
            st.pos = fbx;
            if (st.pos > r.last_term) st.pos = r.last_term;
        } else {
            st.cand = expected;
            st.fb = fbx > r.last_term ? r.last_term : fbx;
            st.have_cand = true;
        }
        st.head_p = exp_head;
        st.cand_batch = exp_batch;
    }
    st.no_batch = handed;
    st.bat_fail = advanced ? 0u : st.bat_fail + 1u;
    st.bat_off = st.bat_fail >= 2u;
    return true;
}

// The batch step: four lines' newlines and heads with one load.  -> false: the walk is over.
__device__ __forceinline__ bool walk_batch(const HopRange &r, HopState &st)
{
    const uint64_t L0 = st.est_len;   // (the windows lie where THIS length puts them; est_len moves on with the chain)
    return batch_chain(r, st, batch_heads(r, st.cand, L0), L0);
}

// ---- one line per step

// The candidate check (WALK, have_cand): is the byte at `cand` the newline the head promised?  Reads the 1 KiB window
// [cand - 15, cand + 1009) — it is the head of the NEXT line as well — or, near the end of the text, the two bytes.
// Consumes the candidate.  -> true, ln.p = cand (ln.hd where the window was read): record, then read_head.  -> true with
// `rehead` set, ln.p = head_p: a batch's candidate failed, the head it came from is read again 1 KiB wide (no newline is
// recorded: head_p already is).  -> false, pos = fb: search_newline from the bound.
// ('\r' in front: bgzf_getline strips it and the sample columns are one byte shorter — not this shape)
__device__ __forceinline__ bool check_candidate(const HopRange &r, HopState &st, HopLine &ln)
{
    const uint64_t cand = st.cand, n = r.n;
    st.have_cand = false;
    uint32_t c15 = 0, c14 = 0;
    if (cand + 1009ull <= n) {   // the window [cand - 15, cand + 1009) lies inside the text
        ln.hd = *reinterpret_cast<const u32x4_unaligned *>(r.text + (cand - 15ull) + 16ull * r.lane);
        c15 = head_byte(ln.hd, HEAD_NL);
        c14 = head_byte(ln.hd, HEAD_NL - 1u);
        ln.have_head = true;
    } else if (cand < n) {
        c15 = r.text[cand];
        c14 = r.text[cand - 1];
    } else if (cand == n && r.virt) {
        c15 = 0x0Au;
        c14 = r.text[n - 1];
    }
    if (c15 == 0x0Au && c14 != '\r') {
        ln.p = cand;
        return true;
    }
    if (st.cand_batch) {
        st.cand_batch = false;
        st.rehead = true;
        ln.have_head = false;
        ln.p = st.head_p;
        return true;
    }
    st.pos = st.fb;
    return false;
}

// The search: the first newline at or behind `pos` in the U KiB from (pos & ~15) on, all loads in flight together.  Reads
// the text only (its last bytes through tail_window16).  -> true, ln.p and, in 15 of 16 cases, the byte behind it (ln.nb_reg):
// record, then read_head / plain_hop.  -> false: none in there, `pos` moved on by U KiB, the search again.
template <int U>
__device__ __forceinline__ bool search_newline(const HopRange &r, HopState &st, HopLine &ln)
{
    const uint64_t pos = st.pos, n = r.n, a0 = pos & ~15ull;
    uint32_t any[U];
    u32x4_t v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t g0 = a0 + (uint64_t)u * 1024u + r.lane * 16u;
        v[u] = u32x4_t{0u, 0u, 0u, 0u};
        if (g0 + 16 <= n) v[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(r.text + g0));   // streamed once
        else if (g0 <= n) v[u] = tail_window16(r.text, n, r.virt, g0);
        uint32_t f = nl_any16(v[u]);   // (the first pass wants a flag per lane only: the exact mask costs more)
        // bytes in front of pos are not part of the search
        if (g0 + 16 <= pos) f = 0;
        any[u] = f;
    }
    bool found = false;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (found) continue;
        unsigned long long b = __builtin_amdgcn_ballot_w64(any[u] != 0u);
        while (b != 0ull && !found) {
            // the exact mask of the first flagged lane (its flag may stem from bytes in front of pos only)
            const int l = __builtin_ctzll(b);
            b &= b - 1ull;
            const uint32_t x0 = (uint32_t)__builtin_amdgcn_readlane((int)v[u].x, l), x1 = (uint32_t)__builtin_amdgcn_readlane((int)v[u].y, l);
            const uint32_t x2 = (uint32_t)__builtin_amdgcn_readlane((int)v[u].z, l), x3 = (uint32_t)__builtin_amdgcn_readlane((int)v[u].w, l);
            uint32_t m = nl_mask16(u32x4_t{x0, x1, x2, x3});
            const uint64_t g0 = a0 + (uint64_t)u * 1024u + (uint64_t)l * 16u;
            if (g0 < pos) m &= ~((1u << (uint32_t)(pos - g0)) - 1u);
            if (m) {
                found = true;
                const uint32_t j = (uint32_t)__builtin_ctz(m);
                ln.p = g0 + j;
                if (j < 15u && g0 + 16 <= n) {
                    const uint32_t k = j + 1u, dw = k >> 2;
                    const uint32_t xd = dw == 0u ? x0 : (dw == 1u ? x1 : (dw == 2u ? x2 : x3));
                    ln.nb_reg = (xd >> (8u * (k & 3u))) & 0xFFu;
                    ln.nb_have = true;
                }
            }
        }
    }
    if (!found) st.pos = a0 + (uint64_t)U * 1024u;
    return found;
}

// The head read (WALK): what the head of the line behind the newline ln.p says about the NEXT newline.  Reads ln.hd (a
// search found p: one more load; the candidate's window is it already).  -> true, one of: a '#' or empty line, pos = p + 1
// (search right behind it); a newline inside the head, pos = exactly there; FORMAT "GT", a new candidate (cand, fb,
// est_len, head_p; cand_batch clear) for walk_batch or check_candidate; another FORMAT, pos = the bound soff + 2 S - 17.
// -> false (no head window inside the text, or fewer than nine tabs in it): plain_hop.
__device__ __forceinline__ bool read_head(const HopRange &r, HopState &st, HopLine &ln)
{
    const uint64_t p = ln.p;
    if (!ln.have_head && p >= 15ull && p + 1009ull <= r.n) {
        ln.hd = *reinterpret_cast<const u32x4_unaligned *>(r.text + (p - 15ull) + 16ull * r.lane);
        ln.have_head = true;
    }
    if (!ln.have_head) return false;
    const u32x4_t &hd = ln.hd;
    const uint64_t wb = p - (uint64_t)HEAD_NL;
    const uint32_t nb = head_byte(hd, HEAD_NL + 1u);
    // the lane's bytes that lie behind the newline (offsets > HEAD_NL): only those belong to the head
    const uint32_t l0 = 16u * r.lane;
    const uint32_t keep = l0 > HEAD_NL ? 0xFFFFu : (l0 + 15u <= HEAD_NL ? 0u : (0xFFFFu << (HEAD_NL - l0 + 1u)) & 0xFFFFu);
    if (nb == '#' || nb == 0x0Au) {
        st.pos = p + 1;   // header and empty lines are short: search right behind them
        return true;
    }
    const uint32_t nlm = nl_mask16(hd) & keep;
    const unsigned long long nlb = __builtin_amdgcn_ballot_w64(nlm != 0u);
    if (nlb != 0ull) {
        // the line ends inside its head (far too short for S samples): exactly there
        const int l = __builtin_ctzll(nlb);
        st.pos = wb + 16ull * (uint64_t)l + (uint64_t)__builtin_ctz((uint32_t)__builtin_amdgcn_readlane((int)nlm, l));
        return true;
    }
    const uint32_t tbm = eq_mask16(hd, 0x09090909u) & keep;
    const uint32_t tc = (uint32_t)__popc(tbm);
    const uint32_t incl = wave_scan_sum_dpp(tc, r.lane);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (total < 9u) return false;
    const uint32_t t8 = head_kth(tbm, incl - tc, 8u), t9 = head_kth(tbm, incl - tc, 9u);
    const uint64_t soff = wb + t9 + 1ull;
    // S fields of at least one byte and S - 1 tabs in front of the newline (16 bytes of margin as in `skip`)
    const uint64_t lo = soff + 2ull * r.S - 17ull;
    const bool gt = t9 - t8 == 3u && head_byte(hd, t8 + 1u) == 'G' && head_byte(hd, t8 + 2u) == 'T';
    if (gt && soff + 4ull * r.S - 1ull <= r.last_term) {
        st.cand = soff + 4ull * r.S - 1ull;
        st.fb = lo;
        st.have_cand = true;
        st.est_len = st.cand - p;
        st.head_p = p;
        st.cand_batch = false;
    } else {
        // another FORMAT ("GT:DP", "GT:AD:DP:GQ:PL" ...; or a GT line that would end past the text): no width to compute,
        // so the first newline behind the bound is the record's.  (The walk once tried the width of the last record of that
        // kind first and took a newline found there on trust: a shorter record followed by lines that happened to end at that
        // byte was merged with them and valid text flagged — test_width_of_the_last_other_format_record_is_not_trusted.)
        st.pos = lo;
    }
    return true;
}

// The plain hop (WALK = false, or the head said nothing): reads the byte behind the newline; pos = behind the bound, or
// right behind the newline in front of a '#' line or an empty one.  -> search_newline.
__device__ __forceinline__ void plain_hop(const HopRange &r, HopState &st, const HopLine &ln)
{
    uint32_t nb = 0x0Au;
    if (ln.nb_have) nb = ln.nb_reg;                 // the byte behind the newline came with the same 16 bytes (15 of 16 cases)
    else if (ln.p + 1 < r.n) nb = r.text[ln.p + 1];
    // ('\r': the empty line of a CRLF text — round 3 hopped behind it and merged it with the record that follows)
    st.pos = ln.p + 1 + ((nb == '#' || nb == 0x0Au || nb == '\r') ? 0u : r.skip);
}

template <int U, bool WALK>
__global__ __launch_bounds__(256) void k_index_hop(const uint8_t *__restrict__ text, uint64_t n, uint32_t *__restrict__ slots,
                                                   uint32_t *__restrict__ counts, uint32_t *__restrict__ region_tot, uint32_t n_regions,
                                                   uint32_t skip, uint32_t S, DevCounters *cnt, uint32_t HOP_K)
{
    HHGT_WAVE_PRIO();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t r_first = w * HOP_K;
    if (r_first >= n_regions) return;
    const uint32_t r_cnt = n_regions - r_first < HOP_K ? n_regions - r_first : HOP_K;
    const bool virt = n > 0 && text[n - 1] != '\n';
    const uint64_t beg = (uint64_t)r_first * INDEX_REGION;
    uint64_t endw = beg + (uint64_t)r_cnt * INDEX_REGION;
    if (endw > n + 1) endw = n + 1;
    const HopRange r = {text, n, endw, virt ? n : n - 1, virt, S, skip, lane, r_first, slots};
    HopState st = {0u, false, beg, 0ull, 0ull, false, 0ull, 0ull, false, false, false, false, 0u};
    while (st.have_cand || st.pos < endw) {
        if constexpr (WALK) {
            // a batch: a candidate, the governor's leave, and four windows inside the text
            if (st.have_cand && !st.no_batch && !st.bat_off && st.est_len != 0ull && st.cand >= 40ull && st.cand + 3ull * st.est_len + 216ull <= n) {
                if (!walk_batch(r, st)) break;
                continue;
            }
        }
        st.no_batch = false;
        HopLine ln = {0ull, u32x4_t{0u, 0u, 0u, 0u}, false, 0u, false};
        const bool found = (WALK && st.have_cand) ? check_candidate(r, st, ln) : search_newline<U>(r, st, ln);
        if (!found) continue;   // (the cursor moved: the search goes on from there)
        if (!st.rehead) {
            if (ln.p >= endw) break;
            record(r, st, ln.p);
        } else
            st.no_batch = true;   // (the candidate the wide head gives is verified by the one-line path)
        st.rehead = false;
        bool hopped = false;
        if constexpr (WALK) hopped = read_head(r, st, ln);
        if (!hopped) plain_hop(r, st, ln);
        // the terminator of the text's last line is always looked at: a file cut off in mid-line ends in a line shorter
        // than the bound, which has to reach the parser (and be reported), not vanish in a hop
        if (st.pos > r.last_term) st.pos = ln.p + 1 > r.last_term ? ln.p + 1 : r.last_term;
        if (st.have_cand && st.fb > r.last_term) st.fb = ln.p + 1 > r.last_term ? ln.p + 1 : r.last_term;
    }
    if (st.overflow && lane == 0) atomicAdd(&cnt->err_density, 1ull);
    const uint32_t mine = lane < r_cnt ? (st.cntv < INDEX_CAP ? st.cntv : INDEX_CAP) : 0u;
    if (lane < r_cnt) counts[r_first + lane] = mine;
    // the totals k_compact_newlines sums instead of a scan of counts[]: the wave's HOP_K <= 64 regions lie in one group of
    // CHAIN_GROUP regions or in two neighbouring ones
    const uint32_t g0 = r_first / CHAIN_GROUP;
    const uint32_t split = (g0 + 1u) * CHAIN_GROUP - r_first;   // the lanes from here on hold regions of group g0 + 1
    const uint32_t a = lane < split ? mine : 0u;
    const uint32_t sum_a = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_sum_dpp(a, lane), 63);
    const uint32_t sum_b = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_sum_dpp(mine - a, lane), 63);
    if (lane == 0) {
        if (sum_a) atomicAdd(&region_tot[g0], sum_a);
        if (sum_b) atomicAdd(&region_tot[g0 + 1u], sum_b);
    }
}

// one thread per region: copy its slot entries to their final place.  The place is the sum of the counts in front of the
// region: the totals of the workgroups (CHAIN_GROUP regions each) in front of this one, left behind by the index kernel
// and summed here by every workgroup for itself, plus a scan of the workgroup's own counts.  *d_nlines = all of them
__global__ __launch_bounds__(CHAIN_GROUP) void k_compact_newlines(const uint32_t *__restrict__ slots,
                                                                  const uint32_t *__restrict__ counts,
                                                                  const uint32_t *__restrict__ region_tot,
                                                                  uint32_t n_regions, uint32_t *__restrict__ nl,
                                                                  uint32_t max_lines, uint32_t *__restrict__ d_nlines)
{
    HHGT_WAVE_PRIO();
    __shared__ uint32_t sm[8];
    const uint32_t r = blockIdx.x * CHAIN_GROUP + threadIdx.x;
    uint32_t pre = 0;
    for (uint32_t g = threadIdx.x; g < blockIdx.x; g += CHAIN_GROUP) pre += region_tot[g];
    uint32_t front, own;
    block_excl_scan(pre, &front, sm);
    const uint32_t c = r < n_regions ? counts[r] : 0u;
    const uint32_t p = front + block_excl_scan(c, &own, sm);
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0u) *d_nlines = front + own;   // (the workgroup of the last region)
    const uint32_t *my = slots + (size_t)r * INDEX_CAP;
    for (uint32_t k = 0; k < c && p + k < max_lines; ++k) nl[p + k] = my[k];   // lines past the caller's bound: err_lines
}

// ---------------------------------------------------------------------------------------------
// fixed columns: one lane per line (k_parse_fixed, below its steps)

// A line's bytes: the first 64 from the LDS row they were staged in, the rest from global memory.  Constructed twice: for
// the thread's own line and for the line in front of it (chrom_run_starts).
struct LineReader {
    const uint8_t *__restrict__ text;
    const uint8_t *row;   // the 64 staged bytes (if `staged`)
    uint32_t s;           // the line's first byte
    bool staged;
    __device__ __forceinline__ uint32_t operator()(uint32_t x) const { return (staged && x - s < 64u) ? (uint32_t)row[x - s] : (uint32_t)text[x]; }
};

// what parse_record makes of a record
struct FixedCols {
    uint32_t flags, soff, pos0, refalt, gtidx, stride;
};

// The walk below is byte-serial per line; straight from global memory that is ~80 dependent loads per lane with
// every wave of the grid resident at once, i.e. the kernel lasts one full latency chain (89 us for 136 k lines).
// So the first 64 bytes of every line (CHROM .. FORMAT of a typical record) are fetched up front by four
// independent 16-byte loads per lane and parked in LDS (row stride 17 dwords: conflict-free byte reads);
// LineReader serves the walk from there and falls back to global memory past byte 64.
__device__ __forceinline__ bool stage_head(const uint8_t *__restrict__ text, uint64_t n, uint32_t s, uint32_t *row)
{
    if ((uint64_t)s + 64ull > n) return false;
    u32x4_unaligned c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = *reinterpret_cast<const u32x4_unaligned *>(text + s + 16 * k);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        row[4 * k + 0] = c[k].x;
        row[4 * k + 1] = c[k].y;
        row[4 * k + 2] = c[k].z;
        row[4 * k + 3] = c[k].w;
    }
    return true;
}

// isSNP (cpp/vcfpp.h:990-1000): |REF| <= 1, n_allele <= 2, ALT in {A,C,G,T}; -> a: the first byte of ALT
__device__ __forceinline__ bool is_snp(const LineReader &rd, uint32_t reflen, uint32_t alt, uint32_t altlen, bool keep_multi, uint32_t &a)
{
    a = altlen >= 1 ? rd(alt) : 0;
    bool snp = reflen == 1 && altlen == 1 && (a == 'A' || a == 'C' || a == 'G' || a == 'T');
    if (keep_multi && reflen == 1 && altlen > 1 && (altlen & 1u)) {
        // non-reference mode: "B,B[,B...]" with every B in {A,C,G,T}
        snp = true;
        for (uint32_t q = 0; snp && q < altlen; ++q) {
            const uint32_t ch = rd(alt + q);
            snp = (q & 1u) ? ch == ',' : (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
        }
    }
    return snp;
}

// GT key index inside FORMAT [q, fe) (bcf_get_genotypes looks the key up) -> k; false: there is no GT key
__device__ __forceinline__ bool gt_key_index(const LineReader &rd, uint32_t q, uint32_t fe, uint32_t &k)
{
    k = 0;
    while (q <= fe) {
        uint32_t q2 = q;
        while (q2 < fe && rd(q2) != ':') ++q2;
        if (q2 - q == 2 && rd(q) == 'G' && rd(q + 1u) == 'T') return true;
        ++k;
        q = q2 + 1;
    }
    return false;
}

// A record [s, e): the nine-field walk, POS, the region, isSNP, FORMAT.  -> flags (LF_RECORD and one of LF_KEEP [| LF_FAST],
// LF_DROP_REGION, LF_DROP_FILTER, LF_MALFORMED), and for a kept record where its sample columns start and how they lie
__device__ __forceinline__ FixedCols parse_record(const LineReader &rd, uint32_t s, uint32_t e, uint32_t S, const RegionFilter *rf)
{
    FixedCols r = {LF_RECORD, e, 0u, 0u, 0u, 0u};
    // walk the first 9 tab-separated fields
    uint32_t fs[10];
    uint32_t nf = 0;
    uint32_t p = s;
    fs[0] = s;
    while (p < e && nf < 9) {
        if (rd(p) == '\t') fs[++nf] = p + 1;
        ++p;
    }
    // nf = number of tabs found (<= 9); field k spans [fs[k], fs[k+1]-1) for k < nf
    bool bad = false;
    uint32_t fe[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) fe[k] = (uint32_t)k < nf ? fs[k + 1] - 1u : e;
    if (nf < 7 || (S > 0 && nf < 9)) bad = true;
    if (!bad) {
        // POS
        unsigned long long pos = 0;
        if (fe[1] == fs[1]) bad = true;
        for (uint32_t q = fs[1]; q < fe[1]; ++q) {
            uint32_t c = rd(q);
            if (c < '0' || c > '9') {
                bad = true;
                break;
            }
            pos = pos * 10ull + (c - '0');
        }
        bool in_region = true;
        if (!bad && rf->contig_len > 0) {
            uint32_t cl = fe[0] - fs[0];
            in_region = cl == (uint32_t)rf->contig_len;
            for (uint32_t q = 0; in_region && q < cl; ++q)
                in_region = rd(fs[0] + q) == (uint32_t)(uint8_t)rf->contig[q];
            if (in_region && rf->has_range)
                in_region = (long long)pos >= rf->beg && (long long)pos <= rf->end;
        }
        const uint32_t reflen = fe[3] - fs[3], altlen = fe[4] - fs[4];
        uint32_t a = 0;   // the first byte of ALT
        if (bad) {
            // (reported below)
        } else if (!in_region)
            r.flags |= LF_DROP_REGION;
        else if (!is_snp(rd, reflen, fs[4], altlen, rf->keep_multi, a))
            r.flags |= LF_DROP_FILTER;
        else {
            r.pos0 = (uint32_t)(pos - 1ull);  // vcfpp.h:1118-1121
            r.refalt = rd(fs[3]) | (a << 8);
            if (S > 0) {
                uint32_t k;
                if (!gt_key_index(rd, fs[8], fe[8], k) || k > 0xFFFu) bad = true;  // vcfpp.h:550-552 "genotypes not present" (or 4096 keys in front of it)
                r.gtidx = k;
                r.soff = fs[9];
                if (!bad) {
                    r.flags |= LF_KEEP;
                    if (k == 0 && fe[8] - fs[8] == 2 && e - r.soff == 4u * S - 1u) r.flags |= LF_FAST;
                    else if (k == 0 && (e - r.soff + 1u) % S == 0u) {
                        // GT first and the sample columns S times some width of 5 .. 8 bytes ("a|b:dd\t"): the
                        // bit-plane encoder tries them at that stride (round 4; every column is checked there)
                        const uint32_t wd = (e - r.soff + 1u) / S;
                        if (wd >= 5u && wd <= 8u) r.stride = wd;
                    }
                }
            } else {
                r.flags |= LF_KEEP;
            }
        }
    }
    if (bad) r.flags = LF_RECORD | LF_MALFORMED;
    return r;
}

// CHROM run boundary: whether record i's CHROM (read by rd, from s) differs from the previous data line's.  The previous
// line sits in the neighbouring thread's LDS row (same staging rule) unless this is thread 0.
__device__ __forceinline__ bool chrom_run_starts(const LineReader &rd, uint32_t s, uint32_t e, uint32_t i, const uint32_t *__restrict__ nl,
                                                 uint64_t n, const uint32_t (*stage)[17])
{
    if (i == 0) return true;
    const uint32_t ps = i > 1 ? nl[i - 2] + 1u : 0u, pe = nl[i - 1];
    const LineReader rdp = {rd.text, reinterpret_cast<const uint8_t *>(stage[threadIdx.x > 0u ? threadIdx.x - 1u : 0u]), ps,
                            threadIdx.x > 0u && (uint64_t)ps + 64ull <= n};
    if (!(pe > ps && rdp(ps) != '#')) return true;
    for (uint32_t q = 0;; ++q) {
        const uint32_t a = s + q < e ? rd(s + q) : '\t';
        const uint32_t b = ps + q < pe ? rdp(ps + q) : '\t';
        if (a != b) return true;
        if (a == '\t') return false;
    }
}

// The hopping index (k_index_hop) never looked at the first hop_skip bytes behind a record's start: a record shorter
// than that — fewer sample columns than the header declares, a parse error in htslib — has its newline in there and
// arrives merged with its successor.  A KEPT record is read byte by byte by the encoders, which report the newline
// (HHGT_ERR_MALFORMED); a record the region / isSNP filter DROPS is read by nobody, and the valid record merged into
// it would vanish unreported.  So the dropped records' unexamined bytes are examined here, a wave per record
// (rare: nothing is dropped from a 1000G-style SNP file), and a newline in there makes the record malformed too.
// Called by whole waves; changes `flags` of the lanes whose record it is.
__device__ __forceinline__ void examine_dropped(const uint8_t *__restrict__ text, uint64_t n, uint32_t hop_skip, uint32_t s, uint32_t e,
                                                uint32_t &flags)
{
    const uint32_t lane = threadIdx.x & 63u;
    const bool chk = (flags & LF_RECORD) && !(flags & (LF_KEEP | LF_MALFORMED));
    unsigned long long todo = __ballot(chk);
    while (todo != 0ull) {   // (wave-uniform)
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const uint32_t ss = (uint32_t)__builtin_amdgcn_readlane((int)s, l), ee = (uint32_t)__builtin_amdgcn_readlane((int)e, l);
        const uint32_t hi = ee - ss < hop_skip ? ee : ss + hop_skip;   // (the index searched from (ss + hop_skip) & ~15 on)
        uint32_t hit = 0;
        // (eight KiB per step, the loads in flight together: behind the walk a dropped record is examined from end to end,
        // 20 KB at 5000 samples — one load per step made config 4's fixed-column stage 1.4 ms instead of 0.8)
        for (uint32_t x0 = ss + 16u * lane; x0 < hi; x0 += 8192u) {
            u32x4_t tv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint32_t x = x0 + 1024u * (uint32_t)u;
                tv[u] = u32x4_t{0u, 0u, 0u, 0u};
                if (x < hi && (uint64_t)x + 16ull <= n) tv[u] = *reinterpret_cast<const u32x4_unaligned *>(text + x);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint32_t x = x0 + 1024u * (uint32_t)u;
                if (x >= hi) continue;
                const uint32_t m = nl_mask16(tv[u]);
                hit |= hi - x >= 16u ? m : (m & ((1u << (hi - x)) - 1u));
            }
            // the lane's one window that reaches past the end of the text, if it lies in this step (hi <= n < xt + 16)
            const uint32_t ut = (uint64_t)x0 + 16ull > n ? 0u : (uint32_t)((n - 16ull - x0) >> 10) + 1u;
            const uint32_t xt = x0 + 1024u * ut;
            if (ut < 8u && xt < hi) hit |= nl_mask16(tail_window16(text, n, false, xt)) & ((1u << (hi - xt)) - 1u);
        }
        if (__ballot(hit != 0u) != 0ull && (int)lane == l) flags = (flags & LF_CHROM_NEW) | LF_RECORD | LF_MALFORMED;
    }
}

// statistics: one atomic per WORKGROUP per category.  (One per wave was 4 k atomic adds on one address for a chr1-sized
// block — they retire one every ~12 ns, so the kernel took 66 us where its parse needs 20: round 4, from the kernel trace.)
// The kept lines and the CHROM-run starts of the workgroup are counted the same way and stored, not added: the totals
// k_compact_kept sums for its prefixes.
__device__ __forceinline__ void workgroup_stats(uint32_t flags, uint32_t *s_stat, uint32_t *__restrict__ l_tot, DevCounters *cnt)
{
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x < 6u) s_stat[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t kinds[6] = {LF_RECORD, LF_DROP_REGION, LF_DROP_FILTER, LF_MALFORMED, LF_KEEP, LF_CHROM_NEW};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const unsigned long long b = __ballot(flags & kinds[k]);
        if (lane == 0 && b) atomicAdd(&s_stat[k], (uint32_t)__popcll(b));
    }
    __syncthreads();
    if (threadIdx.x < 4u && s_stat[threadIdx.x]) {
        unsigned long long *dst = threadIdx.x == 0u ? &cnt->n_records : (threadIdx.x == 1u ? &cnt->n_drop_region : (threadIdx.x == 2u ? &cnt->n_drop_filter : &cnt->n_malformed));
        atomicAdd(dst, (unsigned long long)s_stat[threadIdx.x]);
    }
    if (threadIdx.x == 4u) l_tot[blockIdx.x] = s_stat[4];
    if (threadIdx.x == 5u) l_tot[gridDim.x + blockIdx.x] = s_stat[5];
}

__global__ __launch_bounds__(256) void k_parse_fixed(const uint8_t *__restrict__ text, uint64_t n,
                                                     const uint32_t *__restrict__ nl, const uint32_t *__restrict__ d_nlines,
                                                     uint32_t max_lines, const RegionFilter rfv, uint32_t S,
                                                     uint32_t *__restrict__ l_soff, uint32_t *__restrict__ l_lend,
                                                     uint32_t *__restrict__ l_pos, uint32_t *__restrict__ l_refalt,
                                                     uint32_t *__restrict__ l_flags, uint32_t *__restrict__ l_tot,
                                                     uint32_t *__restrict__ l_keep, uint32_t *__restrict__ l_cnew,
                                                     DevCounters *cnt, uint32_t hop_skip)
{
    static_assert(CHAIN_GROUP == 256u, "one k_parse_fixed workgroup is one group of k_compact_kept's prefix");
    HHGT_WAVE_PRIO();
    __shared__ uint32_t stage[256][17];   // (stage_head)
    __shared__ uint32_t s_stat[6];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_found = *d_nlines;
    const uint32_t n_lines = n_found < max_lines ? n_found : max_lines;
    if (i == 0) {
        cnt->n_lines = n_found;
        cnt->err_lines = n_found > max_lines ? (unsigned long long)(n_found - max_lines) : 0ull;
    }
    if (blockIdx.x * blockDim.x >= n_lines) {
        // the grid is sized by max_lines, and so is k_compact_kept's: every workgroup leaves its two totals (l_keep: the scans
        // behind this kernel run over max_lines flags)
        if (threadIdx.x == 0u) l_tot[blockIdx.x] = l_tot[gridDim.x + blockIdx.x] = 0u;
        if (l_keep && i < max_lines) l_keep[i] = l_cnew[i] = 0u;
        return;
    }
    uint32_t s = 0, e = 0;
    bool staged = false;
    if (i < n_lines) {
        s = i ? nl[i - 1] + 1u : 0u;
        e = nl[i];
        staged = stage_head(text, n, s, stage[threadIdx.x]);
    }
    __syncthreads();
    FixedCols r = {0u, 0u, 0u, 0u, 0u, 0u};
    if (i < n_lines) {
        const LineReader rd = {text, reinterpret_cast<const uint8_t *>(stage[threadIdx.x]), s, staged};
        if (e > s && rd(e - 1u) == '\r') --e;  // bgzf_getline strips a trailing CR
        r.soff = e;
        if (e > s && rd(s) != '#') {
            r = parse_record(rd, s, e, S, &rfv);   // (rfv by value in the kernel arguments: no upload, nothing to keep alive on the host)
            if (chrom_run_starts(rd, s, e, i, nl, n, stage)) r.flags |= LF_CHROM_NEW;
        }
    }
    if (hop_skip) examine_dropped(text, n, hop_skip, s, e, r.flags);
    if (i < n_lines) {
        l_soff[i] = r.soff;
        l_lend[i] = e;
        l_pos[i] = r.pos0;
        l_refalt[i] = r.refalt | ((r.gtidx & 0xFFFu) << 16) | (r.stride << 28);   // (12 bits of GT key index: a FORMAT column of 4096 keys is reported, parse_record)
        l_flags[i] = r.flags;
    }
    if (l_keep && i < max_lines) {
        l_keep[i] = (r.flags & LF_KEEP) ? 1u : 0u;
        l_cnew[i] = (r.flags & LF_CHROM_NEW) ? 1u : 0u;
    }
    workgroup_stats(r.flags, s_stat, l_tot, cnt);
}

// one thread per line; kept lines scatter to their compacted slot.  A line's slot is the number of kept lines in front of
// it (kidx) and its CHROM run the number of run starts in front of it (crun): the totals k_parse_fixed left for the
// workgroups in front of this one, summed here by every workgroup for itself, plus a scan of the workgroup's own flags.
// SCANNED (more workgroups than CHAIN_FANIN_MAX): both come from the scan launches in between, l_kidx / l_crun.
template <bool SCANNED>
__global__ __launch_bounds__(CHAIN_GROUP) void k_compact_kept(
    const uint8_t *__restrict__ text, uint64_t n, const uint32_t *__restrict__ nl, const uint32_t *__restrict__ d_nlines,
    uint32_t max_lines, const uint32_t *__restrict__ l_soff,
    const uint32_t *__restrict__ l_lend, const uint32_t *__restrict__ l_pos, const uint32_t *__restrict__ l_refalt,
    const uint32_t *__restrict__ l_flags, const uint32_t *__restrict__ l_tot, const uint32_t *__restrict__ l_kidx,
    const uint32_t *__restrict__ l_crun,
    uint32_t *__restrict__ k_soff, uint32_t *__restrict__ k_lend, uint32_t *__restrict__ k_meta,
    uint32_t *__restrict__ redo_list, uint32_t *__restrict__ redo_flag, uint64_t *__restrict__ run_first, uint8_t *__restrict__ run_names,
    uint32_t max_runs, const uint64_t *__restrict__ d_cursor, uint64_t v_capacity, uint32_t ring, uint32_t *__restrict__ d_start,
    uint32_t *__restrict__ d_stop, uint8_t *__restrict__ d_ref, uint8_t *__restrict__ d_alt, DevCounters *cnt, uint32_t strided)
{
    HHGT_WAVE_PRIO();
    const uint32_t i = blockIdx.x * CHAIN_GROUP + threadIdx.x;
    const uint32_t n_found = *d_nlines;
    const uint32_t n_lines = n_found < max_lines ? n_found : max_lines;
    if (blockIdx.x * CHAIN_GROUP >= n_lines) return;   // (the whole workgroup: the ones that stay scan together)
    const bool live = i < n_lines;
    const uint32_t flags = live ? l_flags[i] : 0u;
    uint32_t kidx, crun;
    if (SCANNED) {
        kidx = live ? l_kidx[i] : 0u;
        crun = live ? l_crun[i] : 0u;
    } else {
        __shared__ uint32_t sm[8];
        uint32_t pre_k = 0, pre_c = 0;
        for (uint32_t g = threadIdx.x; g < blockIdx.x; g += CHAIN_GROUP) {
            pre_k += l_tot[g];
            pre_c += l_tot[gridDim.x + g];
        }
        uint32_t front_k, front_c, own;
        block_excl_scan(pre_k, &front_k, sm);
        block_excl_scan(pre_c, &front_c, sm);
        // both flags in one scan: at most 256 of either, so the halves of a word hold them
        const uint32_t ex = block_excl_scan(((flags & LF_KEEP) ? 1u : 0u) | ((flags & LF_CHROM_NEW) ? 0x10000u : 0u), &own, sm);
        kidx = front_k + (ex & 0xFFFFu);
        crun = front_c + (ex >> 16);
    }
    if (i == n_lines - 1) {
        cnt->n_kept = (unsigned long long)kidx + ((flags & LF_KEEP) ? 1u : 0u);
        cnt->n_chrom_runs = (unsigned long long)crun + ((flags & LF_CHROM_NEW) ? 1u : 0u);
    }
    const uint64_t v_base = *d_cursor;
    if (flags & LF_CHROM_NEW) {
        // run id = number of CHROM_NEW flags before this line; the run's first kept index is the
        // exclusive kept-prefix here; its name is the CHROM field at the start of this line (copied out now: the text
        // buffer may be recycled before the host looks at the runs)
        uint32_t rid = crun;
        if (rid < max_runs) {
            run_first[rid] = kidx;
            const uint32_t s0 = i ? nl[i - 1] + 1u : 0u;
            uint8_t *nm = run_names + (size_t)rid * 32u;
            uint32_t q = 0;
            for (; q < 31u && (uint64_t)s0 + q < n; ++q) {
                const uint8_t ch = text[s0 + q];
                if (ch == '\t' || ch == '\n') break;
                nm[q] = ch;
            }
            for (; q < 32u; ++q) nm[q] = 0;
        }
    }
    // kept lines that are not of the fixed-width shape go on the variable-width kernel's list: one atomic add per WAVE (config
    // 4 has 88 k such lines per pass — one returning add each on one address was most of this kernel's time)
    // (k_meta: bit 2 FAST, bits 8-19 GT key index, bits 20-23 column stride of a GT-first record whose columns are all of one
    // width; with `strided` — the bit-plane encoder runs — such a record is the tile kernel's, not the variable-width kernel's)
    const bool keep = (flags & LF_KEEP) != 0u;
    const bool slow = keep && !(flags & LF_FAST) && !(strided && (l_refalt[live ? i : 0u] >> 28) != 0u);
    const unsigned long long sm = __ballot(slow);
    unsigned long long slot0 = 0ull;
    if (sm != 0ull) {
        const uint32_t lane = threadIdx.x & 63u;
        const int leader = __builtin_ctzll(sm);
        unsigned long long base = 0ull;
        if ((int)lane == leader) base = atomicAdd(&cnt->n_general, (unsigned long long)__popcll(sm));
        base = (unsigned long long)__shfl((long long)base, leader, 64);
        slot0 = base + (unsigned long long)__popcll(sm & ((1ull << lane) - 1ull));
    }
    if (!keep) return;
    const uint32_t k = kidx;
    uint64_t v = v_base + k;
    const uint32_t ra = l_refalt[i];
    k_soff[k] = l_soff[i];
    k_lend[k] = l_lend[i];
    k_meta[k] = (flags & LF_FAST) | ((ra >> 16) << 8);  // bit 2 = FAST, bits 8-19 = GT key index, bits 20-23 = column stride
    redo_flag[k] = 0u;                                  // (the tile kernel's "line already queued for the general path" mark)
    if (slow) redo_list[slot0] = k;
    if (ring) v %= v_capacity;   // ring of chunk columns: the tables wrap with it
    if (v < v_capacity) {
        uint32_t pos0 = l_pos[i];
        if (d_start) d_start[v] = pos0;
        if (d_stop) d_stop[v] = pos0 + 1u;  // vcfpp.h:1124-1127 with |REF| == 1
        if (d_ref) d_ref[v] = (uint8_t)(ra & 0xFFu);
        if (d_alt) d_alt[v] = (uint8_t)((ra >> 8) & 0xFFu);
    }
}

// ---------------------------------------------------------------------------------------------
// min_line: no line of this text can be shorter (0 = unknown).  Long lines: the hopping / walking index reads the text
// behind the bound only (-> the bytes it skips behind every record start; 0: the plain scan).
// mode (hhgt_set_index_mode; < 0: HHGT_INDEX_MODE, default 2): 0 the plain scan, 1 the hop by the bound, 2 the walk.
int index_mode_default()
{
    static const int m = [] {
        if (const char *e = getenv("HHGT_INDEX_MODE")) return atoi(e);
        if (const char *e = getenv("HHGT_INDEX_HOP")) return atoi(e) ? 2 : 0;   // (round 2's switch)
        return 2;
    }();
    return m < 0 ? 0 : (m > 2 ? 2 : m);
}

static int resolved_mode(int mode) { return mode < 0 ? index_mode_default() : mode; }

// (mode: resolved)
static uint32_t index_hop_skip(uint32_t min_line, int mode)
{
    return mode && min_line >= 1536u ? min_line - 16u : 0u;   // margin: the loads start at the 16-byte line in front of the target
}

template <int U, bool WALK>
static void launch_hop(const uint8_t *d_text, uint64_t n, uint32_t *d_slots, uint32_t *d_counts, uint32_t *d_region_tot, uint32_t n_regions,
                       uint32_t skip, uint32_t S, DevCounters *d_cnt, uint32_t K, hipStream_t st)
{
    hipLaunchKernelGGL((k_index_hop<U, WALK>), dim3(((n_regions + K - 1) / K + 3) / 4), dim3(256), 0, st, d_text, n, d_slots, d_counts,
                       d_region_tot, n_regions, skip, S, d_cnt, K);
}

int launch_index_newlines(const uint8_t *d_text, uint64_t n, uint32_t *d_slots, uint32_t *d_counts, uint32_t *d_region_tot,
                          uint32_t n_regions, uint32_t min_line, uint32_t S, int mode, DevCounters *d_cnt, hipStream_t st)
{
    mode = resolved_mode(mode);
    if (const uint32_t skip = index_hop_skip(min_line, mode)) {
        // regions per wave.  Hop, measured on the bench (3 M x 2504, index stage per step): 3.9 ms for 4 .. 7, 4.0-4.1 for 8, 4.3 for 12,
        // 4.4 for 16 and for "as many as make all waves of the launch resident at once" (11 on chr1) — longer walks per wave
        // cost more than a second, part-filled round of waves; fewer than 4 and the plain scan up to a range's first newline
        // (half a line per wave) starts to show
        const bool walk = mode >= 2 && S > 0;
        // The walk costs one dependent 1 KiB load per line, so a wave is a latency chain and every wave pays a plain scan up
        // to the first newline of its range (half a line, in U KiB windows): as few waves as still fill the chip once —
        // 8 workgroups of 4 waves on each of 256 CUs — at least the hop's 6 regions, at most 64 (the per-lane counters).
        const uint32_t k_walk = (n_regions + 8191u) / 8192u;
        uint32_t K = walk ? (k_walk < 6u ? 6u : k_walk) : 6u;
        K = K > 64u ? 64u : K;
        auto *launch = min_line >= 4096u ? (walk ? launch_hop<5, true> : launch_hop<5, false>) : (walk ? launch_hop<3, true> : launch_hop<3, false>);
        launch(d_text, n, d_slots, d_counts, d_region_tot, n_regions, skip, S, d_cnt, K, st);
        HIP_TRY(hipGetLastError());
        return HHGT_OK;
    }
    hipLaunchKernelGGL(k_index_newlines, dim3((n_regions + 3) / 4), dim3(256), 0, st, d_text, n, d_slots,
                       d_counts, d_region_tot, n_regions, d_cnt);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

int launch_compact_newlines(const uint32_t *d_slots, const uint32_t *d_counts, const uint32_t *d_region_tot,
                            uint32_t n_regions, uint32_t *d_nl, uint32_t max_lines, uint32_t *d_nlines, hipStream_t st)
{
    hipLaunchKernelGGL(k_compact_newlines, dim3(chain_groups(n_regions)), dim3(CHAIN_GROUP), 0, st, d_slots, d_counts,
                       d_region_tot, n_regions, d_nl, max_lines, d_nlines);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

int launch_parse_fixed(const uint8_t *d_text, uint64_t n, const uint32_t *d_nl, const uint32_t *d_nlines,
                       uint32_t max_lines, const RegionFilter &region, uint32_t S, const LineCols &l, int mode,
                       DevCounters *d_cnt, hipStream_t st)
{
    if (max_lines == 0) return HHGT_OK;
    mode = resolved_mode(mode);
    // (the skip the hopping index used on this text, 0 for the plain scan: the same rule as launch_index_newlines; the walk
    // may have looked at nothing but the head of a record: a dropped record is examined from end to end)
    uint32_t hop_skip = index_hop_skip(S ? 2u * S + 17u : 0u, mode);
    if (hop_skip && mode >= 2) hop_skip = 0xFFFFFFFFu;
    hipLaunchKernelGGL(k_parse_fixed, dim3(chain_groups(max_lines)), dim3(CHAIN_GROUP), 0, st, d_text, n, d_nl, d_nlines,
                       max_lines, region, S, l.soff, l.lend, l.pos, l.refalt, l.flags, l.tot, l.keep, l.cnew, d_cnt, hop_skip);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}

template <bool SCANNED>
static void launch_kept(const uint8_t *d_text, uint64_t n, const uint32_t *d_nl, const uint32_t *d_nlines, uint32_t max_lines,
                        const LineCols &l, const KeptCols &k, uint32_t max_runs, const uint64_t *d_cursor, uint64_t v_capacity,
                        uint32_t ring, uint32_t *d_start, uint32_t *d_stop, uint8_t *d_ref, uint8_t *d_alt, DevCounters *d_cnt,
                        bool strided, hipStream_t st)
{
    // (the grid of k_parse_fixed: l.tot holds a pair of totals per workgroup of either)
    hipLaunchKernelGGL(k_compact_kept<SCANNED>, dim3(chain_groups(max_lines)), dim3(CHAIN_GROUP), 0, st, d_text, n, d_nl, d_nlines,
                       max_lines, l.soff, l.lend, l.pos, l.refalt, l.flags, l.tot, l.kidx, l.crun, k.soff, k.lend, k.meta,
                       k.redo_list, k.redo_flag, k.run_first, k.run_names, max_runs, d_cursor, v_capacity, ring, d_start, d_stop,
                       d_ref, d_alt, d_cnt, strided ? 1u : 0u);
}

int launch_compact_kept(const uint8_t *d_text, uint64_t n, const uint32_t *d_nl, const uint32_t *d_nlines, uint32_t max_lines,
                        const LineCols &l, const KeptCols &k, uint32_t max_runs, const uint64_t *d_cursor, uint64_t v_capacity,
                        uint32_t ring, uint32_t *d_start, uint32_t *d_stop, uint8_t *d_ref, uint8_t *d_alt, DevCounters *d_cnt,
                        bool strided, hipStream_t st)
{
    if (max_lines == 0) return HHGT_OK;
    auto *launch = chain_scanned(max_lines) ? launch_kept<true> : launch_kept<false>;
    launch(d_text, n, d_nl, d_nlines, max_lines, l, k, max_runs, d_cursor, v_capacity, ring, d_start, d_stop, d_ref, d_alt, d_cnt, strided, st);
    HIP_TRY(hipGetLastError());
    return HHGT_OK;
}
