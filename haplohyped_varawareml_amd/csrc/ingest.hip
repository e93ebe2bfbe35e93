// ingest.hip — the streaming ingest engine (include/hhgt_ingest.h): files / host text -> framed genotype chunks on
// the host.  Host C++ only (threads, streams, events); every computation is one of libhhgt's kernels, reached through
// the same C entry points a caller would use (hhgt_encode_text_async, hhgt_pad_tail_cursor, hhgt_compress_chunks) or,
// for the device-side BGZF inflate issued from the source thread, through launch_inflate directly.
//
// Why it looks the way it does (round 1's Python loop reached 1.6 / 4.3 M variants/s, host / device inflate, against
// 58 M/s for text already in HBM): every text block cost the host a stream synchronisation for the line count, one for
// the kept count, one for the chunk sizes, pageable uploads of the member tables and a Python callback in between.
// Here the GPU's queue never drains: the driver thread queues block k's encode BEFORE it looks at block k-1's result
// record, the compressed sizes of a batch are read by another thread one stage later, and all staging memory is
// pinned and reused.
#include "common.h"
#include "host_owners.h"
#include "../../include/hhgt_ingest.h"
#include "../../include/hhgt_reader.h"
#include <sys/mman.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <thread>

namespace {

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// blocking FIFO; close() wakes everybody, pop() then drains what is left and returns false
template <class T> struct BQ {
    std::mutex m;
    std::condition_variable cv;
    std::deque<T> q;
    bool closed = false;
    void push(T v)
    {
        {
            std::lock_guard<std::mutex> lk(m);
            q.push_back(std::move(v));
        }
        cv.notify_all();
    }
    bool pop(T &out)
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return closed || !q.empty(); });
        if (q.empty()) return false;
        out = std::move(q.front());
        q.pop_front();
        return true;
    }
    void close()
    {
        {
            std::lock_guard<std::mutex> lk(m);
            closed = true;
        }
        cv.notify_all();
    }
    size_t size()
    {
        std::lock_guard<std::mutex> lk(m);
        return q.size();
    }
};

// What the engine holds on the device and in pinned memory.  Each holder's own code is the only place its resource is released,
// and none can be copied (NoCopy, host_owners.h): a slot cannot free what another still uses.  hhgt_ingest_close synchronises
// the streams, then deletes.
struct Event : NoCopy {
    hipEvent_t e = nullptr;
    ~Event() { if (e) hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};
struct Stream : NoCopy {
    hipStream_t s = nullptr;
    ~Stream() { if (s) hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};
struct DevMem : DevBuf, NoCopy {   // common.h's DevBuf has no destructor: the context shares it
    ~DevMem() { release(); }
};
template <class T> struct PinnedRec : NoCopy {   // one pinned record
    T *p = nullptr;
    ~PinnedRec() { if (p) hipHostFree(p); }
    operator T *() const { return p; }
};
struct PinnedBuf : NoCopy {   // grows on demand; pinned allocations are slow, so they only ever grow
    uint8_t *p = nullptr;
    size_t cap = 0;
    ~PinnedBuf() { if (p) hipHostFree(p); }
    int ensure(size_t n)
    {
        if (n <= cap) return HHGT_OK;
        if (p) hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = n + n / 4 + 4096;
        static const bool dbg = getenv("HHGT_ALLOC_DEBUG") != nullptr;
        if (dbg) fprintf(stderr, "[alloc] %.3f ms  hipHostMalloc %zu\n", now_s() * 1e3, want);
        if (hipHostMalloc(reinterpret_cast<void **>(&p), want, hipHostMallocDefault) != hipSuccess) {
            p = nullptr;
            hhgt_set_error("ingest: hipHostMalloc(%zu) failed", want);
            return HHGT_ERR_HIP;
        }
        cap = want;
        return HHGT_OK;
    }
};

struct Input {
    int index = 0;
    int kind = 0;   // 0 file, 1 memory
    std::string path, region;
    const uint8_t *mem = nullptr;
    uint64_t mem_bytes = 0;
    // discovered by the source thread
    std::string header;
    uint64_t S = 0, S_file = 0, header_lines = 0;
    bool dev_inflate = false, is_bgzf = false;
    hhgt_reader *rd = nullptr;   // opened (possibly ahead of time) by the source thread
    // written by the driver / shipper
    hhgt_ingest_stats st;
    double t_first = 0;
    std::string last_run;
    struct InState *state = nullptr;   // encode state of this input (driver thread)
    bool header_sent = false;
    Input() { memset(&st, 0, sizeof(st)); }
};

struct TextBuf : NoCopy {   // device-resident text block
    uint8_t *d = nullptr;   // sized to the byte by open and take_text, so freed here
    size_t cap = 0;
    Event ready, carry_done;
    uint64_t nbytes = 0;
    Input *in = nullptr;
    bool first = false, last = false;
    // device-side inflate: per-member status and the count of failures (checked at harvest)
    DevMem status, bad;
    PinnedRec<unsigned long long> h_bad;
    uint64_t n_members = 0, first_member = 0;
    ~TextBuf() { if (d) hipFree(d); }
};

struct Staging {   // device-inflate: one block's compressed bytes + member tables, host (pinned) and device
    PinnedBuf h;
    DevMem d;
    Event done;   // the inflate that read the device copy has finished
    bool used = false;
};

enum { B_VARIANTS = 2, B_COLUMNS = 3, B_INPUT_END = 4, B_HEADER = 1, B_END = 0 };

struct Batch {
    int kind = 0;
    Input *in = nullptr;
    hipEvent_t ev = nullptr;   // recorded on the main stream behind the batch's device work (one of batch_events)
    // VARIANTS
    int var_slot = -1;
    uint64_t first_variant = 0, n_variants = 0;
    uint32_t n_runs = 0;
    // COLUMNS
    int dst_slot = -1, out_slot = -1;
    uint64_t n_chunks = 0, first_col = 0, n_cols = 0, raw_bytes = 0, framed_bytes = 0;
    Batch(int kind_ = B_END, Input *in_ = nullptr) : kind(kind_), in(in_) {}
};

struct VarSlot {
    PinnedBuf start, ref, alt;
    uint64_t run_first[MAX_CHROM_RUNS];
    char run_names[MAX_CHROM_RUNS][32];
};
struct DstSlot {
    DevMem d, off;          // framed bytes, chunk_off (device)
    PinnedBuf h_off;        // chunk_off (host)
};
struct OutSlot {
    PinnedBuf h;            // framed bytes (host)
    std::vector<uint64_t> off;
};

#define N_TEXT_HOST 4
#define N_TEXT_DEV 4
#define N_RES 4
#define N_VAR 6
#define N_DST 4
#define N_OUT 5
#define N_STG 4   // device-inflate staging slots: one per text buffer, so the source never waits for an inflate two blocks back

// encode state of an input (driver thread only).  The ring holds the matrix as int8 or as bit planes; the four calls at the end
// are the only places that choose between the two kernel families
struct InState {
    hhgt_layout lay;
    DevMem G, P, t_start, t_ref, t_alt, cursor;
    bool planes = false;   // the ring holds the matrix as bit planes (include/hhgt.h "Bit-plane form"); G only backs calls beyond 0 / 1 / missing
    uint64_t ring_cols = 0, col_bytes = 0, n_sc = 0, chunk_nbytes = 0, kept_per_block = 0, done_cols = 0;

    int encode(hhgt_ctx *ctx, const TextBuf &tb, uint32_t max_lines, hhgt_encode_result *rec, hipStream_t s)   // a text block, at the cursor
    {
        const char *region = tb.in->region.c_str();
        uint64_t *cur = cursor.as<uint64_t>();
        uint32_t *start = t_start.as<uint32_t>();
        uint8_t *ref = t_ref.as<uint8_t>(), *alt = t_alt.as<uint8_t>();
        return planes ? hhgt_encode_text_planes_async(ctx, tb.d, tb.nbytes, region, &lay, cur, max_lines, P.p, G.p, start, nullptr, ref, alt, rec, s)
                      : hhgt_encode_text_async(ctx, tb.d, tb.nbytes, region, &lay, cur, max_lines, G.p, start, nullptr, ref, alt, rec, s);
    }
    int compress(hhgt_ctx *ctx, const hhgt_ingest_opts &o, uint64_t slot, uint64_t n, DstSlot &d, hipStream_t s)   // ring slots [slot, slot + n)
    {
        uint64_t *off = d.off.as<uint64_t>();
        return planes ? hhgt_compress_planes(ctx, &lay, P.p, G.p, (uint32_t)slot, (uint32_t)n, o.format, d.d.p, d.d.cap, off, nullptr, s)
                      : hhgt_compress_chunks(ctx, G.as<uint8_t>() + slot * col_bytes, n * n_sc, chunk_nbytes, o.typesize, o.blocksize, o.format,
                                             d.d.p, d.d.cap, off, nullptr, s);
    }
    int pad_samples(hhgt_ctx *ctx, hipStream_t s)   // zero the sample padding rows (S .. round_up(S, sc)) of every ring column
    {
        return planes ? hhgt_pad_tail_planes(ctx, &lay, lay.v_capacity, 0, ring_cols, P.p, s)
                      : hhgt_pad_tail(ctx, &lay, lay.v_capacity, 0, ring_cols, G.p, s);
    }
    int pad_open_column(hhgt_ctx *ctx, hipStream_t s)   // zero the open column behind the cursor
    {
        return planes ? hhgt_pad_tail_planes_cursor(ctx, &lay, cursor.as<uint64_t>(), P.p, s)
                      : hhgt_pad_tail_cursor(ctx, &lay, cursor.as<uint64_t>(), G.p, s);
    }
};

struct Res {   // result slot of an encoded block
    PinnedRec<hhgt_encode_result> rec;
    // the block's whole CHROM run table (MAX_CHROM_RUNS entries; the record holds the first HHGT_RESULT_RUNS): copied out of
    // the context's scratch on the main stream right behind the encode, before the next block's encode overwrites it
    DevMem run_first, run_names;
    Event ev;
    int text_idx = -1;
};

}  // namespace

struct hhgt_ingest {
    hhgt_ctx *ctx = nullptr;
    hhgt_ingest_opts o;
    int device = 0;
    // The streams stand first: every buffer and event below is released before them.
    Stream s_main, s_copy, s_inf, s_out;
    // device inflate: the blocks alternate between s_inf and s_inf2 (one wave per member is latency-bound: the tail round of
    // one block's launch overlaps the next block's), the few bytes behind a block's last newline move on s_carry
    Stream s_inf2, s_carry;
    std::array<hipStream_t, 6> streams() const { return {s_main.s, s_copy.s, s_inf.s, s_inf2.s, s_carry.s, s_out.s}; }
    uint64_t inf_blocks = 0;              // source thread only
    hipEvent_t last_carry = nullptr;      // the latest carry copy queued (an event of some TextBuf), or null
    // inputs
    std::mutex in_mu;
    std::condition_variable in_cv;
    std::deque<std::unique_ptr<Input>> inputs;   // all inputs ever added (stable addresses)
    size_t next_input = 0;                       // source thread's position
    bool finished = false;
    // error state
    std::mutex err_mu;
    int err = 0;
    std::string errmsg;
    std::atomic<bool> failed{false};
    // text buffers
    std::vector<TextBuf> text;
    BQ<int> free_text;
    BQ<int> q_text;          // indices in order; -1 = end of inputs
    // device-inflate staging
    Staging stg[N_STG];
    int stg_next = 0;            // source thread only: the slots go round across inputs
    // member table of the stretch being cut (source thread only).  Raw arrays that only ever grow: a std::vector sized for the
    // worst case (a member per 26 bytes: a million entries for a 25 MB stretch) zero-fills 20 MB per block — 2-5 ms of the
    // source thread per 3 ms of device work (HHGT_INGEST_DEBUG=2: read_done -> scan_done)
    struct MemberTab {
        std::unique_ptr<uint64_t[]> c_off;
        std::unique_ptr<uint32_t[]> c_len, isz, crc;
        size_t cap = 0;
        bool ensure(size_t n)
        {
            if (n <= cap) return true;
            cap = 0;
            const size_t want = n + n / 4;
            c_off.reset(new (std::nothrow) uint64_t[want]);
            c_len.reset(new (std::nothrow) uint32_t[want]);
            isz.reset(new (std::nothrow) uint32_t[want]);
            crc.reset(new (std::nothrow) uint32_t[want]);
            if (!c_off || !c_len || !isz || !crc) return false;
            cap = want;
            return true;
        }
    } mtab;
    DevMem crc_x2n;
    // Two encode states, used alternately: the first blocks of input k+1 are encoded while the last blocks of input k are still
    // being harvested, so the GPU's queue does not drain at a file boundary
    InState ist[2];
    uint64_t n_begun = 0;
    Res res[N_RES];
    // slot pools
    VarSlot var[N_VAR];
    DstSlot dst[N_DST];
    OutSlot out[N_OUT];
    BQ<int> free_var, free_dst, free_out;
    Event batch_events[N_VAR + N_DST + 4];
    BQ<hipEvent_t> free_ev;
    // stages
    BQ<Batch> q_ship, q_out;
    std::thread th_source, th_driver, th_ship;
    // where the threads spend their time (seconds; HHGT_INGEST_DEBUG prints them at the end of each input)
    struct Times {
        double src_wait_text = 0, src_work = 0, drv_wait_text = 0, drv_launch = 0, drv_harvest_wait = 0, drv_harvest = 0,
               drv_begin = 0, ship_wait_ev = 0, ship_copy = 0, ship_wait_out = 0;
    } tm;
    // consumer side: what the previous hhgt_ingest_next handed out
    Batch held;
    bool have_held = false;
    bool ended = false;
};

namespace {

struct TraceRec {
    double t;
    const char *tag;
    long long a, b;
};
std::mutex g_trace_mu;
std::vector<TraceRec> g_trace;
int trace_level()
{
    static const int lv = getenv("HHGT_INGEST_DEBUG") ? atoi(getenv("HHGT_INGEST_DEBUG")) : 0;
    return lv;
}
// events a host thread waits on: the waiter sleeps (hipEventBlockingSync) instead of spinning — the driver spends ~90 % of a
// host-inflated pass inside such a wait and the shipper and the source most of the rest: up to three of the (16 granted) CPUs
// the reader's inflate threads are short of.  HHGT_INGEST_SPIN=1 restores the spinning waits.
unsigned wait_event_flags()
{
    static const bool spin = getenv("HHGT_INGEST_SPIN") && atoi(getenv("HHGT_INGEST_SPIN")) != 0;
    return hipEventDisableTiming | (spin ? 0u : (unsigned)hipEventBlockingSync);
}
void trace(const char *tag, long long a = 0, long long b = 0)
{
    if (trace_level() < 2) return;
    std::lock_guard<std::mutex> lk(g_trace_mu);
    g_trace.push_back({now_s(), tag, a, b});
}

// records the first error and stops every stage.  Always false, so that an error exit reads `return fail(...)`
bool fail(hhgt_ingest *g, int code, const char *msg)
{
    {
        std::lock_guard<std::mutex> lk(g->err_mu);
        if (!g->err) {
            g->err = code ? code : HHGT_ERR_IO;
            g->errmsg = msg ? msg : "ingest failed";
        }
    }
    g->failed.store(true);
    g->free_text.close();
    g->q_text.close();
    g->free_var.close();
    g->free_dst.close();
    g->free_out.close();
    g->free_ev.close();
    g->q_ship.close();
    g->q_out.close();
    g->in_cv.notify_all();
    return false;
}

// error exits.  G_*: in the threads, through fail().  OPEN_*: in the steps of hhgt_ingest_open, which return HHGT_OK or the code of
// what failed, the message in hhgt_last_error
#define G_TRY(expr) do { int _rc = (expr); if (_rc != HHGT_OK) return fail(g, _rc, hhgt_last_error()); } while (0)
#define G_HIP(expr) \
    do { hipError_t _e = (expr); if (_e != hipSuccess) { hhgt_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); return fail(g, HHGT_ERR_HIP, hhgt_last_error()); } } while (0)
#define OPEN_TRY(expr) do { int _rc = (expr); if (_rc != HHGT_OK) return _rc; } while (0)
#define OPEN_HIP(expr, what) \
    do { hipError_t _e = (expr); if (_e != hipSuccess) { hhgt_set_error("ingest: %s failed: %s", what, hipGetErrorString(_e)); return HHGT_ERR_HIP; } } while (0)

// '#' lines at the start of `p`: bytes, line count, number of sample columns.  false: no complete header in [p, p+n)
bool parse_header_text(const uint8_t *p, size_t n, size_t *header_bytes, uint64_t *n_samples, bool at_eof)
{
    size_t pos = 0;
    bool have = false;
    uint64_t S = 0;
    while (pos < n && p[pos] == '#') {
        const void *nl = memchr(p + pos, '\n', n - pos);
        if (!nl && !at_eof) return false;
        const size_t end = nl ? (size_t)((const uint8_t *)nl - p) : n;
        if (end - pos >= 6 && memcmp(p + pos, "#CHROM", 6) == 0) {
            size_t tabs = 0;
            size_t e = end;
            if (e > pos && p[e - 1] == '\r') --e;
            for (size_t i = pos; i < e; ++i) tabs += p[i] == '\t';
            S = tabs >= 9 ? tabs - 8 : 0;
            have = true;
        }
        pos = nl ? end + 1 : n;
    }
    if (pos >= n && !at_eof) return false;   // the header may continue in the next block
    if (!have) return false;
    *header_bytes = pos;
    *n_samples = S;
    return true;
}

bool is_bgzf_file(const char *path)
{
    uint8_t h[18];
    int fd = open(path, O_RDONLY);
    if (fd < 0) return false;
    const ssize_t k = read(fd, h, 18);
    close(fd);
    return k == 18 && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) && h[12] == 'B' && h[13] == 'C';
}

// does this file take the device inflater?  mode 0: never; 1: every BGZF file; 2 ("auto"): a BGZF file whose first member
// inflates to at least twice its size — then the compressed members are the smaller load for the host-device link, and
// the link (not the inflate) is what bounds the host path at cohort widths (text crosses it at 57 GB/s = 5.7 M variants/s
// for 2504 samples; the same files through the device inflater: 11 M/s).  Other files have nothing to gain.
bool wants_device_inflate(int mode, const char *path)
{
    if (mode == 0 || !is_bgzf_file(path)) return false;
    if (mode == 1) return true;
    uint8_t h[18];
    int fd = open(path, O_RDONLY);
    if (fd < 0) return false;
    bool dev = false;
    if (read(fd, h, 18) == 18) {
        const uint32_t bsize = (uint32_t)h[16] + ((uint32_t)h[17] << 8) + 1u;   // whole member
        uint8_t t[4];
        if (bsize >= 26 && pread(fd, t, 4, (off_t)bsize - 4) == 4) {
            const uint32_t isize = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
            dev = isize >= 2u * bsize;
        }
    }
    close(fd);
    return dev;
}

// ---------------------------------------------------------------------------------------------------------------
// source thread
// ---------------------------------------------------------------------------------------------------------------
// What an early return in this section must not leak: Fd and Inflater (host_owners.h), and the reader's block below.
struct ReaderBlock {   // a pinned block of the reader: it goes back to the reader once its copy has left it (`copied`)
    hhgt_reader *rd = nullptr;
    int tok = -1;
    hipEvent_t copied = nullptr;
    void release()
    {
        if (tok < 0) return;
        hipEventSynchronize(copied);
        hhgt_reader_release(rd, tok);
        tok = -1;
    }
    void hold(int t, hipEvent_t ev)   // in place of the block held so far
    {
        release();
        tok = t;
        copied = ev;
    }
    ~ReaderBlock() { release(); }
};

uint64_t block_bytes(const hhgt_ingest *g, uint64_t dflt)
{
    return g->o.block_bytes ? g->o.block_bytes : dflt;
}

bool push_text(hhgt_ingest *g, int ti)
{
    trace("src:push_text", ti, (long long)g->text[(size_t)ti].nbytes);
    g->q_text.push(ti);
    return !g->failed.load();
}

bool take_text(hhgt_ingest *g, int *ti, size_t need)
{
    const double t0 = now_s();
    const bool got = g->free_text.pop(*ti);
    g->tm.src_wait_text += now_s() - t0;
    if (!got) return false;
    TextBuf &tb = g->text[(size_t)*ti];
    if (tb.cap < need) {   // only when a caller's block is larger than the configured size
        if (tb.d) hipFree(tb.d);
        tb.d = nullptr;
        tb.cap = 0;
        G_HIP(hipMalloc(reinterpret_cast<void **>(&tb.d), need + 256));
        tb.cap = need + 256;
    }
    return true;
}

// The one hand-off to the driver.  The work that fills the buffer is queued, tb.ready is recorded behind it; every field of the
// buffer that the driver reads is set here, whatever the buffer's last use left in it.
bool hand_off(hhgt_ingest *g, int ti, Input *in, uint64_t nbytes, bool first, bool last, uint64_t n_members = 0,
              uint64_t first_member = 0)
{
    TextBuf &tb = g->text[(size_t)ti];
    tb.nbytes = nbytes;
    tb.in = in;
    tb.first = first;
    tb.last = last;
    tb.n_members = n_members;
    tb.first_member = first_member;
    return push_text(g, ti);
}

// n bytes of text in host memory -> a text buffer -> the driver.  n = 0: nothing to copy, the (empty) block goes down the pipe
// all the same.  `copied`: an event of the caller's to record behind the copy, or null
bool upload_text(hhgt_ingest *g, Input *in, const void *src, uint64_t n, bool first, bool last, hipEvent_t copied)
{
    int ti;
    if (!take_text(g, &ti, (size_t)n + 64)) return false;
    TextBuf &tb = g->text[(size_t)ti];
    // (a device-inflated input before this one may still have a carry copy out of this buffer queued on its own stream)
    if ((n && g->last_carry && hipStreamWaitEvent(g->s_copy, g->last_carry, 0) != hipSuccess) ||
        (n && hipMemcpyAsync(tb.d, src, n, hipMemcpyHostToDevice, g->s_copy) != hipSuccess) ||
        hipEventRecord(tb.ready, g->s_copy) != hipSuccess || (copied && hipEventRecord(copied, g->s_copy) != hipSuccess))
        return fail(g, HHGT_ERR_HIP, "ingest: upload of a text block failed");
    return hand_off(g, ti, in, n, first, last);
}

bool open_reader(hhgt_ingest *g, Input *in)
{
    if (in->rd || in->kind != 0) return true;
    G_TRY(hhgt_reader_open(in->path.c_str(), block_bytes(g, 64ull << 20), g->o.n_threads, 6, &in->rd));
    in->is_bgzf = hhgt_reader_is_bgzf(in->rd) != 0;
    return true;
}

bool set_header(hhgt_ingest *g, Input *in, const uint8_t *p, size_t n, bool at_eof)
{
    size_t hb = 0;
    uint64_t S = 0;
    if (!parse_header_text(p, n, &hb, &S, at_eof)) {
        hhgt_set_error("%s: no #CHROM header line in the first block of the VCF", in->kind ? "<memory>" : in->path.c_str());
        return fail(g, HHGT_ERR_MALFORMED, hhgt_last_error());
    }
    in->header.assign(reinterpret_cast<const char *>(p), hb);
    in->header_lines = 0;
    for (size_t i = 0; i < hb; ++i) in->header_lines += p[i] == '\n';
    in->S_file = S;
    in->S = g->o.sites_only ? 0 : S;
    in->st.n_samples = in->S;
    return true;
}

// host reader (BGZF / gzip / plain file): pinned ring -> device text buffers
bool feed_from_reader(hhgt_ingest *g, Input *in)
{
    Event cev[2];
    G_HIP(hipEventCreateWithFlags(&cev[0].e, wait_event_flags()));
    G_HIP(hipEventCreateWithFlags(&cev[1].e, wait_event_flags()));
    ReaderBlock prev{in->rd};   // (declared behind the events: it waits on one of them before they are destroyed)
    bool first = true;
    for (int k = 0;; ++k) {
        const void *ptr = nullptr;
        uint64_t n = 0;
        int tok = -1, last = 0;
        const int rc = hhgt_reader_acquire(in->rd, &ptr, &n, &tok, &last);
        if (rc != HHGT_OK) return fail(g, rc, hhgt_last_error());
        if (n == 0 && first) {
            hhgt_set_error("%s: empty file (no VCF header)", in->path.c_str());
            return fail(g, HHGT_ERR_MALFORMED, hhgt_last_error());
        }
        // The reader may end a stream with an EMPTY last block (a gzip stream whose text fills a block exactly before
        // zlib reports the end).  Blocks were already sent without `last`, so an empty one with last = true still has to go
        // down the pipe: the harvest of THAT block pads and frames the open chunk column and sends INPUT_END — without it
        // up to vc - 1 variants' genotypes would silently be missing behind their variant-table rows.
        if (n == 0) return upload_text(g, in, nullptr, 0, false, true, nullptr);
        if (first && !set_header(g, in, static_cast<const uint8_t *>(ptr), (size_t)n, last != 0)) return false;
        if (!upload_text(g, in, ptr, n, first, last != 0, cev[k & 1].e)) return false;
        first = false;
        // the previous pinned block goes back to the reader once its copy has left it
        prev.hold(tok, cev[k & 1].e);
        if (last) return true;
    }
}

bool run_reader_input(hhgt_ingest *g, Input *in)
{
    if (!open_reader(g, in)) return false;
    const bool ok = feed_from_reader(g, in);
    uint64_t fb = 0, tbytes = 0;
    hhgt_reader_stats(in->rd, &fb, &tbytes);
    in->st.file_bytes = fb;
    hhgt_reader_close(in->rd);
    in->rd = nullptr;
    return ok;
}

// text already in host memory: cut at line ends, upload
bool run_memory_input(hhgt_ingest *g, Input *in)
{
    const uint64_t bb = block_bytes(g, 64ull << 20);
    const uint8_t *p = in->mem;
    const uint64_t N = in->mem_bytes;
    if (N == 0) return fail(g, HHGT_ERR_MALFORMED, "<memory>: empty text (no VCF header)");
    if (!set_header(g, in, p, (size_t)(N < bb ? N : bb), N <= bb)) return false;
    in->st.file_bytes = N;
    uint64_t pos = 0;
    while (pos < N) {
        uint64_t n = N - pos < bb ? N - pos : bb;
        const bool last = pos + n >= N;
        if (!last) {
            const void *nl = memrchr(p + pos, '\n', (size_t)n);
            if (!nl) return fail(g, HHGT_ERR_IO, "a line is longer than the text block size");
            n = (uint64_t)((const uint8_t *)nl - (p + pos)) + 1;
        }
        if (!upload_text(g, in, p + pos, n, pos == 0, last, nullptr)) return false;
        pos += n;
    }
    return true;
}

__global__ void k_count_bad_members(const uint32_t *__restrict__ st, uint64_t n, unsigned long long *out)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long m = __ballot(i < n && st[i] != 0u);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(out, (unsigned long long)__popcll(m));
}

bool pread_all(int fd, uint8_t *dst, size_t n, uint64_t off)
{
    size_t got = 0;
    while (got < n) {
        const ssize_t k = pread(fd, dst + got, n - got, (off_t)(off + got));
        if (k <= 0) return false;
        got += (size_t)k;
    }
    return true;
}

// BGZF file inflated on the device: the host walks the member headers and decides the block cuts, the compressed
// members cross PCIe, one wave per member writes the text (csrc/inflate.hip).
// Per block the source thread: pread()s the next stretch of the file straight into a pinned staging slot (no mapping:
// read() copies out of the page cache without faulting a page per 4 KiB), walks the member headers there until the
// block's text budget is used up, inflates the LAST member(s) on the host to learn where the last whole line ends,
// writes the member tables behind the compressed bytes and queues upload + carry copy + inflate kernels.  The first
// blocks of an input are small (the GPU starts after ~1 ms of host work), later ones grow to block_bytes (a launch
// wants >= 10 k members to fill the chip).
// One DeviceInflate per input; a block passes through its steps in the order they stand here (run_device_inflate_input).
struct DeviceInflate {
    hhgt_ingest *g;
    Input *in;
    Fd file;
    Inflater z;
    std::vector<uint8_t> scratch = std::vector<uint8_t>(65536);   // one inflated member
    uint64_t bb = 0, flen = 0;
    uint64_t fpos = 0;          // file offset of the first member not yet in a block
    uint64_t carry = 0;         // bytes of the previous block behind its last newline
    int prev_ti = -1;
    uint64_t prev_cut = 0;
    bool first = true;
    double ratio = 24.0;        // text bytes per file byte, refined as blocks go by
    uint64_t budget = 0, member_index = 0;
    // the block on its way through the steps; each value is set by one step for the steps behind it
    Staging *stg = nullptr;
    uint64_t want = 0, nm64 = 0;               // file bytes read into the staging slot, whole members among them
    size_t nm = 0;                             // members that go into this block
    uint64_t total = 0, consumed = 0, tail = 0;   // their text bytes and file bytes; text behind the block's last newline
    bool last = false;
    int ti = -1;
    size_t comp_bytes = 0, o_coff = 0, o_ooff = 0, o_clen = 0, o_isz = 0, o_crc = 0, stg_bytes = 0;   // staging layout

    bool host_inflate(size_t m, uint8_t *dst)
    {
        return z.member(stg->h.p + g->mtab.c_off[m], g->mtab.c_len[m], dst, g->mtab.isz[m]);
    }
    bool line_too_long() { return fail(g, HHGT_ERR_IO, "a line is longer than the text block: raise block_bytes"); }

    bool open_file()
    {
        bb = block_bytes(g, 512ull << 20);
        file.fd = open(in->path.c_str(), O_RDONLY);
        struct stat st;
        if (file.fd < 0 || fstat(file.fd, &st) != 0) {
            hhgt_set_error("cannot open %s", in->path.c_str());
            return fail(g, HHGT_ERR_IO, hhgt_last_error());
        }
        flen = (uint64_t)st.st_size;
        in->st.file_bytes = flen;
        in->is_bgzf = true;
        trace("src:file_open", (long long)flen);
        // text budget of the first block: small when nothing is in flight (the GPU starts after ~1 ms of host work instead
        // of ~5), full size when earlier inputs still keep the device busy (a small launch fills a fraction of the chip)
        const bool idle = g->free_text.size() == g->text.size() && g->q_text.size() == 0;
        budget = idle ? (bb < (96ull << 20) ? bb : (96ull << 20)) : bb;
        if (flen == 0) return fail(g, HHGT_ERR_MALFORMED, "empty file (no VCF header)");
        return true;
    }

    // the next stretch of the file -> the next staging slot
    bool read_stretch()
    {
        stg = &g->stg[g->stg_next];
        Staging &sg = *stg;
        g->stg_next = (g->stg_next + 1) % N_STG;
        if (sg.used) hipEventSynchronize(sg.done);   // the inflate that read this staging slot two blocks ago
        trace("src:staging_free");
        // stretch of the file to look at: what the budget should need, plus slack; at least one whole member
        want = (uint64_t)((double)budget / ratio * 1.15) + (256u << 10);
        if (want > flen - fpos) want = flen - fpos;
        const size_t tab_room = (size_t)(want / 26 + 2) * 28 + 64;   // tables live behind the compressed bytes (a member is >= 26 bytes)
        if (sg.h.ensure((size_t)want + 64 + tab_room) != HHGT_OK) return fail(g, HHGT_ERR_HIP, hhgt_last_error());
        // one thread copies ~5 GB/s out of the page cache; a 1 GiB text block needs ~40 MB of file
        const size_t piece = 2u << 20;
        const int nth = want > 4 * piece ? 4 : 1;
        std::atomic<size_t> next{0};
        std::atomic<bool> rd_ok{true};
        auto work = [&] {
            for (;;) {
                const size_t o = next.fetch_add(piece);
                if (o >= want) break;
                const size_t n = want - o < piece ? (size_t)(want - o) : piece;
                if (!pread_all(file.fd, sg.h.p + o, n, fpos + o)) rd_ok.store(false);
            }
        };
        std::vector<std::thread> th;
        for (int i = 1; i < nth; ++i) th.emplace_back(work);
        work();
        for (auto &t : th) t.join();
        if (!rd_ok.load()) return fail(g, HHGT_ERR_IO, "read failed");
        trace("src:read_done", (long long)want);
        return true;
    }

    // member table of the stretch, cut at the text budget
    bool scan_and_cut()
    {
        const size_t max_m = (size_t)(want / 26 + 2);
        if (!g->mtab.ensure(max_m)) return fail(g, HHGT_ERR_IO, "ingest: out of memory for the BGZF member table");
        uint64_t *c_off = g->mtab.c_off.get();
        uint32_t *c_len = g->mtab.c_len.get(), *isz = g->mtab.isz.get();
        uint64_t used = 0;
        const int rc = hhgt_bgzf_scan(stg->h.p, want, max_m, c_off, c_len, isz, g->mtab.crc.get(), &nm64, &used);
        if (rc != HHGT_OK) return fail(g, rc, hhgt_last_error());
        if (nm64 == 0) {
            if (want == flen - fpos) return fail(g, HHGT_ERR_MALFORMED, "bytes behind the last whole BGZF member");
            return fail(g, HHGT_ERR_IO, "a BGZF member larger than the staging stretch");
        }
        nm = 0;
        total = consumed = 0;
        while (nm < nm64 && carry + total + isz[nm] <= budget) {
            total += isz[nm];
            consumed = c_off[nm] + c_len[nm] + 8;   // payload + CRC32 + ISIZE
            ++nm;
        }
        if (nm == 0) return line_too_long();
        last = fpos + consumed >= flen;
        trace("src:scan_done", (long long)nm);
        return true;
    }

    // header (first block only): leading members inflated on the host until the '#' lines are complete
    bool read_header()
    {
        std::vector<uint8_t> head;
        bool have = false;
        for (size_t m = 0; m < nm64 && head.size() < (256u << 20); ++m) {
            const size_t at = head.size(), isz = g->mtab.isz[m];
            head.resize(at + isz);
            if (isz && !host_inflate(m, head.data() + at)) return fail(g, HHGT_ERR_IO, "inflate failed (header members)");
            size_t hb;
            uint64_t S;
            const bool eof = fpos + g->mtab.c_off[m] + g->mtab.c_len[m] + 8 >= flen;
            if (parse_header_text(head.data(), head.size(), &hb, &S, eof)) {
                have = set_header(g, in, head.data(), head.size(), eof);
                break;
            }
        }
        if (!have) {
            if (g->failed.load()) return false;
            hhgt_set_error("%s: no #CHROM header line", in->path.c_str());
            return fail(g, HHGT_ERR_MALFORMED, hhgt_last_error());
        }
        trace("src:header_done");
        return true;
    }

    // bytes behind the last newline move to the next block: the last member(s) are inflated here to find it
    bool find_tail()
    {
        tail = 0;
        if (last) return true;
        for (size_t m = nm; m > 0; --m) {
            const uint32_t isz = g->mtab.isz[m - 1];
            if (isz == 0) continue;
            if (!host_inflate(m - 1, scratch.data())) return fail(g, HHGT_ERR_IO, "inflate failed (block tail)");
            const void *nl = memrchr(scratch.data(), '\n', isz);
            if (nl) {
                tail += isz - ((uint64_t)((const uint8_t *)nl - scratch.data()) + 1);
                return true;
            }
            tail += isz;
        }
        return line_too_long();
    }

    // a text buffer for the block, and the staging slot laid out:
    // [compressed bytes | comp_off u64 | out_off u64 | comp_len u32 | isize u32 | crc u32]
    bool lay_out_staging()
    {
        if (!take_text(g, &ti, (size_t)(carry + total) + 64)) return false;
        TextBuf &tb = g->text[(size_t)ti];
        Staging &sg = *stg;
        trace("src:took_text", (long long)ti);
        comp_bytes = ((size_t)consumed + 3) / 4 * 4 + 4;
        o_coff = (comp_bytes + 7) & ~(size_t)7;
        o_ooff = o_coff + nm * 8;
        o_clen = o_ooff + nm * 8;
        o_isz = o_clen + nm * 4;
        o_crc = o_isz + nm * 4;
        stg_bytes = o_crc + nm * 4;
        if (stg_bytes > sg.h.cap) return fail(g, HHGT_ERR_IO, "ingest: staging slot too small for the member tables");
        if (sg.d.ensure(stg_bytes) != HHGT_OK || tb.status.ensure(nm * 4) != HHGT_OK || tb.bad.ensure(8) != HHGT_OK)
            return fail(g, HHGT_ERR_HIP, hhgt_last_error());
        memset(sg.h.p + consumed, 0, comp_bytes - (size_t)consumed);   // the kernel reads whole dwords
        uint64_t *hc = reinterpret_cast<uint64_t *>(sg.h.p + o_coff), *ho = reinterpret_cast<uint64_t *>(sg.h.p + o_ooff);
        uint32_t *hl = reinterpret_cast<uint32_t *>(sg.h.p + o_clen), *hz = reinterpret_cast<uint32_t *>(sg.h.p + o_isz),
                 *hr = reinterpret_cast<uint32_t *>(sg.h.p + o_crc);
        uint64_t oo = carry;
        for (size_t i = 0; i < nm; ++i) {
            hc[i] = g->mtab.c_off[i];
            ho[i] = oo;
            hl[i] = g->mtab.c_len[i];
            hz[i] = g->mtab.isz[i];
            hr[i] = g->mtab.crc[i];
            oo += g->mtab.isz[i];
        }
        return true;
    }

    // the block's device work, on the streams it belongs to: nothing but the order of HIP calls lives here
    bool queue_device_work()
    {
        Staging &sg = *stg;
        TextBuf &tb = g->text[(size_t)ti];
        uint8_t *dd = sg.d.as<uint8_t>();
        hipStream_t si = (g->inf_blocks++ & 1) ? g->s_inf2 : g->s_inf;
        hipError_t e = hipMemcpyAsync(dd, sg.h.p, stg_bytes, hipMemcpyHostToDevice, si);
        // this block may write a text buffer an earlier carry copy still reads from (they run on their own stream)
        if (e == hipSuccess && g->last_carry) e = hipStreamWaitEvent(si, g->last_carry, 0);
        if (e == hipSuccess && carry) {
            TextBuf &pb = g->text[(size_t)prev_ti];
            e = hipStreamWaitEvent(g->s_carry, pb.ready, 0);   // the previous block's text is complete
            if (e == hipSuccess) e = hipMemcpyAsync(tb.d, pb.d + prev_cut, carry, hipMemcpyDeviceToDevice, g->s_carry);
            if (e == hipSuccess) e = hipEventRecord(tb.carry_done, g->s_carry);
            g->last_carry = tb.carry_done;
            // free_text is a FIFO of four, so a block never lands in the buffer of the one before it; if it ever does, the
            // copy has to read the tail before the inflate overwrites it
            if (e == hipSuccess && ti == prev_ti) e = hipStreamWaitEvent(si, tb.carry_done, 0);
        }
        if (e == hipSuccess) e = hipMemsetAsync(tb.bad.p, 0, 8, si);
        if (e != hipSuccess) return fail(g, HHGT_ERR_HIP, "ingest: upload of compressed members failed");
        G_TRY(launch_inflate(dd, comp_bytes, reinterpret_cast<const uint64_t *>(dd + o_coff),
                             reinterpret_cast<const uint32_t *>(dd + o_clen), reinterpret_cast<const uint64_t *>(dd + o_ooff),
                             reinterpret_cast<const uint32_t *>(dd + o_isz), nm, tb.d, tb.cap, tb.status.as<uint32_t>(),
                             reinterpret_cast<const uint32_t *>(dd + o_crc), g->crc_x2n.as<uint32_t>(), si));
        hipLaunchKernelGGL(k_count_bad_members, dim3((uint32_t)((nm + 255) / 256)), dim3(256), 0, si, tb.status.as<uint32_t>(),
                           (uint64_t)nm, tb.bad.as<unsigned long long>());
        *tb.h_bad = 0;
        e = hipMemcpyAsync(tb.h_bad, tb.bad.p, 8, hipMemcpyDeviceToHost, si);
        if (e == hipSuccess && carry) e = hipStreamWaitEvent(si, tb.carry_done, 0);
        if (e == hipSuccess) e = hipEventRecord(tb.ready, si);
        if (e == hipSuccess) e = hipEventRecord(sg.done, si);
        if (e != hipSuccess) return fail(g, HHGT_ERR_HIP, "ingest: device inflate launch failed");
        sg.used = true;
        return true;
    }

    // the block goes to the driver; where the next one starts, and how much text it may hold
    bool hand_off_and_advance()
    {
        prev_cut = carry + total - tail;
        if (!hand_off(g, ti, in, prev_cut, first, last, nm, member_index)) return false;
        member_index += nm;
        first = false;
        prev_ti = ti;
        carry = tail;
        fpos += consumed;
        if (total && consumed) ratio = 0.5 * ratio + 0.5 * ((double)total / (double)consumed);
        budget = budget * 4 < bb ? budget * 4 : bb;
        return true;
    }
};

bool run_device_inflate_input(hhgt_ingest *g, Input *in)
{
    DeviceInflate d{g, in};
    if (!d.open_file()) return false;
    while (d.fpos < d.flen) {
        if (!d.read_stretch()) return false;
        if (!d.scan_and_cut()) return false;
        if (d.first && !d.read_header()) return false;
        if (!d.find_tail()) return false;
        if (!d.lay_out_staging()) return false;
        if (!d.queue_device_work()) return false;
        if (!d.hand_off_and_advance()) return false;
    }
    return true;
}

void source_main(hhgt_ingest *g)
{
    hipSetDevice(g->device);
    for (;;) {
        Input *in = nullptr;
        {
            std::unique_lock<std::mutex> lk(g->in_mu);
            g->in_cv.wait(lk, [&] { return g->failed.load() || g->finished || g->next_input < g->inputs.size(); });
            if (g->failed.load()) break;
            if (g->next_input >= g->inputs.size()) break;   // finished and drained
            in = g->inputs[g->next_input++].get();
        }
        if (in->kind == 0) in->dev_inflate = wants_device_inflate(g->o.device_inflate, in->path.c_str());
        in->st.device_inflate = in->dev_inflate ? 1 : 0;
        // open the readers of the next file inputs now: their inflate runs while this input is uploaded and encoded
        if (!in->dev_inflate) {
            std::vector<Input *> ahead;
            {
                std::lock_guard<std::mutex> lk(g->in_mu);
                const int A = g->o.files_ahead > 0 ? g->o.files_ahead : 1;
                for (size_t i = g->next_input; i < g->inputs.size() && (int)ahead.size() < A; ++i)
                    if (g->inputs[i]->kind == 0 && !g->inputs[i]->rd) ahead.push_back(g->inputs[i].get());
            }
            for (Input *a : ahead)
                if (!wants_device_inflate(g->o.device_inflate, a->path.c_str()) && !open_reader(g, a)) break;
        }
        bool ok = in->kind == 1 ? run_memory_input(g, in) : (in->dev_inflate ? run_device_inflate_input(g, in) : run_reader_input(g, in));
        in->st.is_bgzf = in->is_bgzf ? 1 : 0;
        if (!ok || g->failed.load()) break;
    }
    // readers opened ahead but never run (error paths)
    {
        std::lock_guard<std::mutex> lk(g->in_mu);
        for (auto &in : g->inputs)
            if (in->rd) {
                hhgt_reader_close(in->rd);
                in->rd = nullptr;
            }
    }
    g->q_text.push(-1);
}

// ---------------------------------------------------------------------------------------------------------------
// driver thread
// ---------------------------------------------------------------------------------------------------------------
// The batch slots for blocks that keep up to `kept` records.  They may still be in use by batches of the previous input that
// are on their way out, so when one has to grow (this input has more samples, or is the first) every slot is collected first —
// the shipper and the consumer give them back as they go; at open all of them sit in their pools — and returned afterwards.
static bool grow_batch_slots(hhgt_ingest *g, size_t need_d, size_t need_off, size_t kept)
{
    const size_t need_start = kept * 4 + 16, need_base = kept + 4;   // k_tables_to_host writes whole groups of four
    bool grow = false;
    for (auto &d : g->dst) grow = grow || d.d.cap < need_d || d.off.cap < need_off || d.h_off.cap < need_off;
    for (auto &v : g->var) grow = grow || v.start.cap < need_start || v.ref.cap < need_base;
    if (grow) {
        int tmp;
        for (int i = 0; i < N_DST; ++i)
            if (!g->free_dst.pop(tmp)) return false;
        for (int i = 0; i < N_VAR; ++i)
            if (!g->free_var.pop(tmp)) return false;
        for (auto &d : g->dst) {
            G_TRY(d.d.ensure(need_d));
            G_TRY(d.off.ensure(need_off));
            G_TRY(d.h_off.ensure(need_off));
        }
        for (auto &v : g->var) {
            G_TRY(v.start.ensure(need_start));
            G_TRY(v.ref.ensure(need_base));
            G_TRY(v.alt.ensure(need_base));
        }
        for (int i = 0; i < N_DST; ++i) g->free_dst.push(i);
        for (int i = 0; i < N_VAR; ++i) g->free_var.push(i);
    }
    return true;
}

// geometry of an input's ring + every buffer whose size follows from the sample count: the state's own (ring of chunk columns
// as planes / int8, variant tables, cursor) and the batch slots.  at_open: called from hhgt_ingest_open with the caller's
// expect_samples, so that the first input finds its buffers made (and pinned) — the shipper's pinned copies among them.
static bool size_input_state(hhgt_ingest *g, InState *X, uint64_t S, uint64_t S_file, uint64_t block_bytes, bool at_open)
{
    const int32_t sc = g->o.sc, vc = g->o.vc;
    // a kept line holds S sample columns of at least two bytes behind nine fixed columns
    // (file inputs: the reader never hands out blocks below 1 MiB and grows a text buffer to what a block needs)
    if (block_bytes < (1ull << 20)) block_bytes = 1ull << 20;
    X->kept_per_block = block_bytes / (2 * S_file + 16) + 2;
    const uint64_t W = X->kept_per_block / (uint64_t)vc + 2;   // chunk columns one block can touch
    X->ring_cols = 2 * W + 6;
    X->lay = hhgt_layout{(int32_t)S, sc, vc, (int32_t)X->ring_cols, X->ring_cols * (uint64_t)vc};   // a ring of ring_cols chunk columns
    X->n_sc = S ? (S + (uint64_t)sc - 1) / (uint64_t)sc : 0;
    X->chunk_nbytes = (uint64_t)sc * (uint64_t)vc * 2;
    X->col_bytes = X->n_sc * X->chunk_nbytes;
    const uint64_t gbytes = hhgt_layout_bytes(&X->lay);
    G_TRY(X->G.ensure((size_t)(gbytes ? gbytes : 16)));
    // the compressor is this engine's only consumer of the matrix: where the chunk geometry allows (typesize 2, 8 KiB Blosc
    // blocks, whole blocks per chunk row) the encoder hands it over as bit planes — a quarter of the bytes each way
    static const bool planes_env = !(getenv("HHGT_INGEST_PLANES") && atoi(getenv("HHGT_INGEST_PLANES")) == 0);
    X->planes = planes_env && S > 0 && g->o.typesize == 2 && g->o.blocksize == 8192 && vc % 4096 == 0 && hhgt_planes_bytes(&X->lay) != 0;
    if (X->planes) G_TRY(X->P.ensure((size_t)hhgt_planes_bytes(&X->lay)));
    G_TRY(X->t_start.ensure((size_t)X->lay.v_capacity * 4));
    G_TRY(X->t_ref.ensure((size_t)X->lay.v_capacity));
    G_TRY(X->t_alt.ensure((size_t)X->lay.v_capacity));
    G_TRY(X->cursor.ensure(8));
    const uint64_t max_cols = W + 2;
    const size_t need_d = (size_t)(max_cols * X->n_sc * (X->chunk_nbytes + 32) + 64), need_off = (size_t)((max_cols * X->n_sc + 1) * 8);
    if (!grow_batch_slots(g, need_d, need_off, (size_t)X->kept_per_block)) return false;
    if (at_open) {
        // the shipper's pinned copies of the framed chunks: a batch is at most need_d bytes and about a fifth of that on
        // genotype planes — a slot that turns out too small still grows where it is used
        for (auto &o : g->out) G_TRY(o.h.ensure(need_d / 4 + 4096));
    }
    return true;
}

bool begin_input(hhgt_ingest *g, Input *in, uint64_t block_bytes)
{
    InState *X = &g->ist[g->n_begun++ & 1u];
    in->state = X;
    if (!size_input_state(g, X, in->S, in->S_file, block_bytes, false)) return false;
    // sample padding rows (S .. round_up(S, sc)) are never written by the encoder: zeroed once per input for every
    // ring column (everything else of a column is overwritten, or zeroed by the tail padding, before it is framed)
    if (hhgt_layout_bytes(&X->lay) && in->S % (uint64_t)g->o.sc) G_TRY(X->pad_samples(g->ctx, g->s_main));
    G_HIP(hipMemsetAsync(X->cursor.p, 0, 8, g->s_main));
    X->done_cols = 0;
    in->t_first = now_s();
    return true;
}

// rows [a, a + n) of the three variant tables (rings of `cap` entries) -> pinned host memory, written by the kernel itself over
// the link.  One launch instead of three to six hipMemcpyAsync calls — and the runtime's copy path is kept out of the driver
// thread: HHGT_INGEST_DEBUG=2 showed the first such copy above ~200 KB blocking the calling thread for as long as the encode
// queued behind it on the stream ran (7 ms of a 60 ms first pass).  Thread i moves variants 4i .. 4i+3.
__global__ void __launch_bounds__(256) k_tables_to_host(const uint32_t *__restrict__ t_start, const uint8_t *__restrict__ t_ref,
                                                        const uint8_t *__restrict__ t_alt, uint64_t a, uint64_t n, uint64_t cap,
                                                        uint32_t *__restrict__ h_start, uint32_t *__restrict__ h_ref,
                                                        uint32_t *__restrict__ h_alt)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x, v0 = i * 4;
    if (v0 >= n) return;
    uint32_t st[4] = {0, 0, 0, 0}, r = 0, al = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (v0 + k < n) {
            const uint64_t s = (a + v0 + k) % cap;
            st[k] = t_start[s];
            r |= (uint32_t)t_ref[s] << (8 * k);
            al |= (uint32_t)t_alt[s] << (8 * k);
        }
    *reinterpret_cast<uint4 *>(h_start + v0) = make_uint4(st[0], st[1], st[2], st[3]);   // slots hold kept_per_block + 4 entries
    h_ref[i] = r;
    h_alt[i] = al;
}

// completed columns [c0, c1) -> compress batches (one per contiguous run of ring slots)
bool queue_columns(hhgt_ingest *g, Input *in, uint64_t c0, uint64_t c1)
{
    InState *X = in->state;
    while (c0 < c1) {
        const uint64_t slot = c0 % X->ring_cols;
        const uint64_t n = (c1 - c0) < (X->ring_cols - slot) ? (c1 - c0) : (X->ring_cols - slot);
        Batch b(B_COLUMNS, in);
        b.first_col = c0;
        b.n_cols = n;
        b.n_chunks = n * X->n_sc;
        b.raw_bytes = n * X->col_bytes;
        if (!g->free_dst.pop(b.dst_slot) || !g->free_ev.pop(b.ev)) return false;
        trace("drv:dst_slot", (long long)n);
        DstSlot &d = g->dst[(size_t)b.dst_slot];
        G_TRY(X->compress(g->ctx, g->o, slot, n, d, g->s_main));
        trace("drv:compress_queued", (long long)b.n_chunks);
        G_HIP(hipMemcpyAsync(d.h_off.p, d.off.p, (size_t)((b.n_chunks + 1) * 8), hipMemcpyDeviceToHost, g->s_main));
        G_HIP(hipEventRecord(b.ev, g->s_main));
        trace("drv:off_copy_queued");
        g->q_ship.push(b);
        c0 += n;
    }
    return true;
}

// The result record of an encoded block, once its event has been waited for: one Harvest per block, its steps in the order of run()
struct Harvest {
    hhgt_ingest *g;
    Res &r;
    TextBuf &tb = g->text[(size_t)r.text_idx];
    Input *in = tb.in;
    InState *X = in->state;
    const bool last = tb.last;
    const hhgt_encode_result rec = *r.rec;
    const uint64_t a = rec.cursor_before, b = rec.cursor_after;   // the input's kept records before and behind the block

    bool report_failed_block()
    {
        if (in->dev_inflate && *tb.h_bad) return report_failed_inflate();   // (the text behind it means nothing)
        if (rec.n_lines_over && !rec.err_density) {
            hhgt_set_error("Error parsing VCF file: %llu more lines than records of %llu samples fit in the block (blank or cut-off lines)",
                           (unsigned long long)rec.n_lines_over, (unsigned long long)in->S_file);
            return fail(g, HHGT_ERR_MALFORMED, hhgt_last_error());
        }
        G_TRY(hhgt_encode_result_status(&rec));   // (more than MAX_CHROM_RUNS runs: HHGT_ERR_CAPACITY)
        return true;
    }
    bool report_failed_inflate()
    {
        // which member, and why: only now is the per-member status worth copying
        std::vector<uint32_t> st((size_t)tb.n_members);
        hipMemcpy(st.data(), tb.status.p, st.size() * 4, hipMemcpyDeviceToHost);
        size_t k = 0;
        while (k < st.size() && !st[k]) ++k;
        const uint32_t code = k < st.size() ? st[k] : 0;
        if (code == 9) hhgt_set_error("BGZF member %llu: CRC-32 of the inflated text differs from the trailer", (unsigned long long)(tb.first_member + k));
        else hhgt_set_error("BGZF member %llu: DEFLATE stream is corrupt (status %u)", (unsigned long long)(tb.first_member + k), code);
        return fail(g, HHGT_ERR_IO, hhgt_last_error());
    }
    // the block's counts; its text has then been consumed and goes back to the source: nothing behind this step reads `tb`
    bool tally_stats_and_release_text()
    {
        in->st.n_lines += rec.stats.n_lines;
        in->st.n_records += rec.stats.n_records;
        in->st.n_drop_region += rec.stats.n_drop_region;
        in->st.n_drop_filter += rec.stats.n_drop_filter;
        in->st.n_haploid_padded += rec.stats.n_haploid_padded;
        in->st.n_general_lines += rec.stats.n_general_lines;
        in->st.text_bytes += tb.nbytes;
        in->st.n_blocks += 1;
        if (b - a > X->kept_per_block) {   // the ring and the variant slots were sized from this bound: never trust it silently
            hhgt_set_error("ingest: a text block kept %llu records, the engine's buffers were sized for %llu (block of %llu bytes)",
                           (unsigned long long)(b - a), (unsigned long long)X->kept_per_block, (unsigned long long)tb.nbytes);
            return fail(g, HHGT_ERR_CAPACITY, hhgt_last_error());
        }
        g->free_text.push(r.text_idx);   // the text has been consumed: the source may overwrite the buffer
        r.text_idx = -1;
        in->st.n_kept = b;
        return true;
    }
    // the block's rows of the variant tables and its CHROM runs, fetched here where the record is too small for them
    bool queue_variants()
    {
        const uint32_t n_runs = (uint32_t)rec.stats.n_chrom_runs;
        if (b == a && !n_runs) return true;
        const uint64_t *run_first = rec.run_first;
        const char *run_names = &rec.run_names[0][0];
        std::vector<uint64_t> more_first;
        std::vector<char> more_names;
        if (n_runs > HHGT_RESULT_RUNS) {
            // every empty or header line and every CHROM change inside the block starts a run (the ones with no kept record
            // included): the rest of the table is in the copy queued behind the block's encode
            more_first.resize(n_runs);
            more_names.resize((size_t)n_runs * 32);
            G_HIP(hipMemcpy(more_first.data(), r.run_first.p, (size_t)n_runs * 8, hipMemcpyDeviceToHost));
            G_HIP(hipMemcpy(more_names.data(), r.run_names.p, (size_t)n_runs * 32, hipMemcpyDeviceToHost));
            run_first = more_first.data();
            run_names = more_names.data();
        }
        Batch v(B_VARIANTS, in);
        v.first_variant = a;
        v.n_variants = b - a;
        if (!g->free_var.pop(v.var_slot) || !g->free_ev.pop(v.ev)) return false;
        trace("drv:var_slot");
        VarSlot &vs = g->var[(size_t)v.var_slot];
        if (b > a) {
            const uint64_t nt = (b - a + 3) / 4;
            hipLaunchKernelGGL(k_tables_to_host, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, g->s_main, X->t_start.as<uint32_t>(),
                               X->t_ref.as<uint8_t>(), X->t_alt.as<uint8_t>(), a, b - a, X->lay.v_capacity, reinterpret_cast<uint32_t *>(vs.start.p),
                               reinterpret_cast<uint32_t *>(vs.ref.p), reinterpret_cast<uint32_t *>(vs.alt.p));
            G_HIP(hipGetLastError());
        }
        trace("drv:tables_queued", (long long)(b - a));
        for (uint32_t i = 0; i < n_runs; ++i) {
            const char *nm = run_names + (size_t)i * 32;
            const std::string name(nm, strnlen(nm, 31));
            if (name == in->last_run) continue;   // the block continues the previous block's (or this block's last) contig
            in->last_run = name;
            vs.run_first[v.n_runs] = a + run_first[i];
            memset(vs.run_names[v.n_runs], 0, 32);
            memcpy(vs.run_names[v.n_runs], name.data(), name.size());
            ++v.n_runs;
        }
        G_HIP(hipEventRecord(v.ev, g->s_main));
        g->q_ship.push(v);
        trace("drv:var_queued");
        return true;
    }
    bool queue_finished_columns()
    {
        if (!in->S) return true;
        const uint64_t vc = (uint64_t)g->o.vc, done = b / vc;
        if (done > X->done_cols) {
            if (!queue_columns(g, in, X->done_cols, done)) return false;
            X->done_cols = done;
        }
        if (last && b % vc) {
            // the open column: zero behind the cursor, frame it
            G_TRY(X->pad_open_column(g->ctx, g->s_main));
            if (!queue_columns(g, in, X->done_cols, X->done_cols + 1)) return false;
            X->done_cols += 1;
        }
        return true;
    }
    bool run()
    {
        if (!in->header_sent) g->q_ship.push(Batch(B_HEADER, in));   // by the input's first harvest: behind the previous input's last events
        in->header_sent = true;
        if (!report_failed_block() || !tally_stats_and_release_text() || !queue_variants() || !queue_finished_columns()) return false;
        if (last) g->q_ship.push(Batch(B_INPUT_END, in));            // end of input
        return true;
    }
};

// Bound on a block's line count (sizes the workspaces and every grid behind the index): a record of a file with S sample
// columns has at least 2 S + 17 bytes (a sites-only file's eight columns: 16), so apart from the header lines of the first
// block more lines than that can only be blank or cut-off lines — which are a parse error anyway (reported as such by
// harvest).  The unconditional bound, 1024 lines per 16 KiB region, would size the grids for lines of 16 bytes: 10 M empty
// workgroups per 1 GiB block.
uint32_t max_lines_of(const TextBuf &tb)
{
    const uint64_t n_regions = (tb.nbytes + 1 + INDEX_REGION - 1) / INDEX_REGION;
    const uint64_t min_record = tb.in->S_file ? 2 * (uint64_t)tb.in->S_file + 17 : 16;
    uint64_t max_lines = tb.nbytes / min_record + (tb.first ? tb.in->header_lines : 0) + 64;
    if (max_lines > n_regions * INDEX_CAP) max_lines = n_regions * INDEX_CAP;
    return (uint32_t)(max_lines > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : max_lines);
}

// One Driver per engine: block() takes the text blocks in order; a block's result is looked at one block later.
struct Driver {
    hhgt_ingest *g;
    std::deque<int> pending;   // result slots in flight, oldest first
    int next_res = 0;

    bool harvest_oldest()
    {
        Res &r = g->res[pending.front()];
        const double t0 = now_s();
        G_HIP(hipEventSynchronize(r.ev));
        const double t1 = now_s();
        trace("drv:encode_done", r.text_idx);
        const bool ok = Harvest{g, r}.run();
        trace("drv:harvested");
        g->tm.drv_harvest_wait += t1 - t0;
        g->tm.drv_harvest += now_s() - t1;
        if (ok) pending.pop_front();
        return ok;
    }
    bool block(int ti)
    {
        TextBuf &tb = g->text[(size_t)ti];
        const double tb0 = now_s();
        if (tb.first && !begin_input(g, tb.in, tb.cap)) return false;
        g->tm.drv_begin += now_s() - tb0;
        if ((int)pending.size() >= N_RES - 1 && !harvest_oldest()) return false;
        Res &r = g->res[next_res];
        const double tl0 = now_s();
        trace("drv:encode_launch", ti, (long long)tb.nbytes);
        G_HIP(hipStreamWaitEvent(g->s_main, tb.ready, 0));
        G_TRY(tb.in->state->encode(g->ctx, tb, max_lines_of(tb), r.rec, g->s_main));
        G_HIP(hipMemcpyAsync(r.run_first.p, g->ctx->enc.run_first.p, MAX_CHROM_RUNS * 8, hipMemcpyDeviceToDevice, g->s_main));
        G_HIP(hipMemcpyAsync(r.run_names.p, g->ctx->enc.run_names.p, MAX_CHROM_RUNS * 32, hipMemcpyDeviceToDevice, g->s_main));
        G_HIP(hipEventRecord(r.ev, g->s_main));
        r.text_idx = ti;
        pending.push_back(next_res);
        next_res = (next_res + 1) % N_RES;
        g->tm.drv_launch += now_s() - tl0;
        // one block behind: the GPU has the encode above queued while the host looks at the previous result.  The
        // last block of an input is only drained at once when nothing else is waiting to be queued.
        while (pending.size() > 1 || (tb.last && !pending.empty() && g->q_text.size() == 0))
            if (!harvest_oldest()) return false;
        return true;
    }
};

void driver_main(hhgt_ingest *g)
{
    hipSetDevice(g->device);
    Driver drv{g};
    for (;;) {
        int ti;
        const double tw = now_s();
        const bool got = g->q_text.pop(ti);
        g->tm.drv_wait_text += now_s() - tw;
        if (!got || ti < 0) break;   // stopped, or the end of inputs
        if (!drv.block(ti)) break;
    }
    while (!g->failed.load() && !drv.pending.empty())
        if (!drv.harvest_oldest()) break;
    if (!g->failed.load()) g->q_ship.push(Batch(B_END, nullptr));
}

// ---------------------------------------------------------------------------------------------------------------
// shipper thread: sizes -> device-to-host copy of the framed bytes -> out queue
// ---------------------------------------------------------------------------------------------------------------
bool wait_batch(hhgt_ingest *g, Batch &b, const char *message)
{
    if (hipEventSynchronize(b.ev) != hipSuccess) return fail(g, HHGT_ERR_HIP, message);
    g->free_ev.push(b.ev);
    b.ev = nullptr;
    return true;
}

bool ship_columns(hhgt_ingest *g, Batch &b, hipEvent_t copied)
{
    const double ts0 = now_s();
    if (!wait_batch(g, b, "ingest: compress failed")) return false;
    g->tm.ship_wait_ev += now_s() - ts0;
    trace("ship:compress_done", (long long)b.n_cols);
    DstSlot &d = g->dst[(size_t)b.dst_slot];
    const uint64_t *off = reinterpret_cast<const uint64_t *>(d.h_off.p);
    // the device wrote these offsets, and the last one sizes an allocation and a copy
    bool sane = off[b.n_chunks] <= d.d.cap;
    for (uint64_t i = 0; i < b.n_chunks && sane; ++i) sane = off[i] <= off[i + 1];
    if (!sane) return fail(g, HHGT_ERR_CAPACITY, "ingest: the chunk offset table of a compressed batch is inconsistent");
    b.framed_bytes = off[b.n_chunks];
    const double tso = now_s();
    if (!g->free_out.pop(b.out_slot)) return false;
    g->tm.ship_wait_out += now_s() - tso;
    const double tsc = now_s();
    OutSlot &o = g->out[(size_t)b.out_slot];
    if (o.h.ensure((size_t)b.framed_bytes + 64) != HHGT_OK) return fail(g, HHGT_ERR_HIP, hhgt_last_error());
    o.off.assign(off, off + b.n_chunks + 1);
    if (hipMemcpyAsync(o.h.p, d.d.p, (size_t)b.framed_bytes, hipMemcpyDeviceToHost, g->s_out) != hipSuccess ||
        hipEventRecord(copied, g->s_out) != hipSuccess || hipEventSynchronize(copied) != hipSuccess)
        return fail(g, HHGT_ERR_HIP, "ingest: copy of the framed chunks failed");
    g->tm.ship_copy += now_s() - tsc;
    trace("ship:copied", (long long)b.framed_bytes, (long long)b.n_cols);
    g->free_dst.push(b.dst_slot);
    b.dst_slot = -1;
    b.in->st.raw_bytes += b.raw_bytes;
    b.in->st.compressed_bytes += b.framed_bytes;
    return true;
}

// the input's seconds; HHGT_INGEST_DEBUG: where the threads spent them, then reset (the counters are only read here: a development aid)
void end_of_input_times(hhgt_ingest *g, Input *in)
{
    in->st.seconds = now_s() - in->t_first;
    static const bool dbg = getenv("HHGT_INGEST_DEBUG") != nullptr;
    if (!dbg) return;
    auto &t = g->tm;
    fprintf(stderr, "[hhgt ingest] input %d: %.1f ms | source: wait for a text buffer %.1f | driver: wait for text %.1f, begin_input %.1f, "
            "encode launch %.1f, harvest wait %.1f, harvest work %.1f | shipper: wait for compress %.1f, wait for an out slot %.1f, "
            "copy %.1f (ms)\n",
            in->index, in->st.seconds * 1e3, t.src_wait_text * 1e3, t.drv_wait_text * 1e3, t.drv_begin * 1e3, t.drv_launch * 1e3,
            t.drv_harvest_wait * 1e3, t.drv_harvest * 1e3, t.ship_wait_ev * 1e3, t.ship_wait_out * 1e3, t.ship_copy * 1e3);
    t = hhgt_ingest::Times();
}

void ship_main(hhgt_ingest *g)
{
    hipSetDevice(g->device);
    Event copied;
    hipEventCreateWithFlags(&copied.e, wait_event_flags());
    for (Batch b; g->q_ship.pop(b);) {
        if (b.kind == B_VARIANTS && !wait_batch(g, b, "ingest: variant table copy failed")) break;
        if (b.kind == B_COLUMNS && !ship_columns(g, b, copied)) break;
        if (b.kind == B_INPUT_END) end_of_input_times(g, b.in);
        g->q_out.push(b);
        if (b.kind == B_END) break;
    }
}

// hhgt_ingest_open, step by step
int resolve_opts(const hhgt_ingest_opts *opts, hhgt_ingest_opts *o)
{
    *o = opts ? *opts : hhgt_ingest_opts{};
    if (o->sc <= 0) o->sc = 64;
    if (o->vc <= 0) o->vc = 8192;
    if (o->typesize <= 0) o->typesize = 2;
    if (o->blocksize <= 0) o->blocksize = o->vc * 2 < 8192 ? o->vc * 2 : 8192;
    if (o->format != HHGT_BLOSC1 && o->format != HHGT_BLOSC2) o->format = HHGT_BLOSC2;
    if ((o->sc & (o->sc - 1)) || o->vc % TILE_V) {
        hhgt_set_error("ingest: sc must be a power of two and vc a multiple of %d", TILE_V);
        return HHGT_ERR_ARG;
    }
    return HHGT_OK;
}

int make_streams(hhgt_ingest *g)
{
    OPEN_HIP(hipSetDevice(g->device), "hipSetDevice");
    OPEN_HIP(hipStreamCreateWithFlags(&g->s_main.s, hipStreamNonBlocking), "stream");
    // the copy streams get the highest priority: on this platform pinned copies can run as blit kernels, and a blit
    // queued behind thousands of resident LZ4 / inflate waves crawled at 4-13 GB/s (a 50 MB batch took up to 12 ms,
    // the driver ran out of batch slots and the GPU idled)
    int prio_lo = 0, prio_hi = 0;
    hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    OPEN_HIP(hipStreamCreateWithPriority(&g->s_copy.s, hipStreamNonBlocking, prio_hi), "stream");
    // the inflate streams at the lowest priority: one wave per member lives for the whole launch, so a freed wave slot should
    // go to the encode / compress kernels of the block before, not to the next inflate
    OPEN_HIP(hipStreamCreateWithPriority(&g->s_inf.s, hipStreamNonBlocking, prio_lo), "stream");
    OPEN_HIP(hipStreamCreateWithPriority(&g->s_inf2.s, hipStreamNonBlocking, prio_lo), "stream");
    OPEN_HIP(hipStreamCreateWithFlags(&g->s_carry.s, hipStreamNonBlocking), "stream");
    OPEN_HIP(hipStreamCreateWithPriority(&g->s_out.s, hipStreamNonBlocking, prio_hi), "stream");
    return HHGT_OK;
}

int make_pools(hhgt_ingest *g)
{
    const bool dev = g->o.device_inflate != 0;
    // a text buffer holds a block of the host reader, or of the device inflater where that may run and is larger
    const uint64_t bb_host = block_bytes(g, 64ull << 20), bb_dev = block_bytes(g, 512ull << 20);
    const size_t text_cap = (size_t)(dev && bb_dev > bb_host ? bb_dev : bb_host) + 256;
    g->text = std::vector<TextBuf>(dev ? N_TEXT_DEV : N_TEXT_HOST);
    for (size_t i = 0; i < g->text.size(); ++i) {
        TextBuf &tb = g->text[i];
        OPEN_HIP(hipMalloc(reinterpret_cast<void **>(&tb.d), text_cap), "hipMalloc(text block)");
        tb.cap = text_cap;
        OPEN_HIP(hipEventCreateWithFlags(&tb.ready.e, hipEventDisableTiming), "event");
        OPEN_HIP(hipEventCreateWithFlags(&tb.carry_done.e, hipEventDisableTiming), "event");
        OPEN_HIP(hipHostMalloc(reinterpret_cast<void **>(&tb.h_bad.p), 8, hipHostMallocDefault), "hipHostMalloc");
        g->free_text.push((int)i);
    }
    for (auto &s : g->stg) OPEN_HIP(hipEventCreateWithFlags(&s.done.e, wait_event_flags()), "event");
    for (auto &r : g->res) {
        OPEN_HIP(hipHostMalloc(reinterpret_cast<void **>(&r.rec.p), sizeof(hhgt_encode_result), hipHostMallocDefault), "hipHostMalloc");
        OPEN_HIP(hipEventCreateWithFlags(&r.ev.e, wait_event_flags()), "event");
        OPEN_TRY(r.run_first.ensure(MAX_CHROM_RUNS * 8));
        OPEN_TRY(r.run_names.ensure(MAX_CHROM_RUNS * 32));
    }
    for (int i = 0; i < N_VAR; ++i) g->free_var.push(i);
    for (int i = 0; i < N_DST; ++i) g->free_dst.push(i);
    for (int i = 0; i < N_OUT; ++i) g->free_out.push(i);
    for (auto &e : g->batch_events) {
        OPEN_HIP(hipEventCreateWithFlags(&e.e, wait_event_flags()), "event");
        g->free_ev.push(e.e);
    }
    if (dev) {
        uint32_t t[32];
        crc32_x2n_table(t);
        OPEN_TRY(g->crc_x2n.ensure(sizeof(t)));
        OPEN_HIP(hipMemcpy(g->crc_x2n.p, t, sizeof(t), hipMemcpyHostToDevice), "hipMemcpy");
    }
    return HHGT_OK;
}

// the device inflater's pinned staging of a block's compressed members, and its status words
int presize_device_inflate(hhgt_ingest *g)
{
    const uint64_t bb = block_bytes(g, 512ull << 20), want = (uint64_t)((double)bb / 24.0 * 1.15) + (256u << 10);
    const size_t tab_room = (size_t)(want / 26 + 2) * 28 + 64;
    for (auto &sg : g->stg) {
        OPEN_TRY(sg.h.ensure((size_t)want + 64 + tab_room));
        OPEN_TRY(sg.d.ensure((size_t)want + 64 + tab_room));
    }
    // per text buffer: a status word per member (files written by bgzip hold ~64 KB of text per member; four times as
    // many fit before these grow inside a pass — a hipFree there waits for the device to drain)
    for (auto &tb : g->text) {
        OPEN_TRY(tb.status.ensure((size_t)(bb / 16384 + 64) * 4));
        OPEN_TRY(tb.bad.ensure(8));
    }
    return HHGT_OK;
}

// one chunk column through the compressor on the engine's stream: the first launch of a kernel that spills
// (k_lz4_blocks) makes the runtime allocate the queue's scratch arena — 28 ms inside the first batch of the first
// input otherwise (HHGT_INGEST_DEBUG: "harvest work" 28.1 ms against 0.3)
int warm_compress(hhgt_ingest *g)
{
    InState &X0 = g->ist[0];
    // (what the compressor reads of ring slot 0: planes are not laid out by column, so all of them)
    OPEN_HIP(X0.planes ? hipMemsetAsync(X0.P.p, 0, (size_t)hhgt_planes_bytes(&X0.lay), g->s_main)
                       : hipMemsetAsync(X0.G.p, 0, (size_t)X0.col_bytes, g->s_main), "hipMemsetAsync");
    OPEN_TRY(X0.compress(g->ctx, g->o, 0, 1, g->dst[0], g->s_main));
    OPEN_HIP(hipStreamSynchronize(g->s_main), "hipStreamSynchronize");
    return HHGT_OK;
}

// one small copy each way on every stream the engine copies on (the first copy of a direction on a stream
// sets the runtime's copy path up: milliseconds, once)
int warm_copies(hhgt_ingest *g)
{
    void *cursor = g->ist[0].cursor.p;
    uint8_t *h8 = g->dst[0].h_off.p;   // pinned, >= 16 bytes
    for (hipStream_t st : g->streams()) {
        OPEN_HIP(hipMemcpyAsync(cursor, h8, 8, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
        OPEN_HIP(hipMemcpyAsync(h8 + 8, cursor, 8, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
        OPEN_HIP(hipMemsetAsync(cursor, 0, 8, st), "hipMemsetAsync");
        OPEN_HIP(hipStreamSynchronize(st), "hipStreamSynchronize");
    }
    return HHGT_OK;
}

// every pinned buffer the device will copy into is copied into once, in full (HHGT_INGEST_DEBUG=2 showed the
// first device -> host copy into each fresh pinned slot taking 7-10 ms where later ones take microseconds)
int touch_pinned_slots(hhgt_ingest *g)
{
    const InState &X0 = g->ist[0];
    auto least = [](size_t a, size_t b) { return a < b ? a : b; };
    for (auto &v : g->var) {
        const size_t n4 = least(v.start.cap, X0.t_start.cap), n1 = least(v.ref.cap, X0.t_ref.cap);
        OPEN_HIP(hipMemcpyAsync(v.start.p, X0.t_start.p, n4, hipMemcpyDeviceToHost, g->s_main), "hipMemcpyAsync");
        OPEN_HIP(hipMemcpyAsync(v.ref.p, X0.t_ref.p, n1, hipMemcpyDeviceToHost, g->s_main), "hipMemcpyAsync");
        OPEN_HIP(hipMemcpyAsync(v.alt.p, X0.t_alt.p, n1, hipMemcpyDeviceToHost, g->s_main), "hipMemcpyAsync");
    }
    for (auto &d : g->dst)
        OPEN_HIP(hipMemcpyAsync(d.h_off.p, d.off.p, least(d.h_off.cap, d.off.cap), hipMemcpyDeviceToHost, g->s_main), "hipMemcpyAsync");
    for (auto &o : g->out)
        OPEN_HIP(hipMemcpyAsync(o.h.p, g->dst[0].d.p, least(o.h.cap, g->dst[0].d.cap), hipMemcpyDeviceToHost, g->s_out), "hipMemcpyAsync");
    OPEN_HIP(hipStreamSynchronize(g->s_main), "hipStreamSynchronize");
    OPEN_HIP(hipStreamSynchronize(g->s_out), "hipStreamSynchronize");
    return HHGT_OK;
}

// the caller knows the cohort's width: everything whose size follows from it is made (and pinned) now instead of
// inside the first input — both ring states, the batch slots, the shipper's pinned copies, and for the device
// inflater the pinned staging of a block's compressed members
int prepare_for_expected_samples(hhgt_ingest *g)
{
    const uint64_t S = g->o.sites_only ? 0ull : (uint64_t)g->o.expect_samples, text_cap = g->text[0].cap;
    for (auto &X : g->ist)
        if (!size_input_state(g, &X, S, (uint64_t)g->o.expect_samples, text_cap, true)) return g->err ? g->err : HHGT_ERR_HIP;
    // the context's own workspaces for a block / a batch of that size
    const InState &X0 = g->ist[0];
    OPEN_TRY(hhgt_reserve(g->ctx, text_cap, (uint32_t)X0.kept_per_block, (X0.kept_per_block / (uint64_t)g->o.vc + 4) * X0.n_sc,
                          X0.chunk_nbytes, g->o.typesize, g->o.blocksize));
    if (g->o.device_inflate != 0) OPEN_TRY(presize_device_inflate(g));
    if (g->o.device_inflate != 1) hhgt_reader_prewarm(block_bytes(g, 64ull << 20), 6 * ((g->o.files_ahead > 0 ? g->o.files_ahead : 1) + 1));
    if (S > 0) OPEN_TRY(warm_compress(g));
    OPEN_TRY(warm_copies(g));
    if (S > 0) OPEN_TRY(touch_pinned_slots(g));
    return HHGT_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// C entry points
// ---------------------------------------------------------------------------------------------------------------
extern "C" int hhgt_ingest_open(hhgt_ctx *ctx, const hhgt_ingest_opts *opts, hhgt_ingest **out)
{
    if (!ctx || !out) return HHGT_ERR_ARG;
    *out = nullptr;
    hhgt_ingest_opts o;
    OPEN_TRY(resolve_opts(opts, &o));
    // a failing step leaves through hhgt_ingest_close: no thread was started, it synchronises whatever streams exist, then releases
    std::unique_ptr<hhgt_ingest, void (*)(hhgt_ingest *)> owner(new hhgt_ingest(), hhgt_ingest_close);
    hhgt_ingest *g = owner.get();
    g->ctx = ctx;
    g->device = ctx->device;
    g->o = o;
    OPEN_TRY(make_streams(g));
    OPEN_TRY(make_pools(g));
    if (g->o.expect_samples > 0) OPEN_TRY(prepare_for_expected_samples(g));
    g->th_source = std::thread(source_main, g);
    g->th_driver = std::thread(driver_main, g);
    g->th_ship = std::thread(ship_main, g);
    *out = owner.release();
    return HHGT_OK;
}

static int add_input(hhgt_ingest *g, std::unique_ptr<Input> in)
{
    std::lock_guard<std::mutex> lk(g->in_mu);
    if (g->finished) {
        hhgt_set_error("ingest: inputs cannot be added after hhgt_ingest_finish");
        return HHGT_ERR_ARG;
    }
    in->index = (int)g->inputs.size();
    const int idx = in->index;
    g->inputs.push_back(std::move(in));
    g->in_cv.notify_all();
    return idx;
}

extern "C" int hhgt_ingest_add_file(hhgt_ingest *g, const char *path, const char *region)
{
    if (!g || !path) return HHGT_ERR_ARG;
    trace("add_file");
    if (access(path, R_OK) != 0) {
        hhgt_set_error("cannot open %s", path);
        return HHGT_ERR_IO;
    }
    std::unique_ptr<Input> in(new Input());
    in->kind = 0;
    in->path = path;
    in->region = region ? region : "";
    return add_input(g, std::move(in));
}

extern "C" int hhgt_ingest_add_memory(hhgt_ingest *g, const void *host_text, uint64_t nbytes, const char *region)
{
    if (!g || (!host_text && nbytes)) return HHGT_ERR_ARG;
    std::unique_ptr<Input> in(new Input());
    in->kind = 1;
    in->mem = static_cast<const uint8_t *>(host_text);
    in->mem_bytes = nbytes;
    in->region = region ? region : "";
    return add_input(g, std::move(in));
}

extern "C" int hhgt_ingest_finish(hhgt_ingest *g)
{
    if (!g) return HHGT_ERR_ARG;
    {
        std::lock_guard<std::mutex> lk(g->in_mu);
        g->finished = true;
    }
    g->in_cv.notify_all();
    return HHGT_OK;
}

static void release_held(hhgt_ingest *g)
{
    if (!g->have_held) return;
    if (g->held.var_slot >= 0) g->free_var.push(g->held.var_slot);
    if (g->held.out_slot >= 0) g->free_out.push(g->held.out_slot);
    g->have_held = false;
}

extern "C" int hhgt_ingest_next(hhgt_ingest *g, hhgt_ingest_event *ev)
{
    if (!g || !ev) return HHGT_ERR_ARG;
    memset(ev, 0, sizeof(*ev));
    release_held(g);
    if (g->ended) return HHGT_OK;   // kind stays HHGT_EV_END
    Batch b;
    if (!g->q_out.pop(b)) {
        std::lock_guard<std::mutex> lk(g->err_mu);
        hhgt_set_error("%s", g->errmsg.empty() ? "ingest: stopped" : g->errmsg.c_str());
        g->ended = true;
        return g->err ? g->err : HHGT_ERR_IO;
    }
    g->held = b;
    g->have_held = true;
    ev->kind = b.kind;
    ev->input = b.in ? b.in->index : -1;
    switch (b.kind) {
    case B_HEADER:
        ev->header = b.in->header.data();
        ev->header_bytes = b.in->header.size();
        ev->n_samples = b.in->S;
        break;
    case B_VARIANTS: {
        VarSlot &v = g->var[(size_t)b.var_slot];
        ev->start = reinterpret_cast<const uint32_t *>(v.start.p);
        ev->ref = v.ref.p;
        ev->alt = v.alt.p;
        ev->first_variant = b.first_variant;
        ev->n_variants = b.n_variants;
        ev->n_runs = b.n_runs;
        ev->run_first = v.run_first;
        ev->run_names = &v.run_names[0][0];
        break;
    }
    case B_COLUMNS: {
        OutSlot &o = g->out[(size_t)b.out_slot];
        ev->framed = o.h.p;
        ev->chunk_off = o.off.data();
        ev->framed_bytes = b.framed_bytes;
        ev->n_chunks = b.n_chunks;
        ev->first_col = b.first_col;
        ev->n_cols = b.n_cols;
        ev->raw_bytes = b.raw_bytes;
        break;
    }
    case B_INPUT_END:
        ev->stats = b.in->st;
        break;
    default:
        g->ended = true;
        break;
    }
    return HHGT_OK;
}

// The event returned by the last hhgt_ingest_next keeps its buffers past the next call: the consumer writes a batch of
// chunks to a file on another thread while it already takes the next event (round 4: the converter's run was the engine's
// 0.2 s stretched to 0.7 by the consumer's writes).  The token names the slots; hhgt_ingest_release may come from any thread.
extern "C" int hhgt_ingest_hold(hhgt_ingest *g, int *token)
{
    if (!g || !token) return HHGT_ERR_ARG;
    if (!g->have_held) {
        hhgt_set_error("hhgt_ingest_hold: no event is held (call it after hhgt_ingest_next, once per event)");
        return HHGT_ERR_ARG;
    }
    *token = (g->held.out_slot + 1) | ((g->held.var_slot + 1) << 8);
    g->have_held = false;
    return HHGT_OK;
}

extern "C" int hhgt_ingest_release(hhgt_ingest *g, int token)
{
    if (!g || token < 0) return HHGT_ERR_ARG;
    const int out = (token & 0xFF) - 1, var = ((token >> 8) & 0xFF) - 1;
    if (out >= N_OUT || var >= N_VAR) return HHGT_ERR_ARG;
    if (var >= 0) g->free_var.push(var);
    if (out >= 0) g->free_out.push(out);
    return HHGT_OK;
}

extern "C" void hhgt_ingest_close(hhgt_ingest *g)
{
    if (!g) return;
    hipSetDevice(g->device);
    if (!g->ended) fail(g, HHGT_ERR_IO, "ingest: closed");   // stop the stages (a normal end has already drained them)
    hhgt_ingest_finish(g);
    for (std::thread *t : {&g->th_source, &g->th_driver, &g->th_ship})
        if (t->joinable()) t->join();
    if (trace_level() >= 2) {
        std::lock_guard<std::mutex> lk(g_trace_mu);
        const double t0 = g_trace.empty() ? 0 : g_trace[0].t;
        fprintf(stderr, "[trace] t0 = %.3f ms (steady clock; HHGT_ALLOC_DEBUG lines carry the same clock)\n", t0 * 1e3);
        for (auto &r : g_trace) fprintf(stderr, "[trace] %9.3f ms  %-20s %lld %lld\n", (r.t - t0) * 1e3, r.tag, r.a, r.b);
        g_trace.clear();
    }
    for (hipStream_t s : g->streams())
        if (s) hipStreamSynchronize(s);
    {   // readers opened ahead and never run
        std::lock_guard<std::mutex> lk(g->in_mu);
        for (auto &in : g->inputs)
            if (in->rd) hhgt_reader_close(in->rd);
    }
    delete g;   // every buffer and event by its holder; the streams, declared first, go last
}
