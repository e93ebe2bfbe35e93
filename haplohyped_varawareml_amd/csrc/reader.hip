// reader.hip — host-side VCF text reader (see include/hhgt_reader.h): mmap + zlib inflate into a ring of pinned,
// line-aligned blocks; hipMemcpyAsync to HBM.  Host C++ only (compiled by hipcc with the rest of libhhgt.so); no
// device code in this file.
//
// BGZF (the format htslib reads under /root/reference/cpp/vcfpp.h:1381,1468): the scanner thread walks the member
// headers — every member's inflated size sits in its trailer, so the place of every member's text in the ring is
// known before anything is inflated — and hands the members to a pool of inflate workers as per-block task lists.
// There is NO barrier per block: workers move from one block's list to the next while the scanner is already laying
// out later blocks, and a block is published to the consumer when its last task finishes.  The one dependency
// between blocks, the partial last line that moves to the front of the next block, is resolved by the scanner
// itself: it inflates the block's LAST member right away (30 us of zlib), finds the last newline in it and thereby
// knows where the next block's members start.  (Round 1 filled one block at a time with a wake-all / wait-all
// around it: 48 threads delivered 20 GB/s of text where one delivers 2.2.)
// Every member's text is hashed and compared with the CRC-32 in its trailer, as htslib's bgzf.c does (crc32.h).
// Plain gzip streams through one inflater, uncompressed files are pread into the ring by the same worker pool.
//
// What the reader holds sits in owners (host_owners.h, BlockBuf): open and close have no cleanup code of their own.
#include "common.h"
#include "../../include/hhgt_reader.h"
#include "crc32.h"
#include "fast_inflate.h"
#include "host_owners.h"
#include <sys/stat.h>
#include <fcntl.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>

// Pinned ring blocks are expensive to make (hipHostMalloc pins page by page) and a converter opens one reader per
// chromosome file: closed readers park their blocks here and the next open takes them back.
static std::mutex g_pool_mu;
static std::vector<std::pair<size_t, void *>> g_pool;
#define POOL_MAX_BLOCKS 32

static void *pool_take(size_t bytes)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); ++i)
        if (g_pool[i].first == bytes) {
            void *p = g_pool[i].second;
            g_pool.erase(g_pool.begin() + (long)i);
            return p;
        }
    return nullptr;
}

static bool pool_give(size_t bytes, void *p)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (g_pool.size() >= POOL_MAX_BLOCKS) return false;
    g_pool.emplace_back(bytes, p);
    return true;
}

extern "C" void hhgt_reader_trim_pool(void)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (auto &e : g_pool) (void)hipHostFree(e.second);
    g_pool.clear();
}

extern "C" int hhgt_reader_prewarm(uint64_t block_bytes, int n_blocks)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return 0;
    if (n_blocks > POOL_MAX_BLOCKS) n_blocks = POOL_MAX_BLOCKS;
    int have = 0;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (auto &e : g_pool) have += e.first == (size_t)block_bytes ? 1 : 0;
    }
    while (have < n_blocks) {
        void *p = nullptr;
        if (hipHostMalloc(&p, (size_t)block_bytes, hipHostMallocDefault) != hipSuccess) break;
        if (!pool_give((size_t)block_bytes, p)) {
            (void)hipHostFree(p);
            break;
        }
        ++have;
    }
    return have;
}

namespace {

// a ring block's memory, which knows how it goes back: pinned to the pool (or hipHostFree when that is full), pageable to free
struct BlockBuf : NoCopy {
    uint8_t *p = nullptr;
    size_t bytes = 0;
    bool pinned = false;
    // Pinned, from the pool or fresh, while *pin holds.  The first hipHostMalloc that fails clears it: that block and the
    // later ones are pageable, the earlier ones stay pinned.
    bool make(size_t n, bool *pin)
    {
        void *m = *pin ? pool_take(n) : nullptr;
        if (!m && *pin && hipHostMalloc(&m, n, hipHostMallocDefault) != hipSuccess) {
            *pin = false;
            m = nullptr;
        }
        pinned = m != nullptr;
        if (!m) m = malloc(n);
        p = static_cast<uint8_t *>(m);
        bytes = n;
        return p != nullptr;
    }
    ~BlockBuf()
    {
        if (!p) return;
        if (!pinned) free(p);
        else if (!pool_give(bytes, p)) (void)hipHostFree(p);
    }
};

struct Task {
    const uint8_t *src = nullptr;
    uint32_t src_len = 0;
    uint8_t *dst = nullptr;
    uint32_t dst_len = 0;
    int fd = -1;            // >= 0: an uncompressed piece, read with pread(fd, dst, dst_len, file_off)
    uint64_t file_off = 0;
    bool check_crc = false;  // BGZF member: compare crc32(dst) with the trailer behind src
};

// one ring block: its task list is written by the scanner before the block is opened to the workers
struct Block {
    BlockBuf buf;
    size_t n = 0;                      // published bytes (whole lines)
    std::vector<Task> tasks;
    // generation << 32 | next task to draw.  Workers advance it by compare-and-swap against the generation they were
    // given with the block, so a worker that still holds a recycled block can neither run a task of its next life
    // nor swallow one of its tickets
    std::atomic<uint64_t> ticket{0};
    std::atomic<uint32_t> done{0};     // tasks finished
    uint32_t gen = 0;
    uint32_t n_tasks = 0;
    bool scanned = false;              // layout complete (n, n_tasks final)
    bool last = false;                 // last block of the input
    bool held = false;                 // in the consumer's hands
};

// every text a read can fail with
const char *const ERR_LONG_LINE = "a line is longer than the reader's block size";
const char *const ERR_HEADER = "corrupt BGZF block header";
const char *const ERR_TRUNCATED = "truncated compressed input";
const char *const ERR_INFLATE = "inflate failed";
const char *const ERR_CRC = "BGZF member: CRC32 checksum mismatch";

}  // namespace

struct hhgt_reader {
    Fd file;
    Mapping map;
    bool is_gzip = false, is_bgzf = false;
    bool check_crc = true;   // HHGT_BGZF_NO_CRC=1 skips the per-member CRC32 (htslib always checks it)
    size_t block_bytes = 0;
    int n_blocks = 0;
    std::unique_ptr<Block[]> ring;
    // block life cycle: free_ -> (scanner) open_ (workers draw tasks) -> order (publication order) -> held by the
    // consumer -> free_
    std::deque<int> free_, open_, order;
    int auto_held = -1;              // block handed out by hhgt_reader_next (released by the following call)
    bool eof = false, stop = false;  // eof: the scanner has laid out the last block
    int error = 0;
    std::string errmsg;
    std::mutex mu;                   // guards the deques, eof/stop/error and the blocks' `held`
    std::condition_variable cv_free, cv_open, cv_pub;
    std::thread producer;
    std::vector<std::thread> workers;
    // totals for hhgt_reader_stats, published by the scanner with each block (its own cursor is private to it)
    std::atomic<uint64_t> file_bytes{0}, text_bytes{0};
};

// one cgroup's CPU quota: false when the cgroup has no such file, *quota stays <= 0 when the file sets none
static bool cgroup_v2_quota(long long *quota, long long *period)
{
    FILE *fp = fopen("/sys/fs/cgroup/cpu.max", "r");
    if (!fp) return false;
    char a[64] = "", b[64] = "";
    const int got = fscanf(fp, "%63s %63s", a, b);
    fclose(fp);
    if (got >= 1 && strcmp(a, "max") != 0) *quota = atoll(a);
    if (got >= 2) *period = atoll(b);
    return true;
}

static bool cgroup_v1_quota(long long *quota, long long *period)
{
    FILE *fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r");
    if (!fp) return false;
    char a[64] = "";
    if (fscanf(fp, "%63s", a) == 1) *quota = atoll(a);
    fclose(fp);
    fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
    if (fp) {
        if (fscanf(fp, "%63s", a) == 1) *period = atoll(a);
        fclose(fp);
    }
    return true;
}

// CPUs this process may actually use: the affinity mask, capped by the cgroup's CPU quota (a GPU box of this pool
// shows 256 hardware threads and grants 16 CPUs' worth of time: 96 inflate threads on it only fight each other)
extern "C" int hhgt_effective_cpus(void)
{
    int n = (int)std::thread::hardware_concurrency();
    auto cap = [&n](long long k) {
        if (k > 0 && (n <= 0 || k < n)) n = (int)k;
    };
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0) cap(CPU_COUNT(&set));
    long long quota = -1, period = 100000;
    if (!cgroup_v2_quota(&quota, &period)) cgroup_v1_quota(&quota, &period);
    if (quota > 0 && period > 0) cap((int)((quota + period - 1) / period));
    return n > 0 ? n : 1;
}

extern "C" int hhgt_fast_inflate(const void *in, uint64_t in_len, void *out, uint64_t out_len)
{
    return hhgt_fast_inflate_impl(static_cast<const uint8_t *>(in), (size_t)in_len, static_cast<uint8_t *>(out), (size_t)out_len);
}

extern "C" uint32_t hhgt_crc32(const void *data, uint64_t n) { return hhgt_crc::crc32(data, (size_t)n); }

// ---- tasks --------------------------------------------------------------------------------------------------------
// nullptr, or the text the read fails with
static const char *run_task(Inflater &z, const Task &t)
{
    if (t.fd >= 0) {
        // plain-text piece of an uncompressed file: pread straight into the pinned block.  (A memcpy out of the
        // mapping takes a minor fault per 4 KiB page it touches first; the copy inside read() does not.)
        size_t got = 0;
        while (got < t.dst_len) {
            ssize_t k = pread(t.fd, t.dst + got, t.dst_len - got, (off_t)(t.file_off + got));
            if (k <= 0) return ERR_INFLATE;
            got += (size_t)k;
        }
        return nullptr;
    }
    // own decoder first (fast_inflate.h: ~4x zlib on genotype text); whatever it does not accept goes to zlib, which
    // stays the arbiter of what is a corrupt member (HHGT_ZLIB_INFLATE=1: zlib only)
    static const bool zlib_only = getenv("HHGT_ZLIB_INFLATE") && atoi(getenv("HHGT_ZLIB_INFLATE")) != 0;
    if ((zlib_only || hhgt_fast_inflate_impl(t.src, t.src_len, t.dst, t.dst_len) != 0) && !z.member(t.src, t.src_len, t.dst, t.dst_len))
        return ERR_INFLATE;
    if (t.check_crc) {
        // the member's trailer (CRC32, ISIZE) follows the payload; htslib's bgzf.c rejects a member whose text does
        // not hash to it ("CRC32 checksum mismatch")
        const uint8_t *tr = t.src + t.src_len;
        const uint32_t want = (uint32_t)tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24);
        if (hhgt_crc::crc32(t.dst, t.dst_len) != want) return ERR_CRC;
    }
    return nullptr;
}

static void set_error(hhgt_reader *r, const char *msg)
{
    std::lock_guard<std::mutex> lk(r->mu);
    if (!r->error) {
        r->error = HHGT_ERR_IO;
        r->errmsg = msg;
    }
    r->eof = true;
    r->cv_pub.notify_all();
    r->cv_open.notify_all();
    r->cv_free.notify_all();
}

#define TASK_BATCH 4u

static void worker_main(hhgt_reader *r)
{
    Inflater z;
    for (;;) {
        int bi;
        uint32_t gen, n_tasks;
        {
            std::unique_lock<std::mutex> lk(r->mu);
            r->cv_open.wait(lk, [&] { return r->stop || !r->open_.empty(); });
            if (r->stop) break;
            bi = r->open_.front();
            gen = r->ring[bi].gen;
            n_tasks = r->ring[bi].n_tasks;
        }
        Block &b = r->ring[bi];
        for (;;) {
            uint64_t cur = b.ticket.load();
            bool got = false;
            while ((uint32_t)(cur >> 32) == gen && (uint32_t)cur < n_tasks) {
                if (b.ticket.compare_exchange_weak(cur, cur + TASK_BATCH)) {
                    got = true;
                    break;
                }
            }
            if (!got) break;
            const uint32_t t0 = (uint32_t)cur;
            const uint32_t t1 = t0 + TASK_BATCH < n_tasks ? t0 + TASK_BATCH : n_tasks;
            for (uint32_t t = t0; t < t1; ++t)
                if (const char *err = run_task(z, b.tasks[t])) set_error(r, err);
            if (b.done.fetch_add(t1 - t0) + (t1 - t0) == n_tasks) {
                std::lock_guard<std::mutex> lk(r->mu);   // the block's last task: it may be published now
                r->cv_pub.notify_all();
            }
        }
        {
            std::lock_guard<std::mutex> lk(r->mu);       // exhausted: take it off the open list (once per life)
            if (!r->open_.empty() && r->open_.front() == bi && r->ring[bi].gen == gen) r->open_.pop_front();
        }
    }
}

// ---- scanner: the steps every source shares ---------------------------------------------------------------------
// a free block (waits), or -1 when the reader is closing
static int take_free(hhgt_reader *r)
{
    std::unique_lock<std::mutex> lk(r->mu);
    r->cv_free.wait(lk, [&] { return r->stop || !r->free_.empty(); });
    if (r->stop) return -1;
    int bi = r->free_.front();
    r->free_.pop_front();
    Block &b = r->ring[bi];
    b.tasks.clear();
    b.n_tasks = 0;
    b.n = 0;
    b.scanned = false;
    b.last = false;
    return bi;
}

// the block's layout is final: open it to the workers and put it in publication order
static void open_block(hhgt_reader *r, int bi, size_t pub, bool last)
{
    Block &b = r->ring[bi];
    b.n = pub;
    b.n_tasks = (uint32_t)b.tasks.size();
    b.last = last;
    r->text_bytes.fetch_add(pub);
    {
        std::lock_guard<std::mutex> lk(r->mu);
        b.gen += 1;
        b.done.store(0);
        b.ticket.store((uint64_t)b.gen << 32);
        b.scanned = true;
        r->order.push_back(bi);
        if (b.n_tasks) r->open_.push_back(bi);
        if (last) r->eof = true;
    }
    r->cv_open.notify_all();
    r->cv_pub.notify_all();
}

// offset behind the last newline of p[0, n), or 0 when there is none
static size_t line_end(const uint8_t *p, size_t n)
{
    const void *nl = n ? memrchr(p, '\n', n) : nullptr;
    return nl ? (size_t)((const uint8_t *)nl - p) + 1 : 0;
}

namespace {
// The block the scanner is laying out, and what it carries from block to block: its place in the file and the partial last
// line.  A source calls begin(), lays out `n` bytes behind the carried ones, looks for the last newline where it may (BGZF: in
// members, inflated from the back; gzip: in the block; plain: in the mapping, before anything is read) and calls cut().
struct Scan : NoCopy {
    hhgt_reader *const r;
    size_t pos = 0;               // next unread byte of the file
    std::vector<uint8_t> carry;   // bytes behind the previous block's last newline: they hold none
    int bi = -1;
    Block *b = nullptr;
    size_t n = 0;                 // bytes laid out in *b
    explicit Scan(hhgt_reader *r_) : r(r_) {}
    bool input_done() const { return pos >= r->map.len; }
    size_t room() const { return r->block_bytes - n; }
    // a free block with the carried bytes at its front; false when the reader is closing
    bool begin()
    {
        bi = take_free(r);
        if (bi < 0) return false;
        b = &r->ring[bi];
        n = carry.size();
        if (n) memcpy(b->buf.p, carry.data(), n);
        carry.clear();
        return true;
    }
    // The line cut.  `end` = offset in the block behind the last newline the source found, 0 for none.  Publishes the block up
    // to there and carries the rest — all of it when it is the last of the input, final newline or not — or fails the read: a
    // line that does not end in this block does not fit any.  false: the scanner is done.
    bool cut(size_t end, bool last)
    {
        if (last) end = n;
        else if (!end) {
            set_error(r, ERR_LONG_LINE);
            return false;
        }
        carry.assign(b->buf.p + end, b->buf.p + n);
        r->file_bytes.store(pos);
        open_block(r, bi, end, last);
        return !last;
    }
};
}  // namespace

// ---- BGZF: barrier-free scanner --------------------------------------------------------------------------------
static bool looks_bgzf(const uint8_t *p, size_t n)
{
    return n >= 18 && p[0] == 0x1f && p[1] == 0x8b && p[2] == 8 && (p[3] & 4) && p[10] == 6 && p[11] == 0 &&
           p[12] == 'B' && p[13] == 'C' && p[14] == 2 && p[15] == 0;
}

// The member at p, of which `left` bytes are mapped: its payload and the size of its text (ISIZE) as a task that still lacks
// its place in a block, and the member's whole size; or the text the read fails with.
static const char *parse_member(const uint8_t *p, size_t left, Task *t, size_t *size)
{
    if (!looks_bgzf(p, left)) return ERR_HEADER;
    *size = (size_t)((uint32_t)p[16] | ((uint32_t)p[17] << 8)) + 1;
    if (*size > left || *size < 26) return ERR_TRUNCATED;
    const uint8_t *tr = p + *size - 4;
    t->dst_len = (uint32_t)tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24);
    if (t->dst_len > 65536) return ERR_INFLATE;
    t->src = p + 18;
    t->src_len = (uint32_t)(*size - 18 - 8);
    return nullptr;
}

// members become tasks while their text fits the block
static const char *lay_out_members(Scan &s)
{
    const hhgt_reader *r = s.r;
    while (!s.input_done()) {
        Task t;
        size_t size;
        if (const char *err = parse_member(r->map.p + s.pos, r->map.len - s.pos, &t, &size)) return err;
        if (t.dst_len > s.room()) break;
        t.dst = s.b->buf.p + s.n;
        t.check_crc = r->check_crc;
        if (t.dst_len) s.b->tasks.push_back(t);
        s.n += t.dst_len;
        s.pos += size;
    }
    return nullptr;
}

// Where does the last whole line end?  Inflate members from the back (normally just the last one) until one holds a
// newline; they are done here, so they leave the task list.  *end stays 0 when no member holds one: the carried bytes in
// front of them hold none either (Scan::carry), so no line ends in this block.
static const char *last_line_end(Block &b, Inflater &z, size_t *end)
{
    while (!*end && !b.tasks.empty()) {
        const Task t = b.tasks.back();
        b.tasks.pop_back();
        if (const char *err = run_task(z, t)) return err;
        if (const size_t e = line_end(t.dst, t.dst_len)) *end = (size_t)(t.dst - b.buf.p) + e;
    }
    return nullptr;
}

static void scan_bgzf(hhgt_reader *r)
{
    Scan s(r);
    Inflater z;
    size_t end;
    do {
        if (!s.begin()) return;
        const char *err = lay_out_members(s);
        end = 0;
        if (!err && !s.input_done()) err = last_line_end(*s.b, z, &end);
        if (err) return set_error(r, err);
    } while (s.cut(end, s.input_done()));
}

// ---- plain gzip (one stream) and uncompressed input ------------------------------------------------------------
// inflates into dst[0, cap) until it is full or the file ends; a gzip member may follow another
static const char *fill_gzip(Scan &s, GzipInflater &z, uint8_t *dst, size_t cap, size_t *produced)
{
    const Mapping &map = s.r->map;
    *produced = 0;
    while (*produced < cap) {
        if (!z.open) {
            if (s.input_done()) break;
            if (!z.begin()) return ERR_INFLATE;
        }
        const uInt chunk_in = (uInt)std::min<size_t>(map.len - s.pos, 1u << 30);
        const uInt chunk_out = (uInt)std::min<size_t>(cap - *produced, 1u << 30);
        z.zs.next_in = const_cast<Bytef *>(map.p + s.pos);
        z.zs.avail_in = chunk_in;
        z.zs.next_out = dst + *produced;
        z.zs.avail_out = chunk_out;
        const int rc = inflate(&z.zs, Z_NO_FLUSH);
        s.pos += chunk_in - z.zs.avail_in;
        *produced += chunk_out - z.zs.avail_out;
        if (rc == Z_STREAM_END) {  // gzip member finished; another may follow
            z.end();
            continue;
        }
        if (rc == Z_BUF_ERROR && chunk_in == 0) return ERR_TRUNCATED;
        if (rc != Z_OK && rc != Z_BUF_ERROR) return ERR_INFLATE;
        if (s.input_done() && z.zs.avail_out != 0) return ERR_TRUNCATED;   // input exhausted mid-member
    }
    return nullptr;
}

static void scan_gzip(hhgt_reader *r)
{
    Scan s(r);
    GzipInflater z;
    bool last;
    do {
        if (!s.begin()) return;
        size_t got = 0;
        if (const char *err = fill_gzip(s, z, s.b->buf.p + s.n, s.room(), &got)) return set_error(r, err);
        s.n += got;
        last = s.input_done() && (!z.open || got == 0);
    } while (s.cut(line_end(s.b->buf.p, s.n), last));
}

// uncompressed: the cut is found in the mapping itself, the bytes are pread by the workers in pieces of 4 MiB
static void scan_plain(hhgt_reader *r)
{
    Scan s(r);
    size_t take;
    bool last;
    do {
        if (!s.begin()) return;
        take = std::min(r->map.len - s.pos, s.room());
        last = s.pos + take == r->map.len;
        if (!last) take = line_end(r->map.p + s.pos, take);
        const size_t piece = 4u << 20;
        for (size_t o = 0; o < take; o += piece) {
            Task t;
            t.dst = s.b->buf.p + s.n + o;
            t.dst_len = (uint32_t)std::min(take - o, piece);
            t.fd = r->file.fd;
            t.file_off = s.pos + o;
            s.b->tasks.push_back(t);
        }
        s.pos += take;
        s.n += take;
    } while (s.cut(take ? s.n : 0, last));
}

static void producer_main(hhgt_reader *r)
{
    if (r->map.len == 0) {   // an empty file: no block will say that it is the last
        std::lock_guard<std::mutex> lk(r->mu);
        r->eof = true;
        r->cv_pub.notify_all();
    } else if (r->is_bgzf)
        scan_bgzf(r);
    else if (r->is_gzip)
        scan_gzip(r);
    else
        scan_plain(r);
}

// BGZF default: one worker per CPU the process may use (hhgt_effective_cpus), at most 96; HHGT_READER_THREADS or the
// n_threads argument override, up to 192.  Uncompressed input: 16 pread threads saturate the page cache copy.  Plain gzip
// is inflated by the scanner alone.
static int worker_count(const hhgt_reader *r, int n_threads)
{
    if (r->is_gzip && !r->is_bgzf) return 0;
    const char *e = getenv("HHGT_READER_THREADS");
    const int eff = hhgt_effective_cpus();
    int nt = n_threads > 0 ? n_threads : (e && atoi(e) > 0 ? atoi(e) : (eff < 96 ? eff : 96));
    if (nt > 192) nt = 192;
    if (!r->is_bgzf && nt > 16) nt = 16;
    return nt;
}

extern "C" int hhgt_reader_open(const char *path, uint64_t block_bytes, int n_threads, int n_blocks, hhgt_reader **out)
{
    if (!path || !out) return HHGT_ERR_ARG;
    *out = nullptr;
    if (block_bytes < (1u << 20)) block_bytes = 1u << 20;
    if (n_blocks <= 0) n_blocks = 4;
    if (n_blocks < 2) n_blocks = 2;
    std::unique_ptr<hhgt_reader> r(new hhgt_reader());
    r->file.fd = open(path, O_RDONLY);
    if (r->file.fd < 0) {
        hhgt_set_error("cannot open %s", path);
        return HHGT_ERR_IO;
    }
    struct stat st;
    if (fstat(r->file.fd, &st) != 0) {
        hhgt_set_error("cannot stat %s", path);
        return HHGT_ERR_IO;
    }
    if (st.st_size) {
        void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, r->file.fd, 0);
        if (m == MAP_FAILED) {
            hhgt_set_error("cannot mmap %s", path);
            return HHGT_ERR_IO;
        }
        madvise(m, (size_t)st.st_size, MADV_SEQUENTIAL);
        r->map.p = static_cast<const uint8_t *>(m);
        r->map.len = (size_t)st.st_size;
    }
    r->is_gzip = r->map.len >= 2 && r->map.p[0] == 0x1f && r->map.p[1] == 0x8b;
    r->is_bgzf = r->is_gzip && looks_bgzf(r->map.p, r->map.len);
    const char *no_crc = getenv("HHGT_BGZF_NO_CRC");
    r->check_crc = !(no_crc && *no_crc && *no_crc != '0');
    r->block_bytes = (size_t)block_bytes;
    r->n_blocks = n_blocks;
    r->ring.reset(new Block[(size_t)n_blocks]);
    // pinned when a HIP device exists (the copy engine can then DMA straight out of the ring);
    // plain pages otherwise (CPU-only hosts still frame and inflate, e.g. in the CPU test suite)
    int ndev = 0;
    bool pin = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    for (int i = 0; i < n_blocks; ++i) {
        if (!r->ring[i].buf.make(r->block_bytes, &pin)) {
            hhgt_set_error("reader: out of memory for %zu-byte blocks", r->block_bytes);
            return HHGT_ERR_IO;
        }
        r->free_.push_back(i);
    }
    // nothing below can fail: the threads only start once the reader is whole
    for (int i = worker_count(r.get(), n_threads); i > 0; --i) r->workers.emplace_back(worker_main, r.get());
    r->producer = std::thread(producer_main, r.get());
    *out = r.release();
    return HHGT_OK;
}

extern "C" void hhgt_reader_close(hhgt_reader *r)
{
    if (!r) return;
    {
        std::lock_guard<std::mutex> lk(r->mu);
        r->stop = true;
    }
    r->cv_free.notify_all();
    r->cv_open.notify_all();
    r->cv_pub.notify_all();
    r->producer.join();
    for (auto &t : r->workers) t.join();
    delete r;
}

extern "C" int hhgt_reader_is_bgzf(const hhgt_reader *r) { return r && r->is_bgzf ? 1 : 0; }

extern "C" int hhgt_reader_acquire(hhgt_reader *r, const void **host_ptr, uint64_t *nbytes, int *token, int *is_last)
{
    if (!r || !host_ptr || !nbytes || !token) return HHGT_ERR_ARG;
    *host_ptr = nullptr;
    *nbytes = 0;
    *token = -1;
    if (is_last) *is_last = 0;
    std::unique_lock<std::mutex> lk(r->mu);
    for (;;) {
        if (r->error) {
            hhgt_set_error("reader: %s", r->errmsg.c_str());
            return r->error;
        }
        const int bi = r->order.empty() ? -1 : r->order.front();
        if (bi < 0 && r->eof) return HHGT_OK;   // end of file
        if (bi < 0 || !r->ring[bi].scanned || r->ring[bi].done.load() < r->ring[bi].n_tasks) {
            if (r->stop) return HHGT_OK;
            r->cv_pub.wait(lk);
            continue;
        }
        Block &b = r->ring[bi];
        r->order.pop_front();
        if (b.n) {
            b.held = true;
            *host_ptr = b.buf.p;
            *nbytes = b.n;
            *token = bi;
            if (is_last) *is_last = b.last ? 1 : 0;
            return HHGT_OK;
        }
        // an empty block (e.g. only empty members): recycle it and look again
        r->free_.push_back(bi);
        r->cv_free.notify_all();
        if (b.last) return HHGT_OK;
    }
}

extern "C" int hhgt_reader_release(hhgt_reader *r, int token)
{
    if (!r || token < 0 || token >= r->n_blocks) return HHGT_ERR_ARG;
    std::lock_guard<std::mutex> lk(r->mu);
    if (!r->ring[token].held) return HHGT_ERR_ARG;
    r->ring[token].held = false;
    r->free_.push_back(token);
    r->cv_free.notify_all();
    return HHGT_OK;
}

extern "C" int hhgt_reader_next(hhgt_reader *r, const void **host_ptr, uint64_t *nbytes)
{
    if (!r || !host_ptr || !nbytes) return HHGT_ERR_ARG;
    if (r->auto_held >= 0) {
        hhgt_reader_release(r, r->auto_held);
        r->auto_held = -1;
    }
    int token = -1;
    const int rc = hhgt_reader_acquire(r, host_ptr, nbytes, &token, nullptr);
    if (rc == HHGT_OK) r->auto_held = token;
    return rc;
}

extern "C" int hhgt_reader_copy_async(hhgt_reader *r, const void *host_ptr, uint64_t nbytes, void *d_dst, void *stream)
{
    if (!r || !host_ptr || !d_dst) return HHGT_ERR_ARG;
    HIP_TRY(hipMemcpyAsync(d_dst, host_ptr, nbytes, hipMemcpyHostToDevice, reinterpret_cast<hipStream_t>(stream)));
    return HHGT_OK;
}

extern "C" int hhgt_reader_stats(const hhgt_reader *r, uint64_t *file_bytes, uint64_t *text_bytes)
{
    if (!r) return HHGT_ERR_ARG;
    if (file_bytes) *file_bytes = r->file_bytes.load();
    if (text_bytes) *text_bytes = r->text_bytes.load();
    return HHGT_OK;
}
