// api.hip — C ABI of libhhgt.so (see include/hhgt.h): context, orchestration of the kernel stages,
// error reporting.  No CPU fallback anywhere: every compute entry point needs a HIP device.
#include "common.h"
#include <chrono>
#include <vector>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

static thread_local char g_err[512] = "";

void hhgt_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *hhgt_last_error(void) { return g_err; }
extern "C" const char *hhgt_version(void) { return "hhgt 0.1 (gfx950)"; }

extern "C" int hhgt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int DevBuf::ensure(size_t bytes)
{
    if (bytes <= cap) return HHGT_OK;
    if (p) {
        hipFree(p);
        p = nullptr;
        cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256;
    static const bool dbg = getenv("HHGT_ALLOC_DEBUG") != nullptr;   // development aid: late allocations stall every stream
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc(&p, want);
    if (dbg)
        fprintf(stderr, "[alloc] %.3f ms  hipMalloc %zu took %.3f ms\n", std::chrono::duration<double>(t0.time_since_epoch()).count() * 1e3,
                want, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
    if (e != hipSuccess) {
        p = nullptr;
        hhgt_set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        return HHGT_ERR_HIP;
    }
    cap = want;
    return HHGT_OK;
}

void DevBuf::release()
{
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
}

#define TRY(expr)                      \
    do {                               \
        int _rc = (expr);              \
        if (_rc != HHGT_OK) return _rc; \
    } while (0)

int EncodeWs::ensure_index(uint32_t n_regions, hipStream_t st)
{
    TRY(slots.ensure((size_t)n_regions * INDEX_CAP * 4));
    TRY(counts.ensure((size_t)n_regions * 4));
    TRY(n_lines.ensure(4));
    const size_t had = region_tot.cap;
    TRY(region_tot.ensure((size_t)chain_groups(n_regions) * 4));
    if (region_tot.cap != had) HIP_TRY(hipMemsetAsync(region_tot.p, 0, region_tot.cap, st));   // new memory: zero once, in front of the index
    return HHGT_OK;
}

int EncodeWs::ensure_lines(uint32_t max_lines)
{
    const size_t nl4 = ((size_t)max_lines + 1) * 4;
    TRY(nl.ensure(nl4));
    for (DevBuf &b : line) TRY(b.ensure(nl4));
    TRY(line_tot.ensure(2 * (size_t)chain_groups(max_lines) * 4));
    if (chain_scanned(max_lines)) {
        for (DevBuf &b : scanned) TRY(b.ensure(nl4));
        TRY(scan_tmp.ensure(2 * scan_tmp_elems(max_lines) * 4));
    }
    return ensure_runs();
}

int EncodeWs::ensure_runs()
{
    TRY(run_first.ensure(MAX_CHROM_RUNS * 8));
    TRY(run_names.ensure(MAX_CHROM_RUNS * 32));
    return result.ensure(sizeof(hhgt_encode_result));
}

int hhgt_ctx::CodecWs::ensure(uint64_t n_chunks, uint32_t nblocks, uint32_t nwaves, size_t slot)
{
    const uint64_t n_streams = n_chunks * nblocks * nwaves;
    TRY(lz_scratch.ensure((size_t)n_streams * slot));
    TRY(lz_csize.ensure((size_t)n_streams * 4));
    TRY(fr_bsize.ensure((size_t)n_chunks * nblocks * 4));
    TRY(fr_csize.ensure(((size_t)n_chunks + 1) * 8));
    return fr_flags.ensure((size_t)n_chunks * 4);
}

// a launch under the timer of its stage
template <typename Launch>
static int timed(hhgt_ctx *c, hipStream_t st, int stage, Launch launch)
{
    StageTimer t(c, st, stage);
    TRY(launch());
    t.stop();
    return HHGT_OK;
}

// "<who>: null context", or "<who>: null <null_arg>" for the first null pointer among those the work needs (nullptr: none)
static int check_not_null(const char *who, const hhgt_ctx *c, const char *null_arg)
{
    if (c && !null_arg) return HHGT_OK;
    hhgt_set_error("%s: null %s", who, !c ? "context" : null_arg);
    return HHGT_ERR_ARG;
}

// what an entry does behind its checks: the stream, the device, nothing without work, then run(stream)
template <typename Run>
static int on_device(hhgt_ctx *c, void *stream, bool work, Run run)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    if (!work) return HHGT_OK;
    return run(st);
}

// the same for one launch under the timer of its stage
template <typename Launch>
static int launch_on_device(hhgt_ctx *c, void *stream, int stage, bool work, Launch launch)
{
    return on_device(c, stream, work, [&](hipStream_t st) { return timed(c, st, stage, [&] { return launch(st); }); });
}

extern "C" int hhgt_ctx_create(int device, hhgt_ctx **out)
{
    if (!out) return HHGT_ERR_ARG;
    *out = nullptr;
    int n = hhgt_device_count();
    if (n <= 0 || device < 0 || device >= n) {
        hhgt_set_error("no usable HIP device (count=%d, requested=%d): libhhgt has no CPU path", n, device);
        return HHGT_ERR_NO_DEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    hhgt_ctx *c = new hhgt_ctx();
    c->device = device;
    // from here on a failure must not leak the context (hhgt_ctx_destroy copes with a half-built one)
    int rc = HHGT_OK;
    hipError_t e = hipGetDeviceProperties(&c->prop, device);
    if (e != hipSuccess) {
        hhgt_set_error("hipGetDeviceProperties failed: %s", hipGetErrorString(e));
        rc = HHGT_ERR_HIP;
    } else if (strncmp(c->prop.gcnArchName, "gfx950", 6) != 0) {
        hhgt_set_error("device %d is %s; libhhgt carries gfx950 code objects only", device, c->prop.gcnArchName);
        rc = HHGT_ERR_NO_DEVICE;
    }
    if (rc == HHGT_OK && (e = hipHostMalloc(reinterpret_cast<void **>(&c->h_counters), sizeof(DevCounters), hipHostMallocDefault)) != hipSuccess) {
        hhgt_set_error("hipHostMalloc failed: %s", hipGetErrorString(e));
        rc = HHGT_ERR_HIP;
    }
    if (rc == HHGT_OK && (e = hipHostMalloc(reinterpret_cast<void **>(&c->h_result_pinned), sizeof(hhgt_encode_result), hipHostMallocDefault)) != hipSuccess) {
        hhgt_set_error("hipHostMalloc failed: %s", hipGetErrorString(e));
        rc = HHGT_ERR_HIP;
    }
    if (rc == HHGT_OK) rc = c->counters.ensure(sizeof(DevCounters));
    if (rc != HHGT_OK) {
        hhgt_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return HHGT_OK;
}

extern "C" void hhgt_ctx_destroy(hhgt_ctx *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    c->enc.each([](DevBuf &b) { b.release(); });
    DevBuf *bufs[] = {&c->counters, &c->cursor, &c->dec_bad, &c->oh_ovl, &c->oh_lut, &c->crc_x2n, &c->ld_bits, &c->score_part, &c->region_part,
                       &c->clump_ws};
    for (DevBuf *b : bufs) b->release();
    for (auto &w : c->cw) {
        DevBuf *wb[] = {&w.lz_scratch, &w.lz_csize, &w.lz_flags, &w.fr_bsize, &w.fr_csize, &w.fr_flags};
        for (DevBuf *b : wb) b->release();
        if (w.lz_done) hipEventDestroy(w.lz_done);
        if (w.fr_done) hipEventDestroy(w.fr_done);
    }
    if (c->h_counters) hipHostFree(c->h_counters);
    if (c->h_result_pinned) hipHostFree(c->h_result_pinned);
    for (auto &p : c->pending) {
        hipEventDestroy(p.a);
        hipEventDestroy(p.b);
    }
    for (auto e : c->event_pool) hipEventDestroy(e);
    delete c;
}

// ---- profiling ------------------------------------------------------------------------------------
static hipEvent_t get_event(hhgt_ctx *c)
{
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}

StageTimer::StageTimer(hhgt_ctx *c, hipStream_t s, int stage_) : ctx(c), st(s), stage(stage_)
{
    if (ctx->profiling) {
        a = get_event(ctx);
        b = get_event(ctx);
        hipEventRecord(a, st);
    }
}

void StageTimer::stop()
{
    if (a) {
        hipEventRecord(b, st);
        ctx->pending.push_back({stage, a, b});
        a = b = nullptr;
    }
}

int hhgt_profile_collect(hhgt_ctx *c)
{
    for (auto &p : c->pending) {
        hipEventSynchronize(p.b);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            c->stage_ms[p.stage] += ms;
            c->stage_launches[p.stage] += 1;
        }
        c->event_pool.push_back(p.a);
        c->event_pool.push_back(p.b);
    }
    c->pending.clear();
    return HHGT_OK;
}

extern "C" int hhgt_profile_enable(hhgt_ctx *c, int on)
{
    if (!c) return HHGT_ERR_ARG;
    c->profiling = on ? 1 : 0;
    return HHGT_OK;
}

extern "C" int hhgt_profile_reset(hhgt_ctx *c)
{
    if (!c) return HHGT_ERR_ARG;
    hhgt_profile_collect(c);
    for (int i = 0; i < HHGT_N_STAGES; ++i) {
        c->stage_ms[i] = 0;
        c->stage_launches[i] = 0;
    }
    return HHGT_OK;
}

extern "C" int hhgt_profile_read(hhgt_ctx *c, double *ms, uint64_t *launches)
{
    if (!c) return HHGT_ERR_ARG;
    hhgt_profile_collect(c);
    for (int i = 0; i < HHGT_N_STAGES; ++i) {
        if (ms) ms[i] = c->stage_ms[i];
        if (launches) launches[i] = c->stage_launches[i];
    }
    return HHGT_OK;
}

// ---- layout ---------------------------------------------------------------------------------------
static int make_layout(const hhgt_layout *lay, LayoutDev *L)
{
    if (!lay || lay->n_samples < 0) {
        hhgt_set_error("layout: bad n_samples");
        return HHGT_ERR_ARG;
    }
    L->S = (uint32_t)lay->n_samples;
    L->v_capacity = lay->v_capacity;
    L->ring = 0;
    L->pad_ = 0;
    if (lay->ring < 0 || (lay->ring > 0 && (lay->vc <= 0 || lay->v_capacity != (uint64_t)lay->ring * (uint64_t)lay->vc))) {
        hhgt_set_error("layout: a ring needs vc > 0 and v_capacity == ring * vc");
        return HHGT_ERR_ARG;
    }
    L->ring = (uint32_t)lay->ring;
    if (lay->vc == 0) {
        L->Vc = lay->v_capacity ? lay->v_capacity : TILE_V;
    } else {
        L->Vc = (uint64_t)lay->vc;
    }
    if (L->Vc % TILE_V) {
        hhgt_set_error("layout: variants per chunk (%llu) must be a multiple of %d (dense: v_capacity)",
                       (unsigned long long)L->Vc, TILE_V);
        return HHGT_ERR_ARG;
    }
    if (lay->v_capacity % L->Vc) {
        hhgt_set_error("layout: v_capacity must be a multiple of vc");
        return HHGT_ERR_ARG;
    }
    if (lay->sc == 0) {
        L->Sc = L->S ? L->S : 1;
        L->sc_log2 = 31;
        L->n_sc = 1;
    } else {
        uint32_t sc = (uint32_t)lay->sc;
        if (sc & (sc - 1)) {
            hhgt_set_error("layout: sc must be a power of two");
            return HHGT_ERR_ARG;
        }
        L->Sc = sc;
        uint32_t lg = 0;
        while ((1u << lg) < sc) ++lg;
        L->sc_log2 = lg;
        L->n_sc = (L->S + sc - 1) / sc;
        if (L->n_sc == 0) L->n_sc = 1;
    }
    return HHGT_OK;
}

extern "C" uint64_t hhgt_layout_bytes(const hhgt_layout *lay)
{
    LayoutDev L;
    if (make_layout(lay, &L) != HHGT_OK) return 0;
    return (uint64_t)L.n_sc * L.Sc * L.v_capacity * 2ull;
}

extern "C" uint64_t hhgt_layout_offset(const hhgt_layout *lay, uint32_t s, uint64_t v)
{
    LayoutDev L;
    if (make_layout(lay, &L) != HHGT_OK) return ~0ull;
    return layout_offset(L, s, v);
}

static int parse_region_host(const char *region, RegionFilter *rf)
{
    memset(rf, 0, sizeof(*rf));
    if (!region || !*region) return HHGT_OK;
    const char *colon = strrchr(region, ':');
    size_t clen = strlen(region);
    if (colon && colon[1] >= '0' && colon[1] <= '9') {
        char *p;
        long long b = strtoll(colon + 1, &p, 10), e = 0x7fffffffffffffffLL;
        while (*p == ',') p++;
        if (*p == '-' && p[1]) e = strtoll(p + 1, &p, 10);
        clen = (size_t)(colon - region);
        rf->has_range = 1;
        rf->beg = b;
        rf->end = e;
    }
    if (clen == 0 || clen >= sizeof(rf->contig)) {
        hhgt_set_error("region '%s': contig name empty or longer than 63 bytes", region);
        return HHGT_ERR_ARG;
    }
    memcpy(rf->contig, region, clen);
    rf->contig_len = (int)clen;
    return HHGT_OK;
}

// ---- encode ---------------------------------------------------------------------------------------
// device-side epilogue of one encode call: advance the cursor, assemble the result record (counts, CHROM runs).  `res` is
// the caller's record itself where the device can write it (pinned host memory: no staging copy behind this kernel), so
// `done` is stored last and with system-scope release: whoever sees it set sees the record.
__global__ void k_encode_finish(DevCounters *cnt, uint64_t *cursor, const uint64_t *__restrict__ run_first,
                                const uint8_t *__restrict__ run_names, uint64_t v_capacity, hhgt_encode_result *res,
                                uint32_t *region_tot, uint32_t n_region_tot)
{
    const uint32_t t = threadIdx.x;
    const uint64_t before = *cursor;
    const uint64_t kept = cnt->n_kept;
    __syncthreads();
    if (t == 0) {
        *cursor = before + kept;
        cnt->cursor_after = before + kept;
        res->stats.n_lines = cnt->n_lines;
        res->stats.n_records = cnt->n_records;
        res->stats.n_kept = kept;
        res->stats.n_drop_region = cnt->n_drop_region;
        res->stats.n_drop_filter = cnt->n_drop_filter;
        res->stats.n_haploid_padded = cnt->n_haploid;
        res->stats.n_malformed = cnt->n_malformed;
        res->stats.n_general_lines = cnt->n_general;
        res->stats.n_chrom_runs = cnt->n_chrom_runs;
        res->cursor_before = before;
        res->cursor_after = before + kept;
        res->n_lines_over = cnt->err_lines;
        res->err_density = cnt->err_density;
        res->v_capacity = v_capacity;
        res->reserved = cnt->n_other > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cnt->n_other;   // bit-plane form: calls beyond 0 / 1 / missing
    }
    const uint64_t n_runs = cnt->n_chrom_runs;
    if (t < HHGT_RESULT_RUNS) res->run_first[t] = t < n_runs ? run_first[t] : 0ull;
    for (uint32_t q = t; q < HHGT_RESULT_RUNS * 32u; q += blockDim.x)
        res->run_names[q >> 5][q & 31u] = (q >> 5) < n_runs ? (char)run_names[q] : 0;
    __threadfence_system();
    // the counters and the index's region totals go back to zero for the next call on this context (one memset launch less
    // per call: counters_clean)
    __syncthreads();
    if (t == 0) __hip_atomic_store(&res->done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (t < sizeof(DevCounters) / 8u) reinterpret_cast<unsigned long long *>(cnt)[t] = 0ull;
    for (uint32_t q = t; q < n_region_tot; q += blockDim.x) region_tot[q] = 0u;
}

__global__ void k_set_u64(uint64_t *p, uint64_t v) { *p = v; }

static int encode_check_args(hhgt_ctx *c, const void *d_text, uint64_t nbytes, const hhgt_layout *lay, LayoutDev *L,
                             const char *region, RegionFilter *rf, void *d_G)
{
    TRY(make_layout(lay, L));
    if (nbytes >= 0xFFFFFFF0ull) {
        hhgt_set_error("encode: text block of %llu bytes; split it below 4 GiB at a line boundary",
                       (unsigned long long)nbytes);
        return HHGT_ERR_ARG;
    }
    if (nbytes && (!d_text || (reinterpret_cast<uintptr_t>(d_text) & 15u))) {
        hhgt_set_error("encode: d_text must be a 16-byte aligned device pointer");
        return HHGT_ERR_ARG;
    }
    if (L->S > 0 && !d_G) {
        hhgt_set_error("encode: d_G is NULL");
        return HHGT_ERR_ARG;
    }
    const int rc = parse_region_host(region, rf);
    rf->keep_multi = c->keep_multi;
    return rc;
}

// regions of the newline index over a text block (and the byte behind it)
static uint32_t index_regions(uint64_t nbytes) { return (uint32_t)((nbytes + 1 + INDEX_REGION - 1) / INDEX_REGION); }

// the DevCounters and the index's region totals are zero when a call starts: the epilogue of the last call left them so
// (counters_clean); behind a call that did not get that far, zero them here
static int encode_begin_clean(hhgt_ctx *c, DevCounters *cnt, hipStream_t st)
{
    if (!c->counters_clean) {
        HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(DevCounters), st));
        if (c->enc.region_tot.p) HIP_TRY(hipMemsetAsync(c->enc.region_tot.p, 0, c->enc.region_tot.cap, st));
    }
    c->counters_clean = false;
    return HHGT_OK;
}

// stage 1: newline index of the block -> slots / counts per region and the totals per CHAIN_GROUP regions, whose sum is the
// line count (k_compact_newlines puts it into enc.n_lines).  min_line: a record with S sample columns cannot be shorter
// than 9 fixed columns and S fields of one byte and a separator each (0: unknown)
static int encode_stage_index(hhgt_ctx *c, const uint8_t *text, uint64_t nbytes, uint32_t n_regions, uint32_t min_line, uint32_t S,
                              DevCounters *cnt, hipStream_t st)
{
    EncodeWs &w = c->enc;
    TRY(w.ensure_index(n_regions, st));
    return launch_index_newlines(text, nbytes, w.slots.as<uint32_t>(), w.counts.as<uint32_t>(), w.region_tot.as<uint32_t>(), n_regions,
                                 min_line, S, c->index_mode, cnt, st);
}

// stages 2..: everything behind the index, sized by max_lines, counts and append position read on the device
static int encode_stage_rest(hhgt_ctx *c, const uint8_t *text, uint64_t nbytes, uint32_t n_regions, uint32_t max_lines,
                             const RegionFilter &rf, const LayoutDev &L, const uint64_t *d_cursor, void *d_G, void *d_P, uint32_t *d_start, uint32_t *d_stop,
                             uint8_t *d_ref, uint8_t *d_alt, DevCounters *cnt, hipStream_t st)
{
    EncodeWs &w = c->enc;
    TRY(w.ensure_lines(max_lines));
    const uint32_t *nl = w.nl.as<uint32_t>(), *d_nlines = w.n_lines.as<uint32_t>();
    const LineCols l = w.line_cols(max_lines);
    const KeptCols k = w.kept_cols();
    TRY(timed(c, st, HHGT_STAGE_INDEX, [&] {
        return launch_compact_newlines(w.slots.as<uint32_t>(), w.counts.as<uint32_t>(), w.region_tot.as<uint32_t>(), n_regions,
                                       w.nl.as<uint32_t>(), max_lines, w.n_lines.as<uint32_t>(), st);
    }));
    if (max_lines == 0) return HHGT_OK;
    TRY(timed(c, st, HHGT_STAGE_FIXED, [&] {
        TRY(launch_parse_fixed(text, nbytes, nl, d_nlines, max_lines, rf, L.S, l, c->index_mode, cnt, st));
        if (chain_scanned(max_lines))   // more lines than k_compact_kept sums totals for: kidx / crun from the scan launches
            TRY(launch_scan_exclusive_u32_pair(l.keep, l.kidx, l.cnew, l.crun, max_lines, w.scan_tmp.as<uint32_t>(), w.scan_tmp.cap / 4, st));
        return launch_compact_kept(text, nbytes, nl, d_nlines, max_lines, l, k, MAX_CHROM_RUNS, d_cursor, L.v_capacity, L.ring,
                                   d_start, d_stop, d_ref, d_alt, cnt, d_P != nullptr, st);
    }));
    if (L.S == 0) return HHGT_OK;
    TRY(timed(c, st, HHGT_STAGE_ENCODE, [&] {
        return d_P ? launch_encode_planes(text, nbytes, k.soff, k.meta, max_lines, d_cursor, L, static_cast<uint8_t *>(d_P),
                                          static_cast<int8_t *>(d_G), k.redo_list, k.redo_flag, cnt, st)
                   : launch_encode_tiles(text, nbytes, k.soff, k.meta, max_lines, d_cursor, L, static_cast<int8_t *>(d_G),
                                         k.redo_list, k.redo_flag, cnt, st);
    }));
    return timed(c, st, HHGT_STAGE_GENERAL, [&] {
        return launch_encode_general(text, nbytes, k.soff, k.lend, k.meta, k.redo_list, d_cursor, L, static_cast<int8_t *>(d_G),
                                     static_cast<uint8_t *>(d_P), cnt, c->prop.multiProcessorCount, st);
    });
}

// the address under which this context's device writes *h_result itself: pinned host memory (hipHostMalloc, hipHostRegister)
// made on its device.  nullptr: anything else (pageable memory, or unknown to the runtime) goes through staging and a copy
static hhgt_encode_result *result_on_device(const hhgt_ctx *c, hhgt_encode_result *h_result)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, h_result) != hipSuccess) {
        (void)hipGetLastError();   // (not an error of the call: the runtime does not know the pointer)
        return nullptr;
    }
    if (a.type != hipMemoryTypeHost || !a.devicePointer || a.device != c->device) return nullptr;
    return static_cast<hhgt_encode_result *>(a.devicePointer);
}

// epilogue of a call over n_regions index regions; h_result (may be NULL) receives the record when the stream gets there
static int encode_finish(hhgt_ctx *c, uint64_t *d_cursor, const LayoutDev &L, DevCounters *cnt, uint32_t n_regions,
                         hhgt_encode_result *h_result, hipStream_t st)
{
    TRY(c->enc.ensure_runs());
    const KeptCols k = c->enc.kept_cols();
    hhgt_encode_result *staging = c->enc.result.as<hhgt_encode_result>();
    hhgt_encode_result *direct = h_result ? result_on_device(c, h_result) : nullptr;
    if (h_result) h_result->done = 0u;
    hipLaunchKernelGGL(k_encode_finish, dim3(1), dim3(256), 0, st, cnt, d_cursor, k.run_first, k.run_names,
                       L.ring ? 0ull : L.v_capacity, direct ? direct : staging, c->enc.region_tot.as<uint32_t>(),
                       c->enc.region_tot.p ? chain_groups(n_regions) : 0u);
    HIP_TRY(hipGetLastError());
    c->counters_clean = true;   // (calls on one context are serialised by the caller: the next one is queued behind this epilogue)
    if (h_result && !direct) HIP_TRY(hipMemcpyAsync(h_result, staging, sizeof(hhgt_encode_result), hipMemcpyDeviceToHost, st));
    return HHGT_OK;
}

extern "C" int hhgt_encode_result_status(const hhgt_encode_result *r)
{
    if (!r) return HHGT_ERR_ARG;
    if (!r->done) {
        hhgt_set_error("encode: the result record is not complete yet (synchronise the stream first)");
        return HHGT_ERR_ARG;
    }
    if (r->err_density) {
        hhgt_set_error("encode: more than %u newlines inside one %u-byte region (not VCF text)", INDEX_CAP, INDEX_REGION);
        return HHGT_ERR_LINE_DENSITY;
    }
    if (r->n_lines_over) {
        hhgt_set_error("encode: %llu lines beyond max_lines were not encoded", (unsigned long long)r->n_lines_over);
        return HHGT_ERR_CAPACITY;
    }
    if (r->stats.n_malformed) {
        hhgt_set_error("Error parsing VCF file: %llu malformed record(s) (too few columns, bad POS, FORMAT without GT)",
                       (unsigned long long)r->stats.n_malformed);
        return HHGT_ERR_MALFORMED;
    }
    if (r->v_capacity && r->cursor_after > r->v_capacity) {
        hhgt_set_error("encode: %llu kept records at v_base %llu exceed v_capacity %llu",
                       (unsigned long long)r->stats.n_kept, (unsigned long long)r->cursor_before,
                       (unsigned long long)r->v_capacity);
        return HHGT_ERR_CAPACITY;
    }
    if (r->stats.n_chrom_runs > MAX_CHROM_RUNS) {
        hhgt_set_error("encode: %llu CHROM runs in one text block, more than the limit of %u (a run starts at every change of CHROM "
                       "and behind every empty or header line)",
                       (unsigned long long)r->stats.n_chrom_runs, MAX_CHROM_RUNS);
        return HHGT_ERR_CAPACITY;
    }
    return HHGT_OK;
}

static void empty_result(hhgt_encode_result *r)
{
    memset(r, 0, sizeof(*r));
    r->done = 1u;
}

// a layout can carry bit planes when a Blosc block (4096 variants of one sample) never crosses a chunk column
static int planes_check_layout(const LayoutDev &L)
{
    if (L.Vc % 4096ull) {
        hhgt_set_error("planes: variants per chunk (%llu; dense: v_capacity) must be a multiple of 4096", (unsigned long long)L.Vc);
        return HHGT_ERR_ARG;
    }
    return HHGT_OK;
}

extern "C" uint64_t hhgt_planes_bytes(const hhgt_layout *lay)
{
    LayoutDev L;
    if (make_layout(lay, &L) != HHGT_OK || planes_check_layout(L) != HHGT_OK) return 0;
    return (uint64_t)L.n_sc * L.Sc * L.v_capacity / 2ull;
}

// columns [col0, col0 + n_cols) of a plane buffer: checks and geometry shared by compress and expand
static int planes_columns(const hhgt_layout *lay, uint32_t col0, uint32_t n_cols, LayoutDev *L, PlanesGeom *pg)
{
    TRY(make_layout(lay, L));
    TRY(planes_check_layout(*L));
    if ((uint64_t)col0 + n_cols > L->v_capacity / L->Vc) {
        hhgt_set_error("planes: columns [%u, %u) outside the layout's %llu", col0, col0 + n_cols, (unsigned long long)(L->v_capacity / L->Vc));
        return HHGT_ERR_ARG;
    }
    *pg = planes_geom(*L, col0);
    return HHGT_OK;
}

// what the four pad_tail entry points begin with: the null checks (the cursor forms add theirs), the device, the layout (planes: one that carries them)
static int pad_tail_begin(hhgt_ctx *c, const void *d_buf, const hhgt_layout *lay, bool planes, LayoutDev *L)
{
    if (!c || !d_buf) return HHGT_ERR_ARG;
    HIP_TRY(hipSetDevice(c->device));
    TRY(make_layout(lay, L));
    return planes ? planes_check_layout(*L) : HHGT_OK;
}

// the range form: v_end and the columns lie inside the layout
static int pad_tail_range(const LayoutDev &L, uint64_t v_end, uint64_t vcol_end)
{
    if (v_end > L.v_capacity || vcol_end > L.v_capacity / L.Vc) {
        hhgt_set_error("pad_tail: range outside the layout");
        return HHGT_ERR_ARG;
    }
    return HHGT_OK;
}

static int encode_async_impl(hhgt_ctx *c, const void *d_text, uint64_t nbytes, const char *region, const hhgt_layout *lay,
                             uint64_t *d_cursor, uint32_t max_lines, void *d_G, void *d_P, bool planes, uint32_t *d_start,
                             uint32_t *d_stop, uint8_t *d_ref, uint8_t *d_alt, hhgt_encode_result *h_result, void *stream)
{
    if (!c || !d_cursor) return HHGT_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    LayoutDev L;
    RegionFilter rf;
    TRY(encode_check_args(c, d_text, nbytes, lay, &L, region, &rf, planes ? d_P : d_G));
    if (planes) TRY(planes_check_layout(L));
    const uint8_t *text = static_cast<const uint8_t *>(d_text);
    DevCounters *cnt = c->counters.as<DevCounters>();
    TRY(encode_begin_clean(c, cnt, st));
    const uint32_t n_regions = index_regions(nbytes);
    if (nbytes) {
        TRY(timed(c, st, HHGT_STAGE_INDEX, [&] { return encode_stage_index(c, text, nbytes, n_regions, L.S ? 2u * L.S + 17u : 0u, L.S, cnt, st); }));
        TRY(encode_stage_rest(c, text, nbytes, n_regions, max_lines, rf, L, d_cursor, d_G, planes ? d_P : nullptr, d_start, d_stop, d_ref,
                              d_alt, cnt, st));
    }
    return encode_finish(c, d_cursor, L, cnt, n_regions, h_result, st);
}

extern "C" int hhgt_encode_text_async(hhgt_ctx *c, const void *d_text, uint64_t nbytes, const char *region,
                                      const hhgt_layout *lay, uint64_t *d_cursor, uint32_t max_lines, void *d_G,
                                      uint32_t *d_start, uint32_t *d_stop, uint8_t *d_ref, uint8_t *d_alt,
                                      hhgt_encode_result *h_result, void *stream)
{
    return encode_async_impl(c, d_text, nbytes, region, lay, d_cursor, max_lines, d_G, nullptr, false, d_start, d_stop, d_ref, d_alt,
                             h_result, stream);
}

extern "C" int hhgt_encode_text_planes_async(hhgt_ctx *c, const void *d_text, uint64_t nbytes, const char *region,
                                             const hhgt_layout *lay, uint64_t *d_cursor, uint32_t max_lines, void *d_P, void *d_G,
                                             uint32_t *d_start, uint32_t *d_stop, uint8_t *d_ref, uint8_t *d_alt,
                                             hhgt_encode_result *h_result, void *stream)
{
    return encode_async_impl(c, d_text, nbytes, region, lay, d_cursor, max_lines, d_G, d_P, true, d_start, d_stop, d_ref, d_alt,
                             h_result, stream);
}

extern "C" int hhgt_pad_tail_planes(hhgt_ctx *c, const hhgt_layout *lay, uint64_t v_end, uint64_t vcol_begin, uint64_t vcol_end,
                                    void *d_P, void *stream)
{
    LayoutDev L;
    TRY(pad_tail_begin(c, d_P, lay, true, &L));
    TRY(pad_tail_range(L, v_end, vcol_end));
    return launch_pad_tail_planes(L, v_end, vcol_begin, vcol_end, static_cast<uint8_t *>(d_P), reinterpret_cast<hipStream_t>(stream));
}

extern "C" int hhgt_pad_tail_planes_cursor(hhgt_ctx *c, const hhgt_layout *lay, const uint64_t *d_cursor, void *d_P, void *stream)
{
    LayoutDev L;
    if (!d_cursor) return HHGT_ERR_ARG;
    TRY(pad_tail_begin(c, d_P, lay, true, &L));
    return launch_pad_tail_planes_cursor(L, d_cursor, static_cast<uint8_t *>(d_P), reinterpret_cast<hipStream_t>(stream));
}

extern "C" int hhgt_planes_expand(hhgt_ctx *c, const hhgt_layout *lay, const void *d_P, const void *d_G, uint32_t col0, uint32_t n_cols,
                                  void *d_out, void *stream)
{
    if (!c || !d_P || !d_out) return HHGT_ERR_ARG;
    HIP_TRY(hipSetDevice(c->device));
    LayoutDev L;
    PlanesGeom pg;
    TRY(planes_columns(lay, col0, n_cols, &L, &pg));
    if (n_cols == 0) return HHGT_OK;
    return launch_planes_expand(L, static_cast<const uint8_t *>(d_P), static_cast<const uint8_t *>(d_G), col0, n_cols,
                                static_cast<uint8_t *>(d_out), reinterpret_cast<hipStream_t>(stream));
}

static int encode_text_once(hhgt_ctx *c, const void *d_text, uint64_t nbytes, const char *region, const hhgt_layout *lay, uint64_t v_base,
                            void *d_G, uint32_t *d_start, uint32_t *d_stop, uint8_t *d_ref, uint8_t *d_alt, hhgt_encode_stats *stats,
                            void *stream);

// The synchronous form decodes whatever the plain scan decodes: when the call comes back MALFORMED and the line index of long
// records skipped bytes (hop / walk, S >= 760), the reason may be a newline in the part it did not look at — a record shorter
// than its S samples that is valid VCF all the same (rows of empty columns; one haploid call + one two-digit allele in front of
// an empty line: DESIGN.md 4).  Then the call runs once more with every byte scanned (mode 0) and THAT outcome stands: an
// error only where the scan errs too.  Costs nothing unless the first pass fails.  (The asynchronous form reports the first
// pass's error — its callers have queued more work behind it.)
extern "C" int hhgt_encode_text(hhgt_ctx *c, const void *d_text, uint64_t nbytes, const char *region,
                                const hhgt_layout *lay, uint64_t v_base, void *d_G, uint32_t *d_start,
                                uint32_t *d_stop, uint8_t *d_ref, uint8_t *d_alt, hhgt_encode_stats *stats,
                                void *stream)
{
    int rc = encode_text_once(c, d_text, nbytes, region, lay, v_base, d_G, d_start, d_stop, d_ref, d_alt, stats, stream);
    if (rc == HHGT_ERR_MALFORMED && c && lay && lay->n_samples >= 760) {
        const int mode = c->index_mode < 0 ? index_mode_default() : c->index_mode;
        if (mode > 0) {
            const int saved = c->index_mode;
            c->index_mode = 0;
            rc = encode_text_once(c, d_text, nbytes, region, lay, v_base, d_G, d_start, d_stop, d_ref, d_alt, stats, stream);
            c->index_mode = saved;
        }
    }
    return rc;
}

static int encode_text_once(hhgt_ctx *c, const void *d_text, uint64_t nbytes, const char *region, const hhgt_layout *lay, uint64_t v_base,
                            void *d_G, uint32_t *d_start, uint32_t *d_stop, uint8_t *d_ref, uint8_t *d_alt, hhgt_encode_stats *stats,
                            void *stream)
{
    if (!c) return HHGT_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    if (stats) memset(stats, 0, sizeof(*stats));
    LayoutDev L;
    RegionFilter rf;
    TRY(encode_check_args(c, d_text, nbytes, lay, &L, region, &rf, d_G));
    c->run_first_kept.clear();
    c->run_names_host.clear();
    if (nbytes == 0) return HHGT_OK;

    const uint8_t *text = static_cast<const uint8_t *>(d_text);
    DevCounters *cnt = c->counters.as<DevCounters>();
    TRY(c->cursor.ensure(8));
    TRY(encode_begin_clean(c, cnt, st));
    hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, st, c->cursor.as<uint64_t>(), v_base);
    const uint32_t n_regions = index_regions(nbytes);
    uint32_t n_lines = 0;
    {
        // the synchronous form sizes everything by the exact line count: the index's totals (at most 1024 words) are read
        // back once and added up (any input, however short its lines, fits), where the asynchronous form takes the
        // caller's bound
        StageTimer t(c, st, HHGT_STAGE_INDEX);
        TRY(encode_stage_index(c, text, nbytes, n_regions, L.S ? 2u * L.S + 17u : 0u, L.S, cnt, st));
        std::vector<uint32_t> totals(chain_groups(n_regions));
        c->h_counters->err_density = 0;
        HIP_TRY(hipMemcpyAsync(totals.data(), c->enc.region_tot.p, totals.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&c->h_counters->err_density, &cnt->err_density, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        t.stop();
        for (uint32_t x : totals) n_lines += x;
        if (c->h_counters->err_density) {
            hhgt_set_error("encode: more than %u newlines inside one %u-byte region (not VCF text)", INDEX_CAP,
                           INDEX_REGION);
            return HHGT_ERR_LINE_DENSITY;
        }
    }
    if (stats) stats->n_lines = n_lines;
    if (n_lines == 0) return HHGT_OK;
    TRY(encode_stage_rest(c, text, nbytes, n_regions, n_lines, rf, L, c->cursor.as<uint64_t>(), d_G, nullptr, d_start, d_stop, d_ref,
                          d_alt, cnt, st));
    TRY(encode_finish(c, c->cursor.as<uint64_t>(), L, cnt, n_regions, c->h_result_pinned, st));
    hhgt_encode_result *hr = &c->h_result;
    HIP_TRY(hipStreamSynchronize(st));
    *hr = *c->h_result_pinned;
    if (stats) *stats = hr->stats;
    TRY(hhgt_encode_result_status(hr));
    // CHROM runs: names were copied out of the text by the compaction kernel
    const uint32_t n_runs = (uint32_t)hr->stats.n_chrom_runs;
    if (n_runs) {
        std::vector<uint64_t> first(n_runs);
        std::vector<char> names((size_t)n_runs * 32);
        if (n_runs <= HHGT_RESULT_RUNS) {
            memcpy(first.data(), hr->run_first, n_runs * 8);
            memcpy(names.data(), hr->run_names, (size_t)n_runs * 32);
        } else {
            HIP_TRY(hipMemcpy(first.data(), c->enc.run_first.p, (size_t)n_runs * 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(names.data(), c->enc.run_names.p, (size_t)n_runs * 32, hipMemcpyDeviceToHost));
        }
        for (uint32_t r = 0; r < n_runs; ++r) {
            c->run_first_kept.push_back(first[r]);
            c->run_names_host.emplace_back(names.data() + (size_t)r * 32, strnlen(names.data() + (size_t)r * 32, 31));
        }
    }
    return HHGT_OK;
}

extern "C" int hhgt_encode_chrom_runs(hhgt_ctx *c, uint32_t max_runs, uint64_t *first_kept, char *names,
                                      uint32_t *n_runs)
{
    if (!c || !n_runs) return HHGT_ERR_ARG;
    uint32_t n = (uint32_t)c->run_first_kept.size();
    *n_runs = n;
    if (n > max_runs) n = max_runs;
    for (uint32_t r = 0; r < n; ++r) {
        if (first_kept) first_kept[r] = c->run_first_kept[r];
        if (names) {
            memset(names + (size_t)r * 32, 0, 32);
            size_t l = c->run_names_host[r].size() < 31 ? c->run_names_host[r].size() : 31;
            memcpy(names + (size_t)r * 32, c->run_names_host[r].data(), l);
        }
    }
    return HHGT_OK;
}

extern "C" int hhgt_pad_tail(hhgt_ctx *c, const hhgt_layout *lay, uint64_t v_end, uint64_t vcol_begin,
                             uint64_t vcol_end, void *d_G, void *stream)
{
    LayoutDev L;
    TRY(pad_tail_begin(c, d_G, lay, false, &L));
    TRY(pad_tail_range(L, v_end, vcol_end));
    return launch_pad_tail(L, v_end, vcol_begin, vcol_end, static_cast<int8_t *>(d_G),
                           reinterpret_cast<hipStream_t>(stream));
}

extern "C" int hhgt_pad_tail_cursor(hhgt_ctx *c, const hhgt_layout *lay, const uint64_t *d_cursor, void *d_G, void *stream)
{
    LayoutDev L;
    if (!d_cursor) return HHGT_ERR_ARG;
    TRY(pad_tail_begin(c, d_G, lay, false, &L));
    return launch_pad_tail_cursor(L, d_cursor, static_cast<int8_t *>(d_G), reinterpret_cast<hipStream_t>(stream));
}

// ---- compress -------------------------------------------------------------------------------------
static int check_codec_args(uint64_t chunk_nbytes, int typesize, int blocksize, int format)
{
    if (typesize < 1 || typesize > 255 || blocksize < 16 || blocksize > 65536 || blocksize % typesize ||
        chunk_nbytes == 0 || chunk_nbytes >= 0x7fffffffull || (format != HHGT_BLOSC1 && format != HHGT_BLOSC2)) {
        hhgt_set_error("compress: bad arguments (chunk_nbytes=%llu typesize=%d blocksize=%d format=%d)",
                       (unsigned long long)chunk_nbytes, typesize, blocksize, format);
        return HHGT_ERR_ARG;
    }
    return HHGT_OK;
}

// c-blosc never writes a blocksize larger than the chunk (its decoder rejects such headers)
static int effective_blocksize(uint64_t chunk_nbytes, int typesize, int blocksize)
{
    if ((uint64_t)blocksize > chunk_nbytes) {
        blocksize = (int)chunk_nbytes;
        if (typesize > 1 && blocksize >= typesize) blocksize -= blocksize % typesize;
    }
    return blocksize > 0 ? blocksize : 1;
}

// the decoders hold a whole Blosc block in LDS: blocks of at most 64 KiB (c-blosc's automatic blocksizes are larger)
static int check_decode_block(int typesize, int blocksize)
{
    if (blocksize > 65536) {
        hhgt_set_error("decode: block of %d bytes x typesize %d does not fit LDS (blocks of at most 65536 bytes)",
                       blocksize, typesize);
        return HHGT_ERR_ARG;
    }
    return HHGT_OK;
}

static void codec_geometry(uint64_t chunk_nbytes, int typesize, int blocksize, uint32_t *nblocks, uint32_t *nwaves,
                           size_t *slot_bytes)
{
    const bool split = typesize >= 2 && typesize <= 16 && blocksize / typesize >= 128;
    *nblocks = (uint32_t)((chunk_nbytes + blocksize - 1) / blocksize);
    *nwaves = split ? (uint32_t)typesize : 1u;
    size_t max_stream = split ? (size_t)blocksize / typesize : (size_t)blocksize;
    if (split && chunk_nbytes % blocksize && chunk_nbytes % blocksize > max_stream) max_stream = chunk_nbytes % blocksize;
    *slot_bytes = lz4_slot_bytes((int)max_stream);
}

extern "C" uint64_t hhgt_compress_bound(uint64_t n_chunks, uint64_t chunk_nbytes, int typesize, int blocksize)
{
    if (check_codec_args(chunk_nbytes, typesize, blocksize, HHGT_BLOSC2) != HHGT_OK) return 0;
    // a chunk never exceeds nbytes + 32 (memcpyed form)
    return n_chunks * (chunk_nbytes + 32);
}

// shuffle + LZ4 + framing of n_chunks chunks that exist as int8 bytes (d_src) or as bit planes (d_planes; d_src then only
// holds the bytes of calls beyond 0 / 1 / missing and may be NULL)
static int compress_impl(hhgt_ctx *c, const void *d_src, const void *d_planes, PlanesGeom pg, uint64_t n_chunks, uint64_t chunk_nbytes,
                         int typesize, int blocksize, int format, void *d_dst, uint64_t dst_cap,
                         uint64_t *d_chunk_off, uint64_t *total_bytes, void *stream)
{
    if (!c || (!d_src && !d_planes) || !d_dst || !d_chunk_off) return HHGT_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    TRY(check_codec_args(chunk_nbytes, typesize, blocksize, format));
    if (total_bytes) *total_bytes = 0;
    if (n_chunks == 0) return HHGT_OK;
    if (!total_bytes && dst_cap < n_chunks * (chunk_nbytes + 32)) {
        // without the read-back an overflow could not be reported: chunks that do not fit would silently be missing
        hhgt_set_error("compress: the asynchronous form (total_bytes == NULL) needs dst_cap >= hhgt_compress_bound() = %llu, got %llu",
                       (unsigned long long)(n_chunks * (chunk_nbytes + 32)), (unsigned long long)dst_cap);
        return HHGT_ERR_CAPACITY;
    }
    blocksize = effective_blocksize(chunk_nbytes, typesize, blocksize);
    uint32_t nblocks, nwaves;
    size_t slot;
    codec_geometry(chunk_nbytes, typesize, blocksize, &nblocks, &nwaves, &slot);
    // With a frame stream the framing of this call runs there, behind the LZ4 kernels, while the caller's stream is free
    // for the LZ4 kernels of the next call — which write the other workspace set, and wait for the framing that last read it.
    hipStream_t fst = c->frame_stream ? c->frame_stream : st;
    hhgt_ctx::CodecWs &w = c->cw[c->frame_stream ? (c->cmp_seq++ & 1u) : 0u];
    TRY(w.ensure(n_chunks, nblocks, nwaves, slot));
    if (w.fr_pending) {
        HIP_TRY(hipStreamWaitEvent(st, w.fr_done, 0));
        w.fr_pending = false;
    }
    TRY(timed(c, st, HHGT_STAGE_LZ4, [&] {
        if (!w.lz_flags.p) {
            TRY(w.lz_flags.ensure(4));
            HIP_TRY(hipMemsetAsync(w.lz_flags.p, 0, 4, st));
        }
        if (++w.lz_tag == 0) w.lz_tag = 1;
        return launch_lz4_blocks(static_cast<const uint8_t *>(d_src), static_cast<const uint8_t *>(d_planes), pg, n_chunks, chunk_nbytes,
                                 typesize, blocksize, w.lz_scratch.as<uint8_t>(), slot, w.lz_csize.as<uint32_t>(), c->clevel,
                                 w.lz_flags.as<uint32_t>(), w.lz_tag, st);
    }));
    if (fst != st) {
        if (!w.lz_done) HIP_TRY(hipEventCreateWithFlags(&w.lz_done, hipEventDisableTiming));
        if (!w.fr_done) HIP_TRY(hipEventCreateWithFlags(&w.fr_done, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(w.lz_done, st));
        HIP_TRY(hipStreamWaitEvent(fst, w.lz_done, 0));
    }
    TRY(timed(c, fst, HHGT_STAGE_FRAME, [&] {
        return launch_frame(w.lz_scratch.as<uint8_t>(), slot, w.lz_csize.as<uint32_t>(), static_cast<const uint8_t *>(d_src),
                            static_cast<const uint8_t *>(d_planes), pg, n_chunks, chunk_nbytes, typesize, blocksize, format,
                            w.fr_bsize.as<uint32_t>(), w.fr_csize.as<uint64_t>(), static_cast<uint8_t *>(d_dst), dst_cap, d_chunk_off,
                            w.fr_flags.as<uint32_t>(), fst);
    }));
    if (fst != st) {
        HIP_TRY(hipEventRecord(w.fr_done, fst));
        w.fr_pending = true;
        if (total_bytes) HIP_TRY(hipStreamWaitEvent(st, w.fr_done, 0));   // the synchronous form: the caller's stream sees the chunks
    }
    if (total_bytes) {
        uint64_t tot = 0;
        HIP_TRY(hipMemcpyAsync(&tot, d_chunk_off + n_chunks, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *total_bytes = tot;
        if (tot > dst_cap) {
            hhgt_set_error("compress: need %llu bytes, dst_cap is %llu", (unsigned long long)tot,
                           (unsigned long long)dst_cap);
            return HHGT_ERR_CAPACITY;
        }
    }
    return HHGT_OK;
}

extern "C" int hhgt_compress_chunks(hhgt_ctx *c, const void *d_src, uint64_t n_chunks, uint64_t chunk_nbytes,
                                    int typesize, int blocksize, int format, void *d_dst, uint64_t dst_cap,
                                    uint64_t *d_chunk_off, uint64_t *total_bytes, void *stream)
{
    if (!d_src) return HHGT_ERR_ARG;
    return compress_impl(c, d_src, nullptr, PlanesGeom{0, 0, 0, 0}, n_chunks, chunk_nbytes, typesize, blocksize, format, d_dst, dst_cap,
                         d_chunk_off, total_bytes, stream);
}

extern "C" int hhgt_compress_planes(hhgt_ctx *c, const hhgt_layout *lay, const void *d_P, const void *d_G, uint32_t col0, uint32_t n_cols,
                                    int format, void *d_dst, uint64_t dst_cap, uint64_t *d_chunk_off, uint64_t *total_bytes,
                                    void *stream)
{
    if (!c || !d_P) return HHGT_ERR_ARG;
    LayoutDev L;
    PlanesGeom pg;
    TRY(planes_columns(lay, col0, n_cols, &L, &pg));
    const uint64_t chunk_nbytes = (uint64_t)L.Sc * L.Vc * 2ull, col_bytes = chunk_nbytes * L.n_sc;
    // the chunks of columns col0.. in the int8 matrix (it only backs the calls beyond 0 / 1 / missing)
    const uint8_t *g = d_G ? static_cast<const uint8_t *>(d_G) + (uint64_t)col0 * col_bytes : nullptr;
    return compress_impl(c, g, d_P, pg, (uint64_t)n_cols * L.n_sc, chunk_nbytes, 2, 8192, format, d_dst, dst_cap, d_chunk_off, total_bytes,
                         stream);
}

// Workspaces of the context made ahead of time for calls of a known size (they otherwise grow inside the first calls: hipMalloc
// of hundreds of MB each, in the middle of a pipeline's first pass).  text_bytes / max_lines: the largest encode call to come;
// n_chunks x chunk_nbytes (typesize, blocksize): the largest compress call.  Either half may be 0.
extern "C" int hhgt_reserve(hhgt_ctx *c, uint64_t text_bytes, uint32_t max_lines, uint64_t n_chunks, uint64_t chunk_nbytes, int typesize,
                            int blocksize)
{
    if (!c) return HHGT_ERR_ARG;
    HIP_TRY(hipSetDevice(c->device));
    if (text_bytes) {
        const uint32_t n_regions = index_regions(text_bytes);
        TRY(c->enc.ensure_index(n_regions, nullptr));
        TRY(c->enc.ensure_lines(max_lines));
        HIP_TRY(hipStreamSynchronize(nullptr));   // (new region totals are zeroed on the null stream: done before any call's stream runs)
    }
    if (n_chunks) {
        TRY(check_codec_args(chunk_nbytes, typesize, blocksize, HHGT_BLOSC2));
        blocksize = effective_blocksize(chunk_nbytes, typesize, blocksize);
        uint32_t nblocks, nwaves;
        size_t slot;
        codec_geometry(chunk_nbytes, typesize, blocksize, &nblocks, &nwaves, &slot);
        TRY(c->cw[0].ensure(n_chunks, nblocks, nwaves, slot));
    }
    return HHGT_OK;
}

extern "C" int hhgt_set_clevel(hhgt_ctx *c, int clevel)
{
    if (!c || clevel < 1 || clevel > 9) {
        hhgt_set_error("clevel must be 1..9");
        return HHGT_ERR_ARG;
    }
    c->clevel = clevel;
    return HHGT_OK;
}

extern "C" int hhgt_stream_create(hhgt_ctx *c, int kind, void **out)
{
    if (!c || !out || (kind != HHGT_STREAM_ENCODE && kind != HHGT_STREAM_COMPRESS && kind != HHGT_STREAM_FRAME)) {
        hhgt_set_error("hhgt_stream_create: bad arguments");
        return HHGT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = nullptr;
    if (kind == HHGT_STREAM_FRAME) {
        HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    } else if (kind == HHGT_STREAM_ENCODE) {
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIP_TRY(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi));
    } else {
        const uint32_t n_cu = (uint32_t)c->prop.multiProcessorCount;
        // the mask works in groups of 32 CUs on this part (one XCD): 3/4 of the chip, rounded to that
        uint32_t use = n_cu >= 128u ? (n_cu * 3u / 4u) / 32u * 32u : n_cu;
        if (const char *e = getenv("HHGT_COMPRESS_CUS")) {
            const int v = atoi(e);
            use = v <= 0 || (uint32_t)v >= n_cu ? n_cu : (uint32_t)v;
        }
        if (use >= n_cu) {
            HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        } else {
            std::vector<uint32_t> mask((n_cu + 31u) / 32u, 0u);
            for (uint32_t i = n_cu - use; i < n_cu; ++i) mask[i >> 5] |= 1u << (i & 31u);   // the last `use` CUs of the mask order
            if (hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
                (void)hipGetLastError();   // a runtime that refuses the mask: an ordinary stream does the same work
                st = nullptr;
                HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            }
        }
    }
    *out = st;
    return HHGT_OK;
}

extern "C" int hhgt_set_frame_stream(hhgt_ctx *c, void *stream)
{
    if (!c) return HHGT_ERR_ARG;
    HIP_TRY(hipSetDevice(c->device));
    // framings still in flight on the old stream read the workspace sets: let them finish before the roles change
    if (c->frame_stream) HIP_TRY(hipStreamSynchronize(c->frame_stream));
    for (auto &w : c->cw) w.fr_pending = false;
    c->frame_stream = reinterpret_cast<hipStream_t>(stream);
    return HHGT_OK;
}

extern "C" int hhgt_stream_destroy(hhgt_ctx *c, void *stream)
{
    if (!c) return HHGT_ERR_ARG;
    if (stream) {
        HIP_TRY(hipSetDevice(c->device));
        if (reinterpret_cast<hipStream_t>(stream) == c->frame_stream) TRY(hhgt_set_frame_stream(c, nullptr));
        HIP_TRY(hipStreamDestroy(reinterpret_cast<hipStream_t>(stream)));
    }
    return HHGT_OK;
}

extern "C" int hhgt_set_index_mode(hhgt_ctx *c, int mode)
{
    if (!c || mode < -1 || mode > 2) {
        hhgt_set_error("index mode must be -1 (default), 0 (scan), 1 (hop) or 2 (walk)");
        return HHGT_ERR_ARG;
    }
    c->index_mode = mode;
    return HHGT_OK;
}

extern "C" int hhgt_set_keep_multiallelic(hhgt_ctx *c, int on)
{
    if (!c) return HHGT_ERR_ARG;
    c->keep_multi = on ? 1 : 0;
    return HHGT_OK;
}

__global__ void k_count_nonzero_u32(const uint32_t *__restrict__ v, uint64_t n, unsigned long long *out)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long m = __ballot(i < n && v[i] != 0u);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(out, (unsigned long long)__builtin_popcountll(m));
}

extern "C" int hhgt_inflate_members(hhgt_ctx *c, const void *d_src, uint64_t src_bytes, const uint64_t *d_comp_off,
                                    const uint32_t *d_comp_len, const uint64_t *d_out_off, const uint32_t *d_isize,
                                    uint64_t n_members, void *d_dst, uint64_t dst_bytes, const uint32_t *d_crc32,
                                    uint32_t *d_status, uint64_t *n_bad, void *stream)
{
    if (!c || !d_src || !d_comp_off || !d_comp_len || !d_out_off || !d_isize || !d_status || (!d_dst && dst_bytes))
        return HHGT_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    if (n_bad) *n_bad = 0;
    if (n_members == 0) return HHGT_OK;
    if (d_crc32 && !c->crc_x2n_ready) {
        uint32_t t[32];
        crc32_x2n_table(t);
        TRY(c->crc_x2n.ensure(sizeof(t)));
        HIP_TRY(hipMemcpy(c->crc_x2n.p, t, sizeof(t), hipMemcpyHostToDevice));
        c->crc_x2n_ready = true;
    }
    TRY(timed(c, st, HHGT_STAGE_INFLATE, [&] {
        return launch_inflate(static_cast<const uint8_t *>(d_src), src_bytes, d_comp_off, d_comp_len, d_out_off, d_isize, n_members,
                              static_cast<uint8_t *>(d_dst), dst_bytes, d_status, d_crc32, c->crc_x2n.as<uint32_t>(), st);
    }));
    if (n_bad) {
        TRY(c->dec_bad.ensure(8));
        HIP_TRY(hipMemsetAsync(c->dec_bad.p, 0, 8, st));
        hipLaunchKernelGGL(k_count_nonzero_u32, dim3((uint32_t)((n_members + 255) / 256)), dim3(256), 0, st, d_status,
                           n_members, c->dec_bad.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        uint64_t nb = 0;
        HIP_TRY(hipMemcpyAsync(&nb, c->dec_bad.p, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *n_bad = nb;
    }
    return HHGT_OK;
}

// the bad-counter protocol around a decode launch: c->dec_bad zeroed on the stream, launch(d_bad) under the DECODE stage
// timer, then, if the caller wants it, the count copied back (synchronises)
template <typename Launch>
static int with_bad_counter(hhgt_ctx *c, hipStream_t st, uint64_t *n_bad, Launch launch)
{
    TRY(c->dec_bad.ensure(8));
    HIP_TRY(hipMemsetAsync(c->dec_bad.p, 0, 8, st));
    TRY(timed(c, st, HHGT_STAGE_DECODE, [&] { return launch(c->dec_bad.as<unsigned long long>()); }));
    if (n_bad) {
        uint64_t nb = 0;
        HIP_TRY(hipMemcpyAsync(&nb, c->dec_bad.p, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *n_bad = nb;
    }
    return HHGT_OK;
}

extern "C" int hhgt_decompress_chunks(hhgt_ctx *c, const void *d_src, const uint64_t *d_chunk_off, uint64_t n_chunks,
                                      uint64_t chunk_nbytes, int typesize, int blocksize, void *d_dst,
                                      uint64_t *n_bad, void *stream)
{
    if (!c || !d_src || !d_dst || !d_chunk_off) return HHGT_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    TRY(check_decode_block(typesize, blocksize));
    TRY(check_codec_args(chunk_nbytes, typesize, blocksize, HHGT_BLOSC2));
    if (n_bad) *n_bad = 0;
    if (n_chunks == 0) return HHGT_OK;
    blocksize = effective_blocksize(chunk_nbytes, typesize, blocksize);
    return with_bad_counter(c, st, n_bad, [&](unsigned long long *d_bad) {
        return launch_decode(static_cast<const uint8_t *>(d_src), d_chunk_off, n_chunks, chunk_nbytes, typesize, blocksize,
                             static_cast<uint8_t *>(d_dst), d_bad, st);
    });
}

extern "C" int hhgt_decompress_blocks(hhgt_ctx *c, const hhgt_block_sel *d_sel, uint32_t n_sel, uint64_t chunk_nbytes,
                                      int typesize, int blocksize, void *d_dst, uint64_t *n_bad, void *stream)
{
    TRY(check_not_null("decompress_blocks", c, !n_sel ? nullptr : !d_sel ? "selection array" : !d_dst ? "destination" : nullptr));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    TRY(check_decode_block(typesize, blocksize));
    TRY(check_codec_args(chunk_nbytes, typesize, blocksize, HHGT_BLOSC2));
    if (n_bad) *n_bad = 0;
    if (n_sel == 0) return HHGT_OK;
    blocksize = effective_blocksize(chunk_nbytes, typesize, blocksize);
    return with_bad_counter(c, st, n_bad, [&](unsigned long long *d_bad) {
        return launch_decode_sel(d_sel, n_sel, chunk_nbytes, typesize, blocksize, static_cast<uint8_t *>(d_dst), d_bad, st);
    });
}

// the geometry the row-walk kernels (hhgt_count_alleles, hhgt_count_samples, hhgt_genotype_planes, hhgt_gather_calls) serve;
// `who` prefixes the message
static int check_row_kernel_args(const char *who, uint32_t sc, uint32_t vc, int typesize, int blocksize)
{
    if (typesize != 2) {
        hhgt_set_error("%s: typesize %d (only 2: one diploid int8 call)", who, typesize);
        return HHGT_ERR_ARG;
    }
    if (sc < 1 || sc > 64 || vc < 1) {
        hhgt_set_error("%s: chunk of %u samples x %u variants (1 to 64 samples)", who, sc, vc);
        return HHGT_ERR_ARG;
    }
    TRY(check_codec_args((uint64_t)sc * vc * 2u, typesize, blocksize, HHGT_BLOSC2));
    if (blocksize > 8192 || ((uint64_t)vc * 2u) % (uint64_t)blocksize) {
        hhgt_set_error("%s: blocksize %d does not cut a row of %u variants into whole blocks of at most 8192 bytes", who,
                       blocksize, vc);
        return HHGT_ERR_ARG;
    }
    return HHGT_OK;
}

// what the row kernels' entry points do alike: the null checks (`out`: the output's name in the message), the geometry, the
// device, *n_bad, nothing to do without selections, the launch under the bad-counter protocol
template <typename Launch>
static int run_row_kernel(const char *who, const char *out, hhgt_ctx *c, const void *d_sel, uint32_t n_sel, const void *d_out,
                          uint32_t sc, uint32_t vc, int typesize, int blocksize, uint64_t *n_bad, void *stream, Launch launch)
{
    TRY(check_not_null(who, c, !n_sel ? nullptr : !d_sel ? "selection array" : !d_out ? out : nullptr));
    TRY(check_row_kernel_args(who, sc, vc, typesize, blocksize));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    if (n_bad) *n_bad = 0;
    if (n_sel == 0) return HHGT_OK;
    return with_bad_counter(c, st, n_bad, [&](unsigned long long *d_bad) { return launch(d_bad, st); });
}

extern "C" int hhgt_count_alleles(hhgt_ctx *c, const hhgt_count_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc,
                                  int typesize, int blocksize, uint32_t *d_counts, uint64_t n_out, uint64_t *n_bad,
                                  void *stream)
{
    return run_row_kernel("count_alleles", "counts", c, d_sel, n_sel, d_counts, sc, vc, typesize, blocksize, n_bad, stream,
                          [&](unsigned long long *d_bad, hipStream_t st) {
                              return launch_count_alleles(d_sel, n_sel, sc, vc, blocksize, d_counts, n_out, d_bad, st);
                          });
}

extern "C" int hhgt_count_samples(hhgt_ctx *c, const hhgt_sample_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc,
                                  int typesize, int blocksize, const uint32_t *d_vmask, uint64_t vmask_words,
                                  uint32_t *d_counts, uint64_t n_out, uint64_t *n_bad, void *stream)
{
    return run_row_kernel("count_samples", "counts", c, d_sel, n_sel, d_counts, sc, vc, typesize, blocksize, n_bad, stream,
                          [&](unsigned long long *d_bad, hipStream_t st) {
                              return launch_count_samples(d_sel, n_sel, sc, vc, blocksize, d_vmask, vmask_words, d_counts,
                                                          n_out, d_bad, st);
                          });
}

extern "C" int hhgt_genotype_planes(hhgt_ctx *c, const hhgt_plane_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc,
                                    int typesize, int blocksize, const uint32_t *d_vmask, uint64_t vmask_words,
                                    uint32_t *d_planes, uint64_t n_rows, uint64_t row_words, uint64_t *n_bad,
                                    void *stream)
{
    return run_row_kernel("genotype_planes", "planes", c, d_sel, n_sel, d_planes, sc, vc, typesize, blocksize, n_bad, stream,
                          [&](unsigned long long *d_bad, hipStream_t st) {
                              return launch_genotype_planes(d_sel, n_sel, sc, vc, blocksize, d_vmask, vmask_words, d_planes,
                                                            n_rows, row_words, d_bad, st);
                          });
}

extern "C" int hhgt_gather_calls(hhgt_ctx *c, const hhgt_gather_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc,
                                 int typesize, int blocksize, const uint32_t *d_vmask, uint64_t vmask_words,
                                 const uint32_t *d_row_map, uint64_t n_map, const void *d_values, int elem_bytes,
                                 void *d_out, uint64_t n_rows, uint64_t n_cols, uint64_t row_stride, uint64_t *n_bad,
                                 void *stream)
{
    const bool table = d_values != nullptr;
    if (table ? (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) : elem_bytes != 2) {
        hhgt_set_error("gather_calls: elem_bytes %d (%s)", elem_bytes, table ? "1, 2, 4 or 8" : "2 without a table: an allele pair");
        return HHGT_ERR_ARG;
    }
    if (row_stride < n_cols) {
        hhgt_set_error("gather_calls: row_stride %llu below n_cols %llu", (unsigned long long)row_stride, (unsigned long long)n_cols);
        return HHGT_ERR_ARG;
    }
    const uintptr_t off = (uintptr_t)elem_bytes - 1u;
    if ((reinterpret_cast<uintptr_t>(d_out) & off) || (reinterpret_cast<uintptr_t>(d_values) & off)) {
        hhgt_set_error("gather_calls: %s not aligned to elem_bytes %d", (reinterpret_cast<uintptr_t>(d_out) & off) ? "d_out" : "d_values",
                       elem_bytes);
        return HHGT_ERR_ARG;
    }
    return run_row_kernel("gather_calls", "output", c, d_sel, n_sel, d_out, sc, vc, typesize, blocksize, n_bad, stream,
                          [&](unsigned long long *d_bad, hipStream_t st) {
                              return launch_gather_calls(d_sel, n_sel, sc, vc, blocksize, d_vmask, vmask_words, d_row_map, n_map,
                                                         d_values, elem_bytes, d_out, n_rows, n_cols, row_stride, d_bad, st);
                          });
}

// what hhgt_pair_counts, hhgt_grm and hhgt_variant_planes do alike.  null_arg: the name of the first null pointer among those
// the work needs, misaligned: what to say about a pointer off its alignment (nullptr: none); the words [w_lo, w_hi) must lie
// in the rows, of which there are at most row_limit; nothing to do without rows or words; the launch under its stage's timer
template <typename Launch>
static int run_plane_kernel(const char *who, int stage, hhgt_ctx *c, const char *null_arg, const char *misaligned, uint64_t n_rows,
                            uint64_t row_words, uint64_t w_lo, uint64_t w_hi, uint64_t row_limit, void *stream, Launch launch)
{
    const bool work = n_rows && w_lo < w_hi;
    TRY(check_not_null(who, c, work ? null_arg : nullptr));
    if (w_lo > w_hi || w_hi > row_words || n_rows > row_limit) {
        hhgt_set_error("%s: words [%llu, %llu) of rows of %llu words, %llu rows", who, (unsigned long long)w_lo,
                       (unsigned long long)w_hi, (unsigned long long)row_words, (unsigned long long)n_rows);
        return HHGT_ERR_ARG;
    }
    if (misaligned) {
        hhgt_set_error("%s: %s", who, misaligned);
        return HHGT_ERR_ARG;
    }
    return launch_on_device(c, stream, stage, work, launch);
}

static bool off_alignment(const void *p, uintptr_t align) { return reinterpret_cast<uintptr_t>(p) & (align - 1u); }

extern "C" int hhgt_pair_counts(hhgt_ctx *c, const uint32_t *d_planes, uint64_t n_rows, uint64_t row_words, uint64_t w_lo,
                                uint64_t w_hi, uint32_t *d_table, void *stream)
{
    return run_plane_kernel("pair_counts", HHGT_STAGE_PAIRS, c, !d_planes ? "planes" : !d_table ? "table" : nullptr,
                            off_alignment(d_table, 16) ? "the table must be 16-byte aligned" : nullptr, n_rows, row_words, w_lo, w_hi,
                            64ull * 65535ull, stream, [&](hipStream_t st) {
                                return launch_pair_counts(d_planes, (uint32_t)n_rows, row_words, w_lo, w_hi, d_table, st);
                            });
}

extern "C" int hhgt_grm(hhgt_ctx *c, const uint32_t *d_planes, uint64_t n_rows, uint64_t row_words, uint64_t w_lo, uint64_t w_hi,
                        const float *d_z, double *d_table, void *stream)
{
    return run_plane_kernel("grm", HHGT_STAGE_GRM, c, !d_planes ? "planes" : !d_z ? "weights" : !d_table ? "table" : nullptr,
                            off_alignment(d_table, 8) || off_alignment(d_z, 16)
                                ? "the table must be 8-byte aligned, the weights 16-byte aligned" : nullptr,
                            n_rows, row_words, w_lo, w_hi, 64ull * 65535ull, stream, [&](hipStream_t st) {
                                return launch_grm(d_planes, (uint32_t)n_rows, row_words, w_lo, w_hi, d_z, d_table, st);
                            });
}

extern "C" int hhgt_variant_planes(hhgt_ctx *c, const uint32_t *d_planes, uint64_t n_rows, uint64_t row_words, uint64_t w_lo,
                                   uint64_t w_hi, uint32_t *d_vplanes, void *stream)
{
    return run_plane_kernel("variant_planes", HHGT_STAGE_LD_TRANSPOSE, c, !d_planes ? "planes" : !d_vplanes ? "variant planes" : nullptr,
                            nullptr, n_rows, row_words, w_lo, w_hi, 256ull * 65535ull, stream, [&](hipStream_t st) {
                                return launch_variant_planes(d_planes, (uint32_t)n_rows, row_words, w_lo, w_hi, d_vplanes, st);
                            });
}

// what hhgt_ld_counts and hhgt_ld_prune check alike: the window (and r2, where there is one), the pointers (null_arg as above),
// the table's alignment
static int check_ld_args(const char *who, hhgt_ctx *c, uint32_t window, const double *r2, const char *null_arg, const uint32_t *d_table)
{
    if (window < 1u || window > 1024u || (r2 && !(*r2 >= 0.0 && *r2 <= 1.0))) {
        if (r2)
            hhgt_set_error("%s: window %u, r2 %g (1 to 1024, 0 to 1)", who, window, *r2);
        else
            hhgt_set_error("%s: window %u (1 to 1024)", who, window);
        return HHGT_ERR_ARG;
    }
    TRY(check_not_null(who, c, null_arg));
    if (off_alignment(d_table, 32)) {
        hhgt_set_error("%s: the table must be 32-byte aligned", who);
        return HHGT_ERR_ARG;
    }
    return HHGT_OK;
}

extern "C" int hhgt_ld_counts(hhgt_ctx *c, const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, uint32_t window,
                              uint32_t *d_table, void *stream)
{
    const bool work = n_var && sw;
    TRY(check_ld_args("ld_counts", c, window, nullptr, !work ? nullptr : !d_vplanes ? "variant planes" : !d_table ? "table" : nullptr, d_table));
    return launch_on_device(c, stream, HHGT_STAGE_LD, work,
                            [&](hipStream_t st) { return launch_ld_counts(d_vplanes, n_var, sw, window, d_table, st); });
}

extern "C" int hhgt_ld_prune(hhgt_ctx *c, const uint32_t *d_table, uint64_t n_var, uint32_t window, double r2,
                             uint8_t *d_keep, void *stream)
{
    TRY(check_ld_args("ld_prune", c, window, &r2, !n_var ? nullptr : !d_table ? "table" : !d_keep ? "keep flags" : nullptr, d_table));
    return on_device(c, stream, n_var != 0, [&](hipStream_t st) {
        TRY(c->ld_bits.ensure((size_t)n_var * ld_walk_words(window) * sizeof(uint64_t)));
        uint64_t *bits = c->ld_bits.as<uint64_t>();
        TRY(timed(c, st, HHGT_STAGE_LD_PRUNE, [&] { return launch_ld_exceeds(d_table, n_var, window, r2, bits, st); }));
        return timed(c, st, HHGT_STAGE_LD_WALK, [&] { return launch_ld_walk(bits, n_var, window, d_keep, st); });
    });
}

// n_var of the clumping calls: int32 owners, 2^33 link words
static int check_clump_variants(const char *who, uint64_t n_var)
{
    if (n_var <= 0x7fffffffull) return HHGT_OK;
    hhgt_set_error("%s: %llu variants (below 2^31)", who, (unsigned long long)n_var);
    return HHGT_ERR_ARG;
}

extern "C" int hhgt_ld_decisions(hhgt_ctx *c, const uint32_t *d_table, uint64_t n_var, uint32_t window, double r2,
                                 const int64_t *d_pos, int64_t max_dist, uint64_t *d_bits, void *stream)
{
    TRY(check_ld_args("ld_decisions", c, window, &r2, !n_var ? nullptr : !d_table ? "table" : !d_bits ? "link bits" : nullptr, d_table));
    TRY(check_clump_variants("ld_decisions", n_var));
    if (max_dist < 0) {
        hhgt_set_error("ld_decisions: max_dist %lld (at least 0)", (long long)max_dist);
        return HHGT_ERR_ARG;
    }
    return launch_on_device(c, stream, HHGT_STAGE_LD_PRUNE, n_var != 0, [&](hipStream_t st) {
        return launch_ld_decisions(d_table, n_var, window, r2, d_pos, max_dist, d_bits, st);
    });
}

// the rounds go out in batches of CLUMP_BATCH launches, each with a counter of its own; the host reads a batch's counters in
// one copy and stops at the first round that decided nothing (the state no longer changes: whichever buffer was written
// last holds it).  All of it under the walk's timer.
extern "C" int hhgt_ld_clump(hhgt_ctx *c, const uint64_t *d_bits, uint64_t n_var, uint32_t window, const uint32_t *d_rank,
                             const uint8_t *d_eligible, int32_t *d_owner, uint32_t *rounds, void *stream)
{
    if (rounds) *rounds = 0;
    TRY(check_ld_args("ld_clump", c, window, nullptr, !n_var ? nullptr : !d_bits ? "link bits" : !d_rank ? "ranks"
                      : !d_eligible ? "eligible flags" : !d_owner ? "owners" : nullptr, nullptr));
    TRY(check_clump_variants("ld_clump", n_var));
    return on_device(c, stream, n_var != 0, [&](hipStream_t st) {
        const uint32_t nq = (window + 63u) / 64u;
        TRY(c->clump_ws.ensure(ClumpWs::bytes(n_var, nq)));
        const ClumpWs ws(c->clump_ws.p, n_var, nq);
        uint64_t decided = 0;
        TRY(timed(c, st, HHGT_STAGE_LD_WALK, [&] {
            TRY(launch_clump_blockers(d_bits, n_var, window, d_rank, d_eligible, ws, st));
            uint32_t from = 0, h_count[CLUMP_BATCH];
            for (bool more = true; more;) {
                HIP_TRY(hipMemsetAsync(ws.counters, 0, sizeof(h_count), st));
                for (uint32_t r = 0; r < CLUMP_BATCH; ++r, from ^= 1u) TRY(launch_clump_round(n_var, window, ws, from, ws.counters + r, st));
                HIP_TRY(hipMemcpyAsync(h_count, ws.counters, sizeof(h_count), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                for (uint32_t r = 0; r < CLUMP_BATCH && more; ++r) {
                    if (h_count[r] == 0u) {
                        more = false;
                    } else if (++decided > n_var) {
                        hhgt_set_error("ld_clump: %llu rounds over %llu variants still decide", (unsigned long long)decided,
                                       (unsigned long long)n_var);
                        return HHGT_ERR_HIP;
                    }
                }
            }
            return launch_clump_owners(d_bits, n_var, window, d_rank, ws, from, d_owner, st);
        }));
        HIP_TRY(hipStreamSynchronize(st));
        if (rounds) *rounds = (uint32_t)decided;
        return HHGT_OK;
    });
}

// 1 to 64 columns of weights: hhgt_assoc_sums and hhgt_score_sums
static int check_columns(const char *who, uint32_t n_cols)
{
    if (n_cols >= 1u && n_cols <= 64u) return HHGT_OK;
    hhgt_set_error("%s: %u columns (1 to 64)", who, n_cols);
    return HHGT_ERR_ARG;
}

// hhgt_assoc_sums: the columns, the pointers its work needs (the sums with a variant, the planes and the weights with a
// variant and a word), their alignment
extern "C" int hhgt_assoc_sums(hhgt_ctx *c, const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, const double *d_w,
                               uint32_t n_cols, double *d_sums, void *stream)
{
    TRY(check_columns("assoc_sums", n_cols));
    const bool reads = n_var && sw;
    TRY(check_not_null("assoc_sums", c,
                       !n_var ? nullptr : !d_sums ? "sums" : !reads ? nullptr : !d_vplanes ? "variant planes" : !d_w ? "weights" : nullptr));
    if (off_alignment(d_w, 8) || off_alignment(d_sums, 8)) {
        hhgt_set_error("assoc_sums: the weights and the sums must be 8-byte aligned");
        return HHGT_ERR_ARG;
    }
    return launch_on_device(c, stream, HHGT_STAGE_ASSOC, n_var != 0,
                            [&](hipStream_t st) { return launch_assoc_sums(d_vplanes, n_var, sw, d_w, n_cols, d_sums, st); });
}

// hhgt_quad_forms: the pointers its work needs (the forms with a variant, everything else with a variant and a word), their
// alignment; the limits on the variants and the words are the launch's
extern "C" int hhgt_quad_forms(hhgt_ctx *c, const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, const double *d_coef,
                               const double *d_a, double *d_q, void *stream)
{
    const bool reads = n_var && sw;
    TRY(check_not_null("quad_forms", c,
                       !n_var ? nullptr : !d_q ? "forms" : !reads ? nullptr : !d_vplanes ? "variant planes"
                       : !d_coef ? "coefficients" : !d_a ? "matrix" : nullptr));
    if (off_alignment(d_coef, 8) || off_alignment(d_a, 16) || off_alignment(d_q, 8)) {
        hhgt_set_error("quad_forms: the coefficients and the forms must be 8-byte aligned, the matrix 16-byte aligned");
        return HHGT_ERR_ARG;
    }
    return launch_on_device(c, stream, HHGT_STAGE_ASSOC, n_var != 0,
                            [&](hipStream_t st) { return launch_quad_forms(d_vplanes, n_var, sw, d_coef, d_a, d_q, st); });
}

// hhgt_logistic_fit: the columns of X, the pointers its work needs (the records with a variant, everything else with a variant
// and a word), their alignment
extern "C" int hhgt_logistic_fit(hhgt_ctx *c, const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, const uint32_t *d_valid,
                                 const double *d_x, uint32_t q, const double *d_y, const double *d_beta0, double *d_out,
                                 void *stream)
{
    if (q < 1u || q > HHGT_LOGIT_MAX_COLS - 1u) {
        hhgt_set_error("logistic_fit: %u columns of X (1 to %u)", q, HHGT_LOGIT_MAX_COLS - 1u);
        return HHGT_ERR_ARG;
    }
    const bool reads = n_var && sw;
    TRY(check_not_null("logistic_fit", c,
                       !n_var ? nullptr : !d_out ? "records" : !reads ? nullptr : !d_vplanes ? "variant planes"
                       : !d_valid ? "valid bits" : !d_x ? "X" : !d_y ? "y" : !d_beta0 ? "beta0" : nullptr));
    if (off_alignment(d_x, 8) || off_alignment(d_y, 8) || off_alignment(d_beta0, 8) || off_alignment(d_out, 8)) {
        hhgt_set_error("logistic_fit: X, y, beta0 and the records must be 8-byte aligned");
        return HHGT_ERR_ARG;
    }
    return launch_on_device(c, stream, HHGT_STAGE_ASSOC, n_var != 0, [&](hipStream_t st) {
        return launch_logistic_fit(d_vplanes, n_var, sw, d_valid, d_x, q, d_y, d_beta0, d_out, st);
    });
}

// hhgt_score_sums: a plane kernel with columns — their number and the rows' length checked here, the rest with the family;
// the partial sums' workspace grows in the call, like hhgt_ld_prune's; both launches run under one timer of HHGT_STAGE_ASSOC
extern "C" int hhgt_score_sums(hhgt_ctx *c, const uint32_t *d_planes, uint64_t n_rows, uint64_t row_words, uint64_t w_lo,
                               uint64_t w_hi, const double *d_w, uint32_t n_cols, double *d_sums, void *stream)
{
    if (check_columns("score_sums", n_cols) != HHGT_OK || row_words >= (1ull << 27)) {   // (one message names both)
        hhgt_set_error("score_sums: %u columns (1 to 64), rows of %llu words (below 2^27)", n_cols, (unsigned long long)row_words);
        return HHGT_ERR_ARG;
    }
    return run_plane_kernel("score_sums", HHGT_STAGE_ASSOC, c, !d_planes ? "planes" : !d_w ? "weights" : !d_sums ? "sums" : nullptr,
                            off_alignment(d_w, 8) || off_alignment(d_sums, 8) ? "the weights and the sums must be 8-byte aligned" : nullptr,
                            n_rows, row_words, w_lo, w_hi, 0xffffffffull, stream, [&](hipStream_t st) {
                                TRY(c->score_part.ensure((size_t)score_spans(w_hi - w_lo) * n_rows * n_cols * sizeof(double)));
                                return launch_score_sums(d_planes, (uint32_t)n_rows, row_words, w_lo, w_hi, d_w, n_cols,
                                                         c->score_part.as<double>(), d_sums, st);
                            });
}

// hhgt_region_sums: the scalars are checked here, the tables — they are on the device — by the kernels, under the bad-counter
// protocol of the row kernels (with_bad_counter) but with both launches under one timer of HHGT_STAGE_ASSOC, and with a
// count above 0 an error of the arguments; the partial sums' workspace grows in the call
extern "C" int hhgt_region_sums(hhgt_ctx *c, const uint32_t *d_planes, uint64_t n_rows, uint64_t row_words, const double *d_w,
                                uint32_t n_cols, const int64_t *d_pieces, uint64_t n_pieces, const int64_t *d_runs, uint64_t n_runs,
                                uint64_t n_slots, uint64_t n_regions, double *d_sums, uint64_t *n_bad, void *stream)
{
    if (n_bad) *n_bad = 0;
    const bool work = n_rows && n_pieces;
    if (n_cols < 1u || n_cols > HHGT_REGION_MAX_COLS || row_words >= (1ull << 27) || n_rows >= (1ull << 32) || n_regions >= (1ull << 32)) {
        hhgt_set_error("region_sums: %u columns (1 to %u), %llu rows (below 2^32) of %llu words (below 2^27), %llu regions (below 2^32)",
                       n_cols, (unsigned)HHGT_REGION_MAX_COLS, (unsigned long long)n_rows, (unsigned long long)row_words,
                       (unsigned long long)n_regions);
        return HHGT_ERR_ARG;
    }
    TRY(check_not_null("region_sums", c, !work ? nullptr : !d_planes ? "planes" : !d_w ? "weights" : !d_pieces ? "pieces"
                       : n_runs && !d_runs ? "runs" : !d_sums ? "sums" : nullptr));
    const uint64_t tiles = (n_rows + 127u) / 128u, per_run = n_rows * n_cols;   // (below 2^25, below 2^36)
    if (n_pieces >= (1ull << 31) || tiles * n_pieces >= (1ull << 31) || n_runs >= (1ull << 31) || n_slots >= (1ull << 31)
        || (per_run && (n_runs * per_run + 255u) / 256u >= (1ull << 31)) || n_slots * per_run >= (1ull << 40)) {
        hhgt_set_error("region_sums: %llu pieces, %llu runs and %llu slots over %llu rows of %u columns: more than a launch or the workspace takes",
                       (unsigned long long)n_pieces, (unsigned long long)n_runs, (unsigned long long)n_slots,
                       (unsigned long long)n_rows, n_cols);
        return HHGT_ERR_ARG;
    }
    if (off_alignment(d_w, 8) || off_alignment(d_sums, 8) || off_alignment(d_pieces, 8) || off_alignment(d_runs, 8)) {
        hhgt_set_error("region_sums: the weights, the sums, the pieces and the runs must be 8-byte aligned");
        return HHGT_ERR_ARG;
    }
    return on_device(c, stream, work, [&](hipStream_t st) {
        TRY(c->region_part.ensure((size_t)(n_slots * per_run) * sizeof(double)));
        TRY(c->dec_bad.ensure(8));
        HIP_TRY(hipMemsetAsync(c->dec_bad.p, 0, 8, st));
        TRY(timed(c, st, HHGT_STAGE_ASSOC, [&] {
            return launch_region_sums(d_planes, (uint32_t)n_rows, row_words, d_w, n_cols, d_pieces, n_pieces, d_runs, n_runs, n_slots,
                                      n_regions, c->region_part.as<double>(), d_sums, c->dec_bad.as<unsigned long long>(), st);
        }));
        if (!n_bad) return HHGT_OK;
        uint64_t nb = 0;
        HIP_TRY(hipMemcpyAsync(&nb, c->dec_bad.p, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *n_bad = nb;
        if (!nb) return HHGT_OK;
        hhgt_set_error("region_sums: %llu pieces or runs outside rows of %llu words, %u words a piece, %llu regions or %llu slots",
                       (unsigned long long)nb, (unsigned long long)row_words, (unsigned)HHGT_REGION_SPAN,
                       (unsigned long long)n_regions, (unsigned long long)n_slots);
        return HHGT_ERR_ARG;
    });
}
