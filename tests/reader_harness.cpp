// CPU-only harness for csrc/reader.hip (built with -fsanitize=thread and with -fsanitize=address,undefined by
// tests/test_reader.py; links reader.hip and nothing else of the library): drives the C API of include/hhgt_reader.h the way
// the ingest engine does — blocks held and released out of order, hhgt_reader_stats on a live reader, close at any moment —
// so that the sanitizers see the scanner, the workers and the consumer at work together.
//
//   reader_harness TEXT BGZF GZIP PLAIN TOO_LONG MISSING
//
// BGZF, GZIP and PLAIN hold TEXT; TOO_LONG is a BGZF file with a line longer than a block; MISSING does not exist.
// Exit status 0 and "ok" iff every read gave TEXT and every call returned what the header says.
#include "../include/hhgt_reader.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include <string>
#include <vector>

// the library's error slot (csrc/api.hip) is not linked: this one keeps the last text
static std::mutex g_err_mu;
static std::string g_err;
void hhgt_set_error(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lk(g_err_mu);
    g_err = buf;
}

static int g_failures = 0;
#define EXPECT(cond, ...)                           \
    do {                                            \
        if (!(cond)) {                              \
            fprintf(stderr, "FAILED %s: ", #cond);  \
            fprintf(stderr, __VA_ARGS__);           \
            fprintf(stderr, "\n");                  \
            ++g_failures;                           \
        }                                           \
    } while (0)

static const uint64_t BLOCK = 1u << 20;

static std::vector<uint8_t> slurp(const char *path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[1 << 16];
    for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

static void stats_are_sane(hhgt_reader *r, uint64_t file_size, uint64_t text_size)
{
    uint64_t fb = ~0ull, tb = ~0ull;
    EXPECT(hhgt_reader_stats(r, &fb, &tb) == HHGT_OK, "stats");
    EXPECT(fb <= file_size && tb <= text_size, "stats %llu / %llu", (unsigned long long)fb, (unsigned long long)tb);
}

// to the end through acquire, up to depth - 1 blocks held, the newest given back first
static void read_all(const char *path, const std::vector<uint8_t> &text, int threads, int depth)
{
    const uint64_t file_size = slurp(path).size();
    hhgt_reader *r = nullptr;
    EXPECT(hhgt_reader_open(path, BLOCK, threads, depth, &r) == HHGT_OK && r, "open %s", path);
    if (!r) return;
    stats_are_sane(r, file_size, text.size());
    std::vector<uint8_t> got;
    std::vector<int> held;
    int saw_last = 0;
    for (;;) {
        const void *p = nullptr;
        uint64_t n = 0;
        int tok = -2, last = 0;
        const int rc = hhgt_reader_acquire(r, &p, &n, &tok, &last);
        EXPECT(rc == HHGT_OK, "acquire %s: %d %s", path, rc, g_err.c_str());
        if (rc != HHGT_OK) break;
        stats_are_sane(r, file_size, text.size());
        if (n == 0) {
            EXPECT(tok == -1, "token at end of file: %d", tok);
            break;
        }
        EXPECT(!saw_last, "a block behind the last one");
        saw_last = last;
        const uint8_t *b = static_cast<const uint8_t *>(p);
        EXPECT(b[n - 1] == '\n' || last, "a block that ends inside a line");
        got.insert(got.end(), b, b + n);
        held.push_back(tok);
        if ((int)held.size() >= depth - 1) {
            EXPECT(hhgt_reader_release(r, held.back()) == HHGT_OK, "release");
            held.pop_back();
        }
    }
    for (int t : held) EXPECT(hhgt_reader_release(r, t) == HHGT_OK, "release");
    EXPECT(saw_last, "no last block from %s", path);
    EXPECT(got == text, "%s (threads %d, depth %d): %zu bytes, want %zu", path, threads, depth, got.size(), text.size());
    uint64_t tb = 0;
    hhgt_reader_stats(r, nullptr, &tb);
    EXPECT(tb == text.size(), "text_bytes %llu", (unsigned long long)tb);
    hhgt_reader_close(r);
}

// close with `hold` blocks in the consumer's hands and the scanner in the middle of the file
static void close_early(const char *path, int threads, int depth, int hold)
{
    hhgt_reader *r = nullptr;
    EXPECT(hhgt_reader_open(path, BLOCK, threads, depth, &r) == HHGT_OK && r, "open %s", path);
    if (!r) return;
    for (int k = 0; k < hold; ++k) {
        const void *p = nullptr;
        uint64_t n = 0;
        int tok = -2;
        EXPECT(hhgt_reader_acquire(r, &p, &n, &tok, nullptr) == HHGT_OK && n > 0 && tok >= 0, "acquire before close");
    }
    hhgt_reader_close(r);
}

static void close_after_error(const char *path, int threads, int depth)
{
    hhgt_reader *r = nullptr;
    EXPECT(hhgt_reader_open(path, BLOCK, threads, depth, &r) == HHGT_OK && r, "open %s", path);
    if (!r) return;
    int rc = HHGT_OK;
    for (int k = 0; k < 64 && rc == HHGT_OK; ++k) {
        const void *p = nullptr;
        uint64_t n = 0;
        int tok = -2;
        rc = hhgt_reader_acquire(r, &p, &n, &tok, nullptr);
        if (rc == HHGT_OK && n == 0) break;
        if (rc == HHGT_OK) hhgt_reader_release(r, tok);
    }
    EXPECT(rc == HHGT_ERR_IO && strstr(g_err.c_str(), "longer than"), "error of %s: %d %s", path, rc, g_err.c_str());
    stats_are_sane(r, ~0ull, ~0ull);
    hhgt_reader_close(r);
}

int main(int argc, char **argv)
{
    if (argc != 7) {
        fprintf(stderr, "usage: %s TEXT BGZF GZIP PLAIN TOO_LONG MISSING\n", argv[0]);
        return 2;
    }
    const std::vector<uint8_t> text = slurp(argv[1]);
    EXPECT(text.size() > 2 * BLOCK, "the text must span several blocks");
    for (int kind = 2; kind <= 4; ++kind)
        for (int threads : {1, 4})
            for (int depth = 2; depth <= 4; ++depth) {
                read_all(argv[kind], text, threads, depth);
                for (int hold = 0; hold <= 2; ++hold) close_early(argv[kind], threads, depth, hold);
            }
    for (int threads : {1, 4}) close_after_error(argv[5], threads, 3);
    hhgt_reader *r = reinterpret_cast<hhgt_reader *>(1);
    EXPECT(hhgt_reader_open(argv[6], BLOCK, 1, 2, &r) == HHGT_ERR_IO && r == nullptr, "open of a missing path");
    hhgt_reader_close(nullptr);
    if (g_failures) return 1;
    printf("ok\n");
    return 0;
}
