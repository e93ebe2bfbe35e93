// crc32.h — CRC-32 (RFC 1952) of a host buffer, header only like fast_inflate.h: what the BGZF reader checks every member's
// text with (htslib's bgzf.c does the same) and what the BGZF writer of the synthetic shards puts into the trailers.  The
// carry-less-multiply folding form where the CPU has PCLMULQDQ — an order of magnitude faster than zlib 1.2.11's table
// crc32(), so that the check does not cost as much as the inflate it guards — and the 16-byte table form elsewhere and for
// the tails.  The library exports it as hhgt_crc32 (include/hhgt_reader.h).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <mutex>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace hhgt_crc {

// table form, sixteen bytes per step (portable path and tails)
static uint32_t g_tab[16][256];
static std::once_flag g_once;

static void init_table()
{
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
        g_tab[0][i] = c;
    }
    for (int t = 1; t < 16; ++t)
        for (uint32_t i = 0; i < 256; ++i) g_tab[t][i] = (g_tab[t - 1][i] >> 8) ^ g_tab[0][g_tab[t - 1][i] & 0xFFu];
}

// raw update: c is the running register (already inverted), returns the register
static uint32_t crc32_table_update(uint32_t c, const uint8_t *p, size_t n)
{
    std::call_once(g_once, init_table);
    const uint32_t(*T)[256] = g_tab;
    while (n >= 16) {
        uint32_t a, b, d, e;
        memcpy(&a, p, 4);
        memcpy(&b, p + 4, 4);
        memcpy(&d, p + 8, 4);
        memcpy(&e, p + 12, 4);
        a ^= c;
        c = T[15][a & 0xFFu] ^ T[14][(a >> 8) & 0xFFu] ^ T[13][(a >> 16) & 0xFFu] ^ T[12][a >> 24] ^
            T[11][b & 0xFFu] ^ T[10][(b >> 8) & 0xFFu] ^ T[9][(b >> 16) & 0xFFu] ^ T[8][b >> 24] ^
            T[7][d & 0xFFu] ^ T[6][(d >> 8) & 0xFFu] ^ T[5][(d >> 16) & 0xFFu] ^ T[4][d >> 24] ^
            T[3][e & 0xFFu] ^ T[2][(e >> 8) & 0xFFu] ^ T[1][(e >> 16) & 0xFFu] ^ T[0][e >> 24];
        p += 16;
        n -= 16;
    }
    while (n--) c = T[0][(c ^ *p++) & 0xFFu] ^ (c >> 8);
    return c;
}

#if defined(__x86_64__)
// Carry-less-multiply folding (Gopal et al., "Fast CRC Computation for Generic Polynomials Using PCLMULQDQ", the
// scheme zlib-ng / Chromium's zlib use): four 128-bit lanes are folded over the input 64 bytes per step, then
// into one lane, then reduced to 32 bits (Barrett).  Constants are x^k mod P for the bit-reflected polynomial
// 0xEDB88320.  n >= 64 and n % 16 == 0; the caller feeds the tail through the table form.
__attribute__((target("pclmul,sse4.1"))) static uint32_t crc32_clmul_update(uint32_t crc, const uint8_t *buf, size_t len)
{
    const __m128i k1k2 = _mm_set_epi64x(0x00000001c6e41596, 0x0000000154442bd4);
    const __m128i k3k4 = _mm_set_epi64x(0x00000000ccaa009e, 0x00000001751997d0);
    const __m128i k5k0 = _mm_set_epi64x(0x0000000000000000, 0x0000000163cd6124);
    const __m128i poly = _mm_set_epi64x(0x00000001f7011641, 0x00000001db710641);
    __m128i x0, x1, x2, x3, x4, x5, x6, x7, x8, y5, y6, y7, y8;
    x1 = _mm_loadu_si128((const __m128i *)(buf + 0x00));
    x2 = _mm_loadu_si128((const __m128i *)(buf + 0x10));
    x3 = _mm_loadu_si128((const __m128i *)(buf + 0x20));
    x4 = _mm_loadu_si128((const __m128i *)(buf + 0x30));
    x1 = _mm_xor_si128(x1, _mm_cvtsi32_si128((int)crc));
    x0 = k1k2;
    buf += 64;
    len -= 64;
    while (len >= 64) {   // fold four lanes in parallel
        x5 = _mm_clmulepi64_si128(x1, x0, 0x00);
        x6 = _mm_clmulepi64_si128(x2, x0, 0x00);
        x7 = _mm_clmulepi64_si128(x3, x0, 0x00);
        x8 = _mm_clmulepi64_si128(x4, x0, 0x00);
        x1 = _mm_clmulepi64_si128(x1, x0, 0x11);
        x2 = _mm_clmulepi64_si128(x2, x0, 0x11);
        x3 = _mm_clmulepi64_si128(x3, x0, 0x11);
        x4 = _mm_clmulepi64_si128(x4, x0, 0x11);
        y5 = _mm_loadu_si128((const __m128i *)(buf + 0x00));
        y6 = _mm_loadu_si128((const __m128i *)(buf + 0x10));
        y7 = _mm_loadu_si128((const __m128i *)(buf + 0x20));
        y8 = _mm_loadu_si128((const __m128i *)(buf + 0x30));
        x1 = _mm_xor_si128(_mm_xor_si128(x1, x5), y5);
        x2 = _mm_xor_si128(_mm_xor_si128(x2, x6), y6);
        x3 = _mm_xor_si128(_mm_xor_si128(x3, x7), y7);
        x4 = _mm_xor_si128(_mm_xor_si128(x4, x8), y8);
        buf += 64;
        len -= 64;
    }
    x0 = k3k4;   // fold the four lanes into one
    x5 = _mm_clmulepi64_si128(x1, x0, 0x00);
    x1 = _mm_clmulepi64_si128(x1, x0, 0x11);
    x1 = _mm_xor_si128(_mm_xor_si128(x1, x2), x5);
    x5 = _mm_clmulepi64_si128(x1, x0, 0x00);
    x1 = _mm_clmulepi64_si128(x1, x0, 0x11);
    x1 = _mm_xor_si128(_mm_xor_si128(x1, x3), x5);
    x5 = _mm_clmulepi64_si128(x1, x0, 0x00);
    x1 = _mm_clmulepi64_si128(x1, x0, 0x11);
    x1 = _mm_xor_si128(_mm_xor_si128(x1, x4), x5);
    while (len >= 16) {   // single-lane folds over the remaining 16-byte pieces
        x2 = _mm_loadu_si128((const __m128i *)buf);
        x5 = _mm_clmulepi64_si128(x1, x0, 0x00);
        x1 = _mm_clmulepi64_si128(x1, x0, 0x11);
        x1 = _mm_xor_si128(_mm_xor_si128(x1, x2), x5);
        buf += 16;
        len -= 16;
    }
    // 128 -> 64 bits
    x2 = _mm_clmulepi64_si128(x1, x0, 0x10);
    x3 = _mm_setr_epi32(~0, 0, ~0, 0);
    x1 = _mm_srli_si128(x1, 8);
    x1 = _mm_xor_si128(x1, x2);
    x0 = k5k0;
    x2 = _mm_srli_si128(x1, 4);
    x1 = _mm_and_si128(x1, x3);
    x1 = _mm_clmulepi64_si128(x1, x0, 0x00);
    x1 = _mm_xor_si128(x1, x2);
    // Barrett reduction 64 -> 32 bits
    x0 = poly;
    x2 = _mm_and_si128(x1, x3);
    x2 = _mm_clmulepi64_si128(x2, x0, 0x10);
    x2 = _mm_and_si128(x2, x3);
    x2 = _mm_clmulepi64_si128(x2, x0, 0x00);
    x1 = _mm_xor_si128(x1, x2);
    return (uint32_t)_mm_extract_epi32(x1, 1);
}

static bool have_clmul()
{
    static const bool ok = __builtin_cpu_supports("pclmul") && __builtin_cpu_supports("sse4.1");
    return ok;
}
#endif

static inline uint32_t crc32(const void *data, size_t n)
{
    const uint8_t *p = static_cast<const uint8_t *>(data);
    uint32_t c = 0xFFFFFFFFu;
#if defined(__x86_64__)
    if (n >= 64 && have_clmul()) {
        const size_t body = n & ~(size_t)15;
        c = crc32_clmul_update(c, p, body);
        p += body;
        n -= body;
    }
#endif
    return ~crc32_table_update(c, p, n);
}

}  // namespace hhgt_crc
