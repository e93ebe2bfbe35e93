// CPU-only check of the helpers of csrc/common.h that take k_lz4_bitplanes_uni from a workgroup index to the bytes its
// lanes load (built with -fsanitize=address,undefined by tests/test_gpu_lz4_plane_head.py; calls nothing of the HIP
// runtime).  For every workgroup of the grid of each geometry below:
//   * the dealing of 128 workgroups to 64 blocks hits every (block, byte plane) of the call exactly once;
//   * planes_block32 (multiply-shift by the launch's reciprocals) gives the column, row and block in the row that
//     planes_block (two divisions) gives;
//   * every lane's 8 bytes of the ONE planes and of the EXC planes lie inside the planes buffer, where planes_piece puts
//     the piece of its tile.
// And planes_div32 against the division itself at the edges of its range (dividends below 2^31, divisors below 2^31).
#include "../haplohyped_varawareml_amd/csrc/common.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Geom {
    uint32_t S_pad, bpr, col0, n_cols, buf_cols;   // the call works on columns [col0, col0 + n_cols) of a buffer of buf_cols
};

static int fail(const char *what, const Geom &g, uint32_t wg)
{
    printf("FAIL %s: S_pad %u bpr %u col0 %u n_cols %u, workgroup %u\n", what, g.S_pad, g.bpr, g.col0, g.n_cols, wg);
    return 1;
}

static int check_geom(const Geom &g)
{
    PlanesGeom pg;
    pg.S_pad = g.S_pad, pg.bpr = g.bpr, pg.tpc = 16u * g.bpr, pg.col0 = g.col0;
    const PlanesDiv dv = planes_div(pg);
    const uint64_t planes_bytes = (uint64_t)g.buf_cols * pg.tpc * 4u * g.S_pad * 32u;
    const uint32_t n_blocks = g.n_cols * g.S_pad * g.bpr, grid = (n_blocks + 63u) / 64u * 128u;
    std::vector<uint8_t> seen(2u * (size_t)n_blocks, 0);
    for (uint32_t wg = 0; wg < grid; ++wg) {
        uint32_t bid, h;
        planes_wg_plane(wg, &bid, &h);
        if (h > 1u || bid >= grid / 2u) return fail("dealing out of the grid", g, wg);
        if (bid >= n_blocks) continue;
        if (seen[2u * (size_t)bid + h]++) return fail("plane dealt twice", g, wg);
        uint64_t col, col32;
        uint32_t row, bi, row32, bi32;
        planes_block(pg, bid, &col, &row, &bi);
        planes_block32(pg, dv, bid, &col32, &row32, &bi32);
        if (col != col32 || row != row32 || bi != bi32) return fail("planes_block32 != planes_block", g, wg);
        if (col < g.col0 || col >= (uint64_t)g.col0 + g.n_cols || row >= g.S_pad || bi >= g.bpr) return fail("block outside the call", g, wg);
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const uint64_t at = planes_lane_bytes(pg, dv, bid, h, lane);
            if (at != planes_piece(pg, col, bi * 16u + (lane >> 2), h, row) + (lane & 3u) * 8u) return fail("lane address", g, wg);
            if (planes_piece(pg, col, bi * 16u + (lane >> 2), h + 2u, row) != planes_piece(pg, col, bi * 16u + (lane >> 2), h, row) + planes_exc_step(pg))
                return fail("EXC step", g, wg);
            if (at + 8u > planes_bytes || at + planes_exc_step(pg) + 8u > planes_bytes) return fail("load outside the planes", g, wg);
        }
    }
    for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] != 1) return fail("plane not dealt", g, (uint32_t)i);
    return 0;
}

static int check_div()
{
    const uint32_t top = 0x7fffffffu;
    std::vector<uint32_t> ds = {1, 2, 3, 5, 7, 70, 140, 5120, 65535, 65536, 65537, 0x3fffffff, 0x40000000, 0x40000001, top - 1u, top};
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 20000; ++i) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        ds.push_back((uint32_t)(x >> 33) % top + 1u);
        ds.push_back((uint32_t)(x >> 40) % 100000u + 1u);
    }
    for (uint32_t d : ds) {
        uint32_t mul, sh;
        planes_recip(d, &mul, &sh);
        std::vector<uint64_t> ns = {0, 1, d - 1ull, d, d + 1ull, top / 2u, top - 1ull, top};
        for (uint64_t k : {(uint64_t)2, (uint64_t)3, (uint64_t)(top / d), (uint64_t)(top / d / 2u)})
            for (int e = -1; e <= 1; ++e) ns.push_back(k * d + e);
        for (uint64_t n : ns) {
            if (n > top) continue;
            if (planes_div32((uint32_t)n, mul, sh) != (uint32_t)n / d) {
                printf("FAIL planes_div32: %llu / %u\n", (unsigned long long)n, d);
                return 1;
            }
        }
    }
    return 0;
}

int main()
{
    // (samples padded, blocks per row, first column, columns of the call, columns of the buffer): the shapes of
    // tests/test_gpu_lz4_plane_head.py and the flagship's (2504 -> 2560 rows, 8192 variants per chunk, 32 columns)
    const Geom geoms[] = {
        {1, 1, 0, 1, 1},   {7, 1, 0, 9, 9},   {8, 2, 0, 4, 4},    {65, 1, 0, 1, 1},  {127, 1, 0, 1, 1},    {128, 1, 0, 1, 1},     {43, 1, 0, 3, 3},
        {257, 1, 0, 1, 1}, {11, 2, 0, 3, 3},  {16, 2, 0, 4, 4},   {43, 2, 0, 3, 3},  {7, 1, 2, 9, 12},     {8, 2, 1, 4, 6},       {43, 1, 1, 3, 5},
        {128, 1, 2, 1, 3}, {128, 1, 0, 2, 2}, {8, 1, 0, 1, 1},    {3, 5, 1, 11, 12}, {2560, 2, 0, 32, 32}, {2560, 2, 7, 20, 32},
    };
    for (const Geom &g : geoms)
        if (check_geom(g)) return 1;
    if (check_div()) return 1;
    printf("ok\n");
    return 0;
}
