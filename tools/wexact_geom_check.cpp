// wexact_geom_check.cpp — host check of the exact-weight kernels' geometry
// (spx_pbox.h pbox_wexact_geometry / pbox_wexact_slice): tile
// counts, partial-buffer sizes and list slicing over a range of m, walked the way
// the kernels index them on real buffers of exactly the allocated size, so an
// address sanitizer sees any index past a buffer.  No device code runs.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -D__HIP_PLATFORM_AMD__ -I$ROCM/include -Iinclude tools/wexact_geom_check.cpp -o wexact_geom_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../simplex_method_gpu_amd/csrc/spx_pbox.h"

using namespace spx;

static int fails = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            ++fails;                                                     \
        }                                                                \
    } while (0)

static void one(int64_t m, int64_t n) {
    const int64_t L = (m + 127) / 128 * 128;
    const PboxWexactCfg c = pbox_wexact_geometry(m, n, L);
    const int64_t cnt = n - m;
    CHECK(c.cap == cnt);
    CHECK((int64_t)c.row_blocks * PBOX_WX_TILE >= m && (int64_t)(c.row_blocks - 1) * PBOX_WX_TILE < m);
    CHECK((int64_t)c.col_tiles * PBOX_WX_TILE >= cnt && (cnt == 0 || (int64_t)(c.col_tiles - 1) * PBOX_WX_TILE < cnt));
    CHECK((int64_t)c.slack_grid * PBOX_WX_BLOCK >= m && (int64_t)c.sum_grid * PBOX_WX_BLOCK >= cnt);
    CHECK(c.parts == (size_t)c.row_blocks * (size_t)cnt && c.sparts == (size_t)c.row_blocks * (size_t)L);
    // buffers of the allocated sizes; S holds its row index, the list a permutation of the non-basic columns
    std::vector<int32_t> list((size_t)cnt);
    for (int64_t s = 0; s < cnt; ++s) list[(size_t)s] = (int32_t)(cnt - 1 - s);
    std::vector<int> parts(c.parts, 0), sparts(c.sparts, 0);
    std::vector<char> slot_seen((size_t)cnt, 0);
    // k_pbox_wexact: every (row block, column tile) workgroup, its load map and its store
    int64_t rows_covered = 0;
    for (int rb = 0; rb < c.row_blocks; ++rb) {
        int64_t live = 0;
        for (int t = 0; t < PBOX_WX_BLOCK; ++t)
            for (int u = 0; u < 4; ++u) {
                const int64_t i = (int64_t)rb * PBOX_WX_TILE + (t >> 3) + 32 * u;
                if ((t & 7) == 0 && i < m) ++live;
            }
        rows_covered += live;
        for (int ct = 0; ct < c.col_tiles; ++ct) {
            const PboxWexactSlice sl = pbox_wexact_slice(ct, cnt);
            CHECK(sl.lo == (int64_t)ct * PBOX_WX_TILE && sl.hi > sl.lo && sl.hi <= cnt);
            for (int64_t s = sl.lo; s < sl.hi; ++s) {
                const int32_t j = list[(size_t)s];  // (the kernel's gather)
                CHECK(j >= 0 && j < n);
                ++parts[(size_t)rb * (size_t)c.cap + (size_t)s];
                if (rb == 0) slot_seen[(size_t)s] = 1;
            }
        }
    }
    CHECK(rows_covered == m);
    for (int v : parts) CHECK(v == 1);
    for (char v : slot_seen) CHECK(v == 1);
    CHECK(pbox_wexact_slice(c.col_tiles, cnt).lo == cnt && pbox_wexact_slice(c.col_tiles, cnt).hi == cnt);
    // the K loop: 16-wide chunks cover [0, m) and stay inside a row of L doubles
    const int64_t nchunk = (m + PBOX_WX_KC - 1) / PBOX_WX_KC;
    CHECK(nchunk * PBOX_WX_KC >= m && nchunk * PBOX_WX_KC <= L);
    // k_pbox_wexact_slack: one partial per (row block, column k < m)
    for (int rb = 0; rb < c.row_blocks; ++rb)
        for (int gx = 0; gx < c.slack_grid; ++gx)
            for (int t = 0; t < PBOX_WX_BLOCK; ++t) {
                const int64_t k = (int64_t)gx * PBOX_WX_BLOCK + t;
                if (k < m) ++sparts[(size_t)rb * (size_t)L + (size_t)k];
            }
    for (int rb = 0; rb < c.row_blocks; ++rb)
        for (int64_t k = 0; k < L; ++k) CHECK(sparts[(size_t)rb * (size_t)L + (size_t)k] == (k < m ? 1 : 0));
    // k_pbox_wexact_sum: every slot once
    int64_t summed = 0;
    for (int gx = 0; gx < c.sum_grid; ++gx)
        for (int t = 0; t < PBOX_WX_BLOCK; ++t)
            if ((int64_t)gx * PBOX_WX_BLOCK + t < cnt) ++summed;
    CHECK(summed == cnt);
    std::printf("m=%lld n=%lld L=%lld: %d row blocks x %d column tiles, %zu + %zu partials\n", (long long)m,
                (long long)n, (long long)L, c.row_blocks, c.col_tiles, c.parts, c.sparts);
}

int main() {
    const int64_t ms[] = {1, 7, 15, 16, 17, 65, 130, 4096};
    for (int64_t m : ms) {
        one(m, m);          // no non-basic column
        one(m, m + 1);      // one
        one(m, 3 * m);
        one(m, 4 * m);
        one(m, 4 * m + 5);  // a last tile with five slots
    }
    if (fails) std::printf("%d checks failed\n", fails);
    else std::printf("ok\n");
    return fails ? 1 : 0;
}
