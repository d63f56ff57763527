// bound_ranging_geom_check.cpp — host check of the bound ranging kernels' geometry
// (spx_bndrange.h bnd_geometry): grid extents, the partial buffer's
// size and every index k_rng_bound_gather, k_rng_bound, k_rng_bound_min and
// k_rng_bound_basic form, walked the way the kernels form them on real buffers of
// exactly the allocated size, so an address sanitizer sees any index past a
// buffer.  No device code runs.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -D__HIP_PLATFORM_AMD__ -I$ROCM/include -Iinclude tools/bound_ranging_geom_check.cpp \
//       -o bound_ranging_geom_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../simplex_method_gpu_amd/csrc/spx_bndrange.h"

using namespace spx;

static int fails = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            ++fails;                                                     \
        }                                                                \
    } while (0)

// the LDS layout of k_rng_bound's epilogue (spx_bndrange.hip): the staged rows, then the half records
static const int LDS_DOUBLES = 2 * 2 * RNG_TILE * RNG_LD;
static const int ROWS_DBL = 3 * RNG_TILE;
static const int HALF_BYTES = 24;

static void one(int64_t m, int64_t n) {
    const int64_t L = (m + 127) / 128 * 128;
    const BndCfg c = bnd_geometry(m, n);
    const int64_t cnt = n - m;
    CHECK(c.cap == cnt);
    CHECK((int64_t)c.row_blocks * RNG_TILE >= m && (int64_t)(c.row_blocks - 1) * RNG_TILE < m);
    CHECK((int64_t)c.col_tiles * RNG_TILE >= cnt && (cnt == 0 || (int64_t)(c.col_tiles - 1) * RNG_TILE < cnt));
    CHECK((int64_t)c.slot_grid * RNG_BLOCK >= cnt && (int64_t)c.row_grid * RNG_BLOCK >= m);
    CHECK(c.parts == (size_t)c.row_blocks * (size_t)cnt);
    CHECK(2 * ((int64_t)c.row_blocks * RNG_TILE) + 1 < 0x7fffffff);  // the in-kernel keys are 32-bit
    // buffers of the allocated sizes: the list a permutation of the non-basic columns, the basis the rest
    std::vector<int32_t> list((size_t)cnt), col((size_t)cnt, -1), kind((size_t)cnt, -1);
    for (int64_t s = 0; s < cnt; ++s) list[(size_t)s] = (int32_t)(cnt - 1 - s);
    std::vector<int64_t> b_ixs((size_t)m);
    for (int64_t i = 0; i < m; ++i) b_ixs[(size_t)i] = cnt + i;
    std::vector<double> S((size_t)m * (size_t)L, 1.0), A((size_t)L * (size_t)n, 1.0), ub((size_t)n, 1.0);
    std::vector<double> ubj((size_t)cnt, 0.0), x_b((size_t)L, 1.0), ub_B((size_t)L, 1.0);
    std::vector<signed char> at_upper((size_t)n, 0), is_free((size_t)n, 0);
    std::vector<int> parts(c.parts, 0), out_n((size_t)n, 0);
    double sink = 0.0;
    // k_rng_bound_gather: every slot once
    for (int gx = 0; gx < c.slot_grid; ++gx)
        for (int t = 0; t < RNG_BLOCK; ++t) {
            const int64_t s = (int64_t)gx * RNG_BLOCK + t;
            if (s >= cnt) continue;
            const int32_t j = list[(size_t)s];
            CHECK(j >= 0 && j < n);
            sink += is_free[(size_t)j] + at_upper[(size_t)j];
            col[(size_t)s] = j;
            kind[(size_t)s] = 0;
            ubj[(size_t)s] = ub[(size_t)j];
        }
    for (int32_t v : col) CHECK(v >= 0);
    // k_rng_bound: every (row block, column tile) workgroup: its load map over the whole K loop, the staged rows,
    // the half records and its store
    const int64_t nchunk = (m + RNG_KC - 1) / RNG_KC;
    CHECK(nchunk * RNG_KC >= m && nchunk * RNG_KC <= L);
    CHECK(ROWS_DBL * 8 + 2 * RNG_TILE * HALF_BYTES <= LDS_DOUBLES * 8);  // rows and half records fit the staging buffers
    for (int rb = 0; rb < c.row_blocks; ++rb)
        for (int ct = 0; ct < c.col_tiles; ++ct) {
            const int64_t row0 = (int64_t)rb * RNG_TILE, slot0 = (int64_t)ct * RNG_TILE;
            for (int t = 0; t < RNG_BLOCK; ++t) {
                const int lk = 2 * (t & 7), lr = t >> 3;
                for (int u = 0; u < 4; ++u) {
                    const int64_t i = row0 + lr + 32 * u, s = slot0 + lr + 32 * u;
                    const double* srow = i < m ? S.data() + i * L : nullptr;
                    const double* acol = s < cnt ? A.data() + (int64_t)list[(size_t)s] * L : nullptr;
                    CHECK((lr + 32 * u) * RNG_LD + lk + 1 < RNG_TILE * RNG_LD);  // the LDS slot of the staged dbl2
                    for (int64_t ch = 0; ch < nchunk; ++ch) {
                        const int64_t k = ch * RNG_KC + lk;
                        if (k >= m) continue;  // (bd_load: zeros without a load)
                        if (srow) sink += srow[k] + srow[k + 1];  // (k + 1 <= L - 1: inside the row's pitch)
                        if (acol) sink += acol[k] + acol[k + 1];
                    }
                }
            }
            for (int t = 0; t < RNG_TILE; ++t) {  // the staged rows: x_b, ub_B, the basic column's flag
                const int64_t i = row0 + t;
                if (i < m) sink += x_b[(size_t)i] + ub_B[(size_t)i] + is_free[(size_t)b_ixs[(size_t)i]];
            }
            int half_seen[2 * RNG_TILE] = {0};
            int row_seen[RNG_TILE] = {0};
            for (int wave = 0; wave < 4; ++wave)
                for (int lane = 0; lane < 64; ++lane) {
                    const int cl = lane & 15, kr = lane >> 4, wr = wave >> 1, wc = wave & 1;
                    for (int it = 0; it < 4; ++it)
                        for (int r = 0; r < 4; ++r) {
                            const int li = wr * 64 + 16 * it + 4 * r + kr;
                            CHECK(li >= 0 && li < RNG_TILE);  // s_x / s_u / s_fr
                            if (wc == 0 && cl == 0) ++row_seen[li];
                        }
                    if (kr == 0)
                        for (int jt = 0; jt < 4; ++jt) ++half_seen[wr * RNG_TILE + wc * 64 + 16 * jt + cl];
                }
            for (int v : half_seen) CHECK(v == 1);
            for (int v : row_seen) CHECK(v == 1);
            for (int t = 0; t < RNG_TILE; ++t)
                if (slot0 + t < cnt) ++parts[(size_t)rb * (size_t)cnt + (size_t)(slot0 + t)];
        }
    for (int v : parts) CHECK(v == 1);
    // k_rng_bound_min: every slot once, every partial of the slot, the scatter through col
    for (int gx = 0; gx < c.slot_grid; ++gx)
        for (int t = 0; t < RNG_BLOCK; ++t) {
            const int64_t s = (int64_t)gx * RNG_BLOCK + t;
            if (s >= cnt) continue;
            for (int rb = 0; rb < c.row_blocks; ++rb) sink += parts[(size_t)rb * (size_t)cnt + (size_t)s];
            sink += kind[(size_t)s] + ubj[(size_t)s];
            ++out_n[(size_t)col[(size_t)s]];
        }
    // k_rng_bound_basic: every row once, the scatter through b_ixs
    for (int gx = 0; gx < c.row_grid; ++gx)
        for (int t = 0; t < RNG_BLOCK; ++t) {
            const int64_t i = (int64_t)gx * RNG_BLOCK + t;
            if (i >= m) continue;
            const int64_t j = b_ixs[(size_t)i];
            sink += ub_B[(size_t)i] + x_b[(size_t)i] + is_free[(size_t)j];
            ++out_n[(size_t)j];
        }
    for (int v : out_n) CHECK(v == 1);  // every column's range written exactly once
    CHECK(sink > 0.0 || m == 0);
    std::printf("m=%lld n=%lld L=%lld: %d row blocks x %d column tiles, %zu partials; gather / min %d workgroups, basic "
                "%d\n", (long long)m, (long long)n, (long long)L, c.row_blocks, c.col_tiles, c.parts, c.slot_grid,
                c.row_grid);
}

int main() {
    const int64_t ms[] = {1, 7, 15, 16, 17, 65, 130, 4096};
    for (int64_t m : ms) {
        one(m, m);          // no non-basic column
        one(m, m + 1);      // one
        one(m, 3 * m);
        one(m, m == 4096 ? 2 * m : 4 * m);
        one(m, (m == 4096 ? 2 * m : 4 * m) + 5);  // a last tile with five slots
    }
    if (fails) std::printf("%d checks failed\n", fails);
    else std::printf("ok\n");
    return fails ? 1 : 0;
}
