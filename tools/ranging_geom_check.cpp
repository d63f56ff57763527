// ranging_geom_check.cpp — host check of the ranging kernels' geometry
// (spx_ranging.h rng_geometry): grid extents, partial-buffer sizes
// and every index k_rng_gather, k_rng_cost, k_rng_cost_min, k_rng_rhs and
// k_rng_rhs_min form, walked the way the kernels form them on real buffers of
// exactly the allocated size, so an address sanitizer sees any index past a
// buffer.  No device code runs.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -D__HIP_PLATFORM_AMD__ -I$ROCM/include -Iinclude tools/ranging_geom_check.cpp -o ranging_geom_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../simplex_method_gpu_amd/csrc/spx_ranging.h"

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
    const RngCfg c = rng_geometry(m, n);
    const int64_t cnt = n - m;
    CHECK(c.cap == cnt);
    CHECK((int64_t)c.row_blocks * RNG_TILE >= m && (int64_t)(c.row_blocks - 1) * RNG_TILE < m);
    CHECK((int64_t)c.col_tiles * RNG_TILE >= cnt && (cnt == 0 || (int64_t)(c.col_tiles - 1) * RNG_TILE < cnt));
    CHECK((int64_t)c.gather_grid * RNG_BLOCK >= cnt && (int64_t)c.min_grid * RNG_BLOCK >= m);
    CHECK((int64_t)c.rhs_grid_x * RNG_BLOCK >= m && (int64_t)c.rhs_blocks * RNG_ROWS >= m &&
          (int64_t)(c.rhs_blocks - 1) * RNG_ROWS < m);
    CHECK(c.cparts == (size_t)c.col_tiles * (size_t)m && c.rparts == (size_t)c.rhs_blocks * (size_t)m);
    // buffers of the allocated sizes: the list a permutation of the non-basic columns, the basis the rest
    std::vector<int32_t> list((size_t)cnt), col((size_t)cnt, -1);
    for (int64_t s = 0; s < cnt; ++s) list[(size_t)s] = (int32_t)(cnt - 1 - s);
    std::vector<int64_t> b_ixs((size_t)m);
    for (int64_t i = 0; i < m; ++i) b_ixs[(size_t)i] = cnt + i;
    std::vector<double> S((size_t)m * (size_t)L, 1.0), A((size_t)L * (size_t)n, 1.0), d((size_t)n, 0.0);
    std::vector<double> sk((size_t)cnt, 0.0), sig((size_t)cnt, 0.0), x_b((size_t)L, 0.0), ub_B((size_t)L, 0.0);
    std::vector<int> cparts(c.cparts, 0), rparts(c.rparts, 0), cout_n((size_t)n, 0), rout_m((size_t)m, 0);
    double sink = 0.0;
    // k_rng_gather: every slot once; the non-basic columns' outputs
    for (int gx = 0; gx < c.gather_grid; ++gx)
        for (int t = 0; t < RNG_BLOCK; ++t) {
            const int64_t s = (int64_t)gx * RNG_BLOCK + t;
            if (s >= cnt) continue;
            const int32_t j = list[(size_t)s];
            CHECK(j >= 0 && j < n);
            sink += d[(size_t)j];
            sk[(size_t)s] = sig[(size_t)s] = 1.0;
            col[(size_t)s] = j;
            ++cout_n[(size_t)j];
        }
    for (int32_t v : col) CHECK(v >= 0);
    // k_rng_cost: every (row block, column tile) workgroup: its load map over the whole K loop, the slots its
    // epilogue reads, the half records and its store
    const int64_t nchunk = (m + RNG_KC - 1) / RNG_KC;
    CHECK(nchunk * RNG_KC >= m && nchunk * RNG_KC <= L);
    for (int rb = 0; rb < c.row_blocks; ++rb)
        for (int ct = 0; ct < c.col_tiles; ++ct) {
            const int64_t row0 = (int64_t)rb * RNG_TILE, slot0 = (int64_t)ct * RNG_TILE;
            for (int t = 0; t < RNG_BLOCK; ++t) {
                const int lk = 2 * (t & 7), lr = t >> 3;
                for (int u = 0; u < 4; ++u) {
                    const int64_t i = row0 + lr + 32 * u, s = slot0 + lr + 32 * u;
                    const double* srow = i < m ? S.data() + i * L : nullptr;
                    const double* acol = s < cnt ? A.data() + (int64_t)list[(size_t)s] * L : nullptr;
                    // the LDS slot of the staged dbl2
                    CHECK((lr + 32 * u) * RNG_LD + lk + 1 < RNG_TILE * RNG_LD);
                    for (int64_t ch = 0; ch < nchunk; ++ch) {
                        const int64_t k = ch * RNG_KC + lk;
                        if (k >= m) continue;  // (rg_load: zeros without a load)
                        if (srow) sink += srow[k] + srow[k + 1];  // (k + 1 <= L - 1: inside the row's pitch)
                        if (acol) sink += acol[k] + acol[k + 1];
                    }
                }
            }
            int half_seen[2 * RNG_TILE] = {0};
            for (int wave = 0; wave < 4; ++wave)
                for (int lane = 0; lane < 64; ++lane) {
                    const int cl = lane & 15, kr = lane >> 4, wr = wave >> 1, wc = wave & 1;
                    for (int jt = 0; jt < 4; ++jt) {
                        const int64_t s = slot0 + wc * 64 + 16 * jt + cl;
                        if (s < cnt) sink += sk[(size_t)s] + sig[(size_t)s] + col[(size_t)s];
                    }
                    if (cl == 0)
                        for (int it = 0; it < 4; ++it)
                            for (int r = 0; r < 4; ++r) ++half_seen[wc * RNG_TILE + wr * 64 + 16 * it + 4 * r + kr];
                }
            for (int v : half_seen) CHECK(v == 1);
            CHECK(2 * RNG_TILE * 24 <= 2 * 2 * RNG_TILE * RNG_LD * 8);  // the half records fit the staging buffers
            for (int t = 0; t < RNG_TILE; ++t)
                if (row0 + t < m) ++cparts[(size_t)ct * (size_t)m + (size_t)(row0 + t)];
        }
    for (int v : cparts) CHECK(v == 1);
    // k_rng_cost_min: every row once, every partial of the row, the scatter through b_ixs
    for (int gx = 0; gx < c.min_grid; ++gx)
        for (int t = 0; t < RNG_BLOCK; ++t) {
            const int64_t i = (int64_t)gx * RNG_BLOCK + t;
            if (i >= m) continue;
            for (int ct = 0; ct < c.col_tiles; ++ct) sink += cparts[(size_t)ct * (size_t)m + (size_t)i];
            ++cout_n[(size_t)b_ixs[(size_t)i]];
        }
    for (int v : cout_n) CHECK(v == 1);  // every column's range written exactly once
    // k_rng_rhs: the staged rows and the stream of every (column block, row block) workgroup
    for (int rb = 0; rb < c.rhs_blocks; ++rb)
        for (int gx = 0; gx < c.rhs_grid_x; ++gx) {
            const int64_t i0 = (int64_t)rb * RNG_ROWS;
            const int rows = (int)(i0 + RNG_ROWS < m ? RNG_ROWS : m - i0);
            CHECK(rows >= 1 && rows <= RNG_ROWS);
            for (int t = 0; t < RNG_ROWS; ++t)
                if (i0 + t < m) sink += x_b[(size_t)(i0 + t)] + ub_B[(size_t)(i0 + t)] + (double)b_ixs[(size_t)(i0 + t)];
            for (int t = 0; t < RNG_BLOCK; ++t) {
                const int64_t r = (int64_t)gx * RNG_BLOCK + t;
                if (r >= m) continue;
                const double* p = S.data() + i0 * L + r;
                int staged_max = -1;
                for (int i8 = 0; i8 < rows; i8 += 8)  // (RG_AHEAD rows per trip; a row past the block is not loaded)
                    for (int u = 0; u < 8; ++u) {
                        if (i8 + u < rows) sink += p[(int64_t)(i8 + u) * L];
                        staged_max = i8 + u;  // s_x / s_u / s_fr are indexed for the whole chunk
                    }
                CHECK(staged_max < RNG_ROWS);
                ++rparts[(size_t)rb * (size_t)m + (size_t)r];
            }
        }
    for (int v : rparts) CHECK(v == 1);
    // k_rng_rhs_min
    for (int gx = 0; gx < c.min_grid; ++gx)
        for (int t = 0; t < RNG_BLOCK; ++t) {
            const int64_t r = (int64_t)gx * RNG_BLOCK + t;
            if (r >= m) continue;
            for (int rb = 0; rb < c.rhs_blocks; ++rb) sink += rparts[(size_t)rb * (size_t)m + (size_t)r];
            ++rout_m[(size_t)r];
        }
    for (int v : rout_m) CHECK(v == 1);
    CHECK(sink > 0.0 || cnt == 0 || m == 0);
    std::printf("m=%lld n=%lld L=%lld: cost %d row blocks x %d column tiles, %zu partials; rhs %d x %d workgroups, %zu "
                "partials\n", (long long)m, (long long)n, (long long)L, c.row_blocks, c.col_tiles, c.cparts, c.rhs_grid_x,
                c.rhs_blocks, c.rparts);
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
