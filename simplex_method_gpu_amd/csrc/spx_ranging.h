// spx_ranging.h — sensitivity ranging at the optimum (spx_ranging.hip; host side
// spx_api_ranging.cpp): how far one cost coefficient or one
// right-hand side may move before the optimal basis changes, and what blocks.
// Conventions are the bounded loops' (spx_pbox.h): maximise c.x, d = y.A - c,
// sigma_k = +1 for a non-basic column at its lower bound and -1 at its upper,
// optimal means sigma_k d_k >= 0.  Every result is a non-negative delta, +inf
// where nothing blocks, with the index of what blocks (-1: nothing).
//
// All kernels read R.S = the true B^-1 of the basis (m x L row-major, nothing
// pending: the host materialises it first; no kernel here applies an eta) and
// R.d = y.A - c for all n columns (k_reduced_costs).  Ordering is by kernel
// boundaries only; every reduction is a minimum under a total order (value,
// then index), so no result depends on a tile or block order; no atomics.
//   k_rng_gather    per nb_list slot s (column k): sig[s] = sigma_k (0: free),
//                  sk[s] = max(sigma_k d_k, 0) (0 for a free column), col[s] = k;
//                  and the non-basic column's own cost range: at lower up = s_k,
//                  at upper down = s_k, the other side +inf; free: both 0.
//   k_rng_cost      T = S A_N tile by tile: k_pbox_wexact's tiling and K loop
//                  (128 rows x 128 slots per workgroup, four 64 x 64 wave
//                  quadrants of 4 x 4 v_mfma_f64_16x16x4_f64 accumulators, 16-wide
//                  K chunks double-buffered in LDS at pitch 18, zeros without a
//                  load past m and past the list).  A non-basic slack column goes
//                  through the tiles like any other: its unit column is streamed
//                  from A, so T_ik is B^-1[i, r] exactly (products with 0 add
//                  nothing).  Epilogue, per accumulator element: g = sigma_k T_ik
//                  (free: T_ik), for |g| > piv_tol the ratio s_k / |g| with the
//                  key (ratio, k): g < 0 blocks "up", g > 0 blocks "down", a free
//                  column both at 0.  Two running minima per row, merged across
//                  the lane's four tiles, the 16 lanes of a row (xor 1, 2, 4, 8)
//                  and the two column halves (LDS); one RngPart per (column
//                  tile, row), plain stores.
//   k_rng_cost_min  per row i the column tiles' partials merged by key, scattered
//                  to down / up / block_* [b_ixs[i]].
//   k_rng_rhs       one stream over S: workgroup (x, y) owns columns [256 x, 256 x
//                  + 256) of S and rows [64 y, 64 y + 64); x_b (clamped into [0,
//                  ub_B]), ub_B and "row's basic column is free" staged in LDS once;
//                  a lane owns column r and walks the rows ascending: beta =
//                  S[i, r]; beta > tol blocks "down" at x_i / beta (side 0) and,
//                  ub_B[i] finite, "up" at (ub_B[i] - x_i) / beta (side 1); beta <
//                  -tol blocks "up" at x_i / -beta (side 0) and, ub_B[i] finite,
//                  "down" at (ub_B[i] - x_i) / -beta (side 1); a free row never
//                  blocks.  Key (ratio, 2 i + side).  One RngPart per (row block, r).
//   k_rng_rhs_min   per r the row blocks' partials merged by key.
// The geometry is a function of m and n alone: no tuning option reaches it.
#pragma once
#include <hip/hip_runtime.h>

#include "spx_device.h"

namespace spx {

constexpr int RNG_BLOCK = 256;     // threads per workgroup of every kernel here
constexpr int RNG_TILE = 128;      // rows of S and list slots per k_rng_cost workgroup
constexpr int RNG_KC = 16;         // doubles of k per staged chunk
constexpr int RNG_LD = RNG_KC + 2; // LDS row pitch (doubles): conflict-free fragment reads
constexpr int RNG_ROWS = 64;       // rows of S per k_rng_rhs workgroup

struct alignas(16) RngPart {  // two keyed minima: (down, kdown) and (up, kup); k = -1: none (+inf)
    double down;
    double up;
    int64_t kdown;
    int64_t kup;
};

struct RngCfg {
    int row_blocks = 0;   // k_rng_cost: blocks of RNG_TILE rows: ceil(m / 128)
    int col_tiles = 0;    // tiles of RNG_TILE list slots: ceil((n - m) / 128)
    int gather_grid = 0;  // blocks of RNG_BLOCK list slots
    int min_grid = 0;     // k_rng_cost_min / k_rng_rhs_min: blocks of RNG_BLOCK rows (columns of S)
    int rhs_grid_x = 0;   // k_rng_rhs: blocks of RNG_BLOCK columns of S
    int rhs_blocks = 0;   // blocks of RNG_ROWS rows: ceil(m / 64)
    int64_t cap = 0;      // list slots: n - m
    size_t cparts = 0;    // RngPart: col_tiles x m
    size_t rparts = 0;    // RngPart: rhs_blocks x m
};

inline RngCfg rng_geometry(int64_t m, int64_t n) {
    RngCfg c;
    c.cap = n - m;
    c.row_blocks = (int)((m + RNG_TILE - 1) / RNG_TILE);
    c.col_tiles = (int)((c.cap + RNG_TILE - 1) / RNG_TILE);
    c.gather_grid = (int)((c.cap + RNG_BLOCK - 1) / RNG_BLOCK);
    c.min_grid = (int)((m + RNG_BLOCK - 1) / RNG_BLOCK);
    c.rhs_grid_x = c.min_grid;
    c.rhs_blocks = (int)((m + RNG_ROWS - 1) / RNG_ROWS);
    c.cparts = (size_t)c.col_tiles * (size_t)m;
    c.rparts = (size_t)c.rhs_blocks * (size_t)m;
    return c;
}

struct RngArgs {
    const double* S;         // m x L: the true B^-1
    const double* d;         // n: y.A - c
    const int8_t* at_upper;  // n, or nullptr: every non-basic column at lower
    const int8_t* is_free;   // n, or nullptr: no free column
    const double* ub_B;      // L, or nullptr: no bound on any basic column
    double* sk;              // cap: s_k per list slot
    double* sig;             // cap: sigma_k per list slot, 0 = free
    int32_t* col;            // cap: the slot's column
    RngPart* cparts;         // col_tiles x m
    RngPart* rparts;         // rhs_blocks x m
    double* c_down;          // n: cost ranges
    double* c_up;
    int64_t* c_kdown;        // n: blocking columns
    int64_t* c_kup;
    double* r_down;          // m: right-hand-side ranges
    double* r_up;
    int64_t* r_kdown;        // m: 2 row + side
    int64_t* r_kup;
    int64_t cap;
    int32_t col_tiles;
    int32_t rhs_blocks;
    double tol;              // opts.piv_tol
};

hipError_t rng_prepare();  // once per process and device: k_rng_cost's LDS size
hipError_t launch_rng_cost(const Params& P, const RngArgs& R, const RngCfg& c, hipStream_t s);
hipError_t launch_rng_rhs(const Params& P, const RngArgs& R, const RngCfg& c, hipStream_t s);

}  // namespace spx
