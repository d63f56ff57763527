// spx_bndrange.h — bound ranging at the optimum (spx_bndrange.hip; host side
// spx_api_ranging.cpp): how far one bound of one column may move
// before the optimal basis changes, and what blocks.  Conventions are
// spx_ranging.h's: the shifted variables x' = x - l with ranges ub = u - l, x_i
// the basic values clamped into [0, ub_B[i]], tol = opts.piv_tol; every result
// is a non-negative delta, +inf where nothing blocks, with 2 row + side of the
// row that leaves (side 1: to its upper bound), -1 where nothing blocks, BND_OWN
// (-2) where the moving bound meets the column's own other bound first.
//
// All kernels read B.S = the true B^-1 of the basis (m x L row-major, nothing
// pending: the host materialises it first; no kernel here applies an eta).
// Ordering is by kernel boundaries only; every reduction is a minimum under a
// total order (value, then 2 row + side), so no result depends on a tile or
// block order; no atomics.
//   k_rng_bound_gather  per nb_list slot s (column k): col[s] = k, kind[s] = 0 at
//                  lower / 1 at upper / 2 free, ubj[s] = the column's range ub[k].
//   k_rng_bound    T = S A_N tile by tile: k_rng_cost's tiling and K loop, copied
//                  (128 rows x 128 slots per workgroup, four 64 x 64 wave
//                  quadrants of 4 x 4 v_mfma_f64_16x16x4_f64 accumulators, 16-wide
//                  K chunks double-buffered in LDS at pitch 18, zeros without a
//                  load past m and past the list).  After the K loop's last
//                  barrier the workgroup's 128 rows of clamped x_b, ub_B and
//                  "basic column is free" are staged in the staging buffers.
//                  Epilogue, per accumulator element alpha = T_is of a row that
//                  is not free, |alpha| > tol, a = |alpha|: x_i / a (side 0) blocks
//                  "up" where alpha > 0 and "down" where alpha < 0; ub_B[i] finite,
//                  (ub_B[i] - x_i) / a (side 1) blocks "down" where alpha > 0 and
//                  "up" where alpha < 0: k_rng_rhs's two divisions, with the
//                  directions of x_B(t) = x_B - t alpha.  Two running minima per
//                  slot, merged over the lane's 16 rows, the lanes xor 16 and 32
//                  and the two row halves (LDS); one RngPart per (row block,
//                  slot), plain stores.
//   k_rng_bound_min  per slot the row blocks' partials merged by key; free: both
//                  +inf / -1; else the own-bound cap (at lower "up", at upper
//                  "down": ub_j where strictly smaller, blocker BND_OWN);
//                  scattered to the slot's column.
//   k_rng_bound_basic  per row i the basic column's two slacks: up = x_i (2 i; a
//                  free column: +inf, -1), down = ub_B[i] - x_i (2 i + 1; no upper
//                  bound: +inf, -1).
// The geometry is a function of m and n alone: no tuning option reaches it.
#pragma once
#include <hip/hip_runtime.h>

#include "spx_device.h"
#include "spx_ranging.h"  // RngPart and the tile constants

namespace spx {

constexpr int64_t BND_OWN = -2;  // SPX_RANGING_OWN_BOUND

struct BndCfg {
    int row_blocks = 0;   // k_rng_bound: blocks of RNG_TILE rows: ceil(m / 128)
    int col_tiles = 0;    // tiles of RNG_TILE list slots: ceil((n - m) / 128)
    int slot_grid = 0;    // k_rng_bound_gather / _min: blocks of RNG_BLOCK list slots
    int row_grid = 0;     // k_rng_bound_basic: blocks of RNG_BLOCK rows
    int64_t cap = 0;      // list slots: n - m
    size_t parts = 0;     // RngPart: row_blocks x cap
};

inline BndCfg bnd_geometry(int64_t m, int64_t n) {
    BndCfg c;
    c.cap = n - m;
    c.row_blocks = (int)((m + RNG_TILE - 1) / RNG_TILE);
    c.col_tiles = (int)((c.cap + RNG_TILE - 1) / RNG_TILE);
    c.slot_grid = (int)((c.cap + RNG_BLOCK - 1) / RNG_BLOCK);
    c.row_grid = (int)((m + RNG_BLOCK - 1) / RNG_BLOCK);
    c.parts = (size_t)c.row_blocks * (size_t)c.cap;
    return c;
}

struct BndArgs {
    const double* S;         // m x L: the true B^-1
    const double* ub;        // n ranges, or nullptr: no bound on any column
    const int8_t* at_upper;  // n, or nullptr: every non-basic column at lower
    const int8_t* is_free;   // n, or nullptr: no free column
    const double* ub_B;      // L, or nullptr: no bound on any basic column
    int32_t* col;            // cap: the slot's column
    int32_t* kind;           // cap: 0 at lower, 1 at upper, 2 free
    double* ubj;             // cap: the slot's range
    RngPart* parts;          // row_blocks x cap
    double* down;            // n: bound ranges
    double* up;
    int64_t* kdown;          // n: 2 row + side, -1, BND_OWN
    int64_t* kup;
    int64_t cap;
    int32_t row_blocks;
    double tol;              // opts.piv_tol
};

hipError_t bnd_prepare();  // once per process and device: k_rng_bound's LDS size
hipError_t launch_rng_bound(const Params& P, const BndArgs& B, const BndCfg& c, hipStream_t s);

}  // namespace spx
