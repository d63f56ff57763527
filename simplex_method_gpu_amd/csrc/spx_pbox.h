// spx_pbox.h — the bounded primal simplex loop's kernels (spx_pbox.hip): 0 <= x
// <= u, one rank, explicit B^-1 (Params::win == 0, in-place storage), Dantzig
// entering column.  DESIGN.md §7e.
//
// A pass at iteration it is three launches on the context's stream; the kernel
// boundaries are the only ordering between them:
//   k_pbox_price   for every non-basic column j on nb_list d_j = y.A_j - c_j (y
//                  in LDS; a non-basic slack column from y[k] alone), sigma_j =
//                  -1 at its upper bound, candidates sigma_j d_j < -eps, argmin
//                  (smallest column on ties) per workgroup.
//   k_pbox_update  every workgroup reduces k_pbox_price's partials (no
//                  candidate: ST_OPTIMAL), then FTRAN fused with the pending
//                  rank-1 update exactly as k_dual_update: row i of B^-1 is read
//                  once, the pending pivot applied, written once and dotted with
//                  A_p.  The wave that holds alpha_i also forms row i's entry of
//                  the two-sided ratio test from x_b[i], ub_B[i] and sigma_p;
//                  the workgroup reduces its rows to one partial (t, row, side).
//   k_pbox_step    one workgroup.  Merges the ratio partials and decides:
//                    flip      u_p finite and (no row, or u_p <= t_q): x_b -= u_p
//                              ahat, at_upper[p] toggled, P.b -= dx_p A_p; no
//                              pivot, iter unchanged;
//                    unbounded no row and u_p = +inf: ST_UNBOUNDED;
//                    pivot     theta = t_q: x_b -= theta ahat, x_b[q] = (u_p at
//                              upper, else 0) + sigma_p theta, y -= (d_p /
//                              alpha_q) rho, basis bookkeeping with at_upper /
//                              ub_B, trace, iter + 1; rho = row q of B^-1 (as
//                              k_pbox_update left it: B^-1 before this pivot) is
//                              staged into Params::rbuf on the way.
// Every pass ends committed: there is nothing for a closing launch to finish.
//
// The B^-1 state keeps the primal loop's convention (spx_device.h): P.B0 = S =
// B^-1 before the last pivot, whose (st->q, st->aq, alpha[iter & 1]) are
// pending; x_b and y are always current (y_applied = xb_applied = iter).  A
// pass that makes no pivot (flip, unbounded) has still applied the pending
// pivot to S, and iter has not moved: it leaves the "nothing pending" state of
// a reinversion (k_rv_yreduce / k_rv_rows: st->q = 0, st->aq = 1, alpha[iter & 1]
// = e_0, for which every eta entry is 0), so k_materialize, k_flush, the dual
// kernels and the next pass here read S as the true B^-1.
//
// The boxed state (ub, ub_B, at_upper, the caller's b) is the dual loop's
// (DualBoxArgs, spx_ctx.h DualState): the two loops hand a basis to each other.
#pragma once
#include <hip/hip_runtime.h>

#include "spx_device.h"

namespace spx {

struct alignas(16) PboxPartial {  // a k_pbox_price workgroup's candidate
    double key;   // sigma_j d_j
    int64_t idx;  // entering column, INT64_MAX when none
    double d;     // y . A_idx - c_idx
    double pad;
};

struct alignas(16) PboxRec {  // the pass in flight, and the counters
    int64_t p;         // entering column (k_pbox_update)
    double d_p;        // its reduced cost
    int32_t fresh;     // 1: k_pbox_update ran the FTRAN, the pass awaits k_pbox_step
    int32_t pad;
    int64_t flips;     // flip passes since create / spx_reset
    int64_t to_upper;  // pivots whose leaving column went to its upper bound
    int64_t pad2;
};

struct PboxArgs {
    PboxPartial* parts;   // price_grid
    ArgMinEntry* rparts;  // update_grid: (t, 2 row + side), side 1 = the row leaves to its upper bound
    PboxRec* rec;
    const double* ub;     // n: upper bounds, +inf = none
    double* ub_B;         // L: the bound of row i's basic column
    int8_t* at_upper;     // n: 1 = the non-basic column sits at its upper bound
    double* b_eff;        // L: Params::b, the effective right-hand side
    int32_t price_grid;
    int32_t update_grid;
    double piv_tol;
};

struct PboxCfg {
    int price_grid = 0;
    bool price_lds = false;   // y staged in LDS (8 L bytes) or read from global memory
    int update_grid = 0;
    bool update_lds = false;  // the pending row and A_p staged in LDS (16 L bytes)
};

constexpr int PBOX_BLOCK = 512;  // threads per workgroup of k_pbox_price / k_pbox_update
constexpr int PBOX_WAVES = PBOX_BLOCK / 64;

// geometry: price_grid_opt > 0 fixes the pricing grid, global_y keeps y in global memory
hipError_t pbox_prepare(const Params& P, int cus, int price_grid_opt, bool global_y, PboxCfg* cfg);
hipError_t launch_pbox_price(const Params& P, const PboxArgs& D, const PboxCfg& c, hipStream_t s, hipEvent_t e0,
                             hipEvent_t e1);
hipError_t launch_pbox_update(const Params& P, const PboxArgs& D, const PboxCfg& c, hipStream_t s, hipEvent_t e0,
                              hipEvent_t e1);
hipError_t launch_pbox_step(const Params& P, const PboxArgs& D, hipStream_t s);
// rbuf = row st->q of S where a pivot is pending (entry from another loop, whose
// last launch does not leave it staged)
hipError_t launch_pbox_stage(const Params& P, hipStream_t s);

}  // namespace spx
