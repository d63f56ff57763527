// spx_dual.h — the dual simplex loop's kernels (spx_dual.hip): one rank,
// explicit B^-1 (Params::win == 0, in-place storage).  DESIGN.md §7d.
//
// A dual pass at iteration it is three launches on the context's stream; the
// kernel boundaries are the only ordering between them:
//   k_dual_step    one workgroup.  Finishes the pivot the previous pass left
//                  in DualRec (x_b -= theta alpha, x_b[q] = theta, y -= (d_p /
//                  alpha_q) rho, basis bookkeeping, iter + 1), then picks the
//                  leaving row q = argmin x_b[i] over x_b[i] < -feas_tol (none:
//                  ST_OPTIMAL), forms the pivot row rho = row q of the true
//                  B^-1 and stages the pending pivot's row into Params::rbuf.
//   k_dual_price   the dual ratio test: for every non-basic column j on
//                  nb_list a_j = rho.A_j and d_j = y.A_j - c_j (rho and y in
//                  LDS), candidates a_j < -piv_tol, key max(d_j, 0) / -a_j,
//                  argmin (smallest column on ties) per workgroup.
//   k_dual_update  every workgroup reduces k_dual_price's partials (no
//                  candidate: ST_INFEASIBLE), then FTRAN fused with the pending
//                  rank-1 update exactly as k_update's explicit pass: row i of
//                  B^-1 is read once, the pending pivot applied, written once
//                  and dotted with A_p.
// The B^-1 state keeps the primal loop's convention (spx_device.h): P.B0 = S =
// B^-1 before the last pivot, whose (st->q, st->aq, alpha[iter & 1]) are
// pending; x_b and y are always current after k_dual_step (y_applied =
// xb_applied = iter), so k_flush has nothing to do, k_materialize applies the
// pending pivot, and a primal pass can follow a dual one and vice versa.
//
// Dual steepest-edge pricing (SPX_DUAL_PRICING_STEEPEST) runs the same three
// launches in their steepest-edge instantiations: k_dual_update<., SE> also
// dots every updated row with rho (tau) and with itself (wex, the exact weight
// before the pivot), k_dual_step_se's commit turns them into the weights after
// the pivot (DualSeArgs::w) and its selection takes argmin -x_b^2 / w.
// k_dual_norms recomputes w from B^-1 where no pass has kept it.
//
// Boxed variables 0 <= x <= u (spx_set_bounds) run k_dual_step_box /
// k_dual_step_se_box and k_dual_price<., true>: the selection takes the two-sided
// violation delta and leaves its side s in DualRec, the ratio test flips a_j and
// d_j by s and sigma_j (DualBoxArgs::at_upper), the commit starts the entering
// column from the bound it sat at and keeps at_upper / ub_B with the basis.
// k_dual_update and k_dual_norms are shared: alpha, tau and wex do not depend on
// bounds.  P.b is then the effective right-hand side (k_box_rhs).  A context
// with no finite bound launches the unboxed kernels only.
//
// The bound-flipping (long-step) ratio test (SPX_DUAL_RATIO_LONG_STEP, boxed
// contexts only) makes a pass five launches:
//   k_dual_step_long / k_dual_step_se_long   as above; the commit also takes the
//                  flipped columns' B^-1 v (DualLongArgs::fl) off x_b.
//   k_dual_price<., ., true>   the boxed ratio test, which also stores every list
//                  slot's record: key, u_j (-ahat_j), d_j.
//   k_dual_long    one workgroup: merges the partials and walks the candidates in
//                  (key, column) order with slope |delta_q|; a bounded candidate
//                  whose u_j (-ahat_j) leaves the slope > 0 is flipped, the first
//                  other one enters (p, d_p into DualRec; none: ST_INFEASIBLE,
//                  nothing flipped).  Leaves the flip list and the counters.
//   k_dual_flips   returns at once without flips; else v = sum_F dx_j A_j in the
//                  list's order (one thread per row), P.b -= v, at_upper toggled.
//   k_dual_update<., ., true>   takes p from DualRec and, when the pass has flips,
//                  also dots every updated row with v into fl.
// Without a flip every value is the textbook boxed pass's, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "spx_device.h"

namespace spx {

struct alignas(16) DualPartial {  // a k_dual_price workgroup's candidate
    double key;
    int64_t idx;  // entering column, INT64_MAX when none
    double a;     // rho . A_idx
    double d;     // y . A_idx - c_idx
};

struct alignas(16) DualRec {  // the pass in flight
    int64_t q;      // leaving row (k_dual_step)
    int64_t p;      // entering column (k_dual_update)
    double d_p;     // its reduced cost
    int32_t fresh;  // 1: k_dual_update ran the FTRAN, the pivot awaits k_dual_step
    int32_t s;      // boxed passes: +1 the row leaves to its lower bound, -1 to its upper bound
};

struct DualArgs {
    double* rho;         // L: the pivot row
    DualPartial* parts;  // price_grid
    DualRec* rec;
    int32_t price_grid;
    int32_t pad;
    double feas_tol;
    double piv_tol;
};

// the steepest-edge instantiations' arguments (the Dantzig ones take DualArgs
// alone: their kernel arguments are what they were before the rule existed)
struct DualSeArgs : DualArgs {
    double* tau;  // L: row_i . rho of the pass in flight (k_dual_update<., SE>)
    double* wex;  // L: row_i . row_i of the pass in flight, B^-1 before its pivot
    double* w;    // L: the weights of the current basis (k_dual_step_se, k_dual_norms)
};

// the boxed instantiations' arguments (0 <= x <= u; a context with no finite
// bound never launches them)
struct DualBoxArgs : DualSeArgs {
    const double* ub;   // n: upper bounds, +inf = none
    double* ub_B;       // L: the bound of row i's basic column (ub[b_ixs[i]])
    int8_t* at_upper;   // n: 1 = the non-basic column sits at its upper bound
};

struct alignas(16) DualLongRec {  // the long-step pass in flight (k_dual_long) and its counters
    int32_t nflip;     // columns this pass flips (0: fl and v are not read)
    int32_t pad;
    int64_t flips;     // columns flipped since create / spx_reset
    int64_t passes;    // passes with at least one flip
    int64_t max_pass;  // the largest flip count of one pass
};

struct alignas(16) DualFlip {  // one flipped column, in the walk's order
    int64_t j;
    double dx;  // +u_j from lower to upper, -u_j back
};

// the long-step instantiations' arguments (boxed contexts under SPX_DUAL_RATIO_LONG_STEP)
struct DualLongArgs : DualBoxArgs {
    double* rkey;       // n: list slot s: the candidate's key, +inf when nb_list[s] is none
    double* rcd;        // 2 n: (u_j (-ahat_j), d_j) of the slot's column
    DualFlip* flist;    // n
    double* v;          // L: sum over the flipped columns of dx_j A_j
    double* fl;         // L: B^-1 v (k_dual_update<., ., true>)
    DualLongRec* lrec;
    int32_t walk_global;  // 1: k_dual_long reads the keys from global memory every round (its path beyond
    int32_t pad2;         //    16,384 list slots, forced: SPX_DUAL_LONG_GLOBAL=1)
};

struct DualCfg {
    int price_grid = 0;
    bool price_lds = false;  // rho and y staged in LDS (2 * 8 * L bytes) or read from global
    int update_grid = 0;
    bool update_lds = false;  // the pending row and A_p staged in LDS
    bool se_update_lds = false;  // k_dual_update<., SE>: its operands staged in LDS (24 L bytes must fit)
    bool se_rho_lds = false;     // ... rho among them (24 L bytes of LDS), or read from global memory (16 L)
};

constexpr int DUAL_BLOCK = 512;  // threads per workgroup of k_dual_price / k_dual_update
constexpr int DUAL_WAVES = DUAL_BLOCK / 64;
constexpr double DUAL_W_FLOOR = 1e-300;  // steepest-edge weights stay positive: the key -x_b^2 / w stays finite

// geometry: price_grid_opt > 0 fixes the pricing grid, global_y keeps rho and y
// (and the steepest-edge update's operands) in global memory; lds_cap_opt > 0
// lowers the bytes of LDS a staged layout may take (tests: SPX_DUAL_LDS_CAP), it
// never raises them
hipError_t dual_prepare(const Params& P, int cus, int price_grid_opt, bool global_y, bool se_rho_lds,
                        size_t lds_cap_opt, DualCfg* cfg);
// se: the steepest-edge instantiations (leaving row by -x_b^2 / w, weights kept in D.w)
// box: the boxed instantiations (two-sided leaving rows, sigma_j in the ratio test)
hipError_t launch_dual_step(const Params& P, const DualBoxArgs& D, bool se, bool box, bool finish_only, hipStream_t s);
// the long-step pass (boxed): the step and price instantiations above with the
// flips, then k_dual_long + k_dual_flips (one timed span e0..e1), then the update
hipError_t launch_dual_step_long(const Params& P, const DualLongArgs& D, bool se, bool finish_only, hipStream_t s);
hipError_t launch_dual_price_long(const Params& P, const DualLongArgs& D, const DualCfg& c, hipStream_t s,
                                  hipEvent_t e0, hipEvent_t e1);
hipError_t launch_dual_long(const Params& P, const DualLongArgs& D, hipStream_t s);
hipError_t launch_dual_flips(const Params& P, const DualLongArgs& D, double* b_eff, hipStream_t s);
hipError_t launch_dual_update_long(const Params& P, const DualLongArgs& D, const DualCfg& c, bool se, hipStream_t s,
                                   hipEvent_t e0, hipEvent_t e1);
hipError_t launch_dual_price(const Params& P, const DualBoxArgs& D, const DualCfg& c, bool box, hipStream_t s,
                             hipEvent_t e0, hipEvent_t e1);
hipError_t launch_dual_update(const Params& P, const DualSeArgs& D, const DualCfg& c, bool se, hipStream_t s,
                              hipEvent_t e0, hipEvent_t e1);
// D.w = squared row norms of the true B^-1 (pending pivot applied in registers)
hipError_t launch_dual_norms(const Params& P, const DualSeArgs& D, const DualCfg& c, hipStream_t s);

// b_eff = b_user - sum over the non-basic columns at upper of u_j A_j (ascending
// j, one thread per row: no atomics), and D.ub_B from b_ixs
hipError_t launch_box_rhs(const Params& P, const DualBoxArgs& D, const double* b_user, double* b_eff, hipStream_t s);
// shifted variables x' = x - l (D.ub = u - l, lsh = n lower bounds,
// 0 where none): b_eff = b_user - A lsh - the at-upper sum, the columns with
// lsh[j] != 0 or at upper only, ascending j, no atomics; D.ub_B as above
hipError_t launch_box_rhs_lu(const Params& P, const DualBoxArgs& D, const double* lsh, const double* b_user,
                             double* b_eff, hipStream_t s);
// x_b = (true B^-1) P.b, the pending pivot applied in registers (k_dual_norms' form)
hipError_t launch_box_xb(const Params& P, const DualCfg& c, hipStream_t s);

}  // namespace spx
