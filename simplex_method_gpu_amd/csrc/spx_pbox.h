// spx_pbox.h — the bounded primal simplex loop's kernels (spx_pbox.hip): 0 <= x
// <= u, one rank, explicit B^-1 (Params::win == 0, in-place storage), Dantzig
// entering column, or exact steepest edge (the *_se kernels at the end of this
// file; through phase 1 with the *_se1 kernels, §7l; with free
// columns with the *_se_f kernels, §7m).  DESIGN.md §7e.
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

// Phase 1: the device phase word and the phase-1 counters.
// Written by one-workgroup kernels only (k_pbox_step1, k_pbox_classify) and by
// stream-ordered host memsets, so every kernel of a pass reads one value.
struct alignas(16) PboxPhase {
    int32_t ninf;     // rows out of their bounds as of the last classification: > 0 makes the next pass a phase-1 pass
    int32_t y_stale;  // 1: a phase-1 pivot was made since y = c_B B^-1 was last current
    int64_t passes;   // phase-1 passes since create / spx_reset, flip passes included
    int64_t pivots;   // phase-1 pivots
    int64_t ninf0;    // ninf at the last entry check
    int64_t pad;
};

struct Pbox1Args {  // what the phase-1 capable kernels take beside PboxArgs
    PboxPhase* ph;
    double* w;           // L: +1 below, -1 above, 0 feasible (rows m..L-1: 0)
    double* yp;          // L: w B^-1, the phase-1 pricing vector
    double* vparts;      // vtb_blocks x L: k_pbox_vtb's per-row-block partial vectors
    int32_t vtb_blocks;  // row blocks of PBOX_VTB_ROWS rows
    int32_t force;       // 1: a readback's refresh of y (ignores status and limit, rebuilds y iff y_stale)
    double feas_tol;
};

struct PboxCfg {
    int price_grid = 0;
    bool price_lds = false;   // y staged in LDS (8 L bytes) or read from global memory
    int update_grid = 0;
    bool update_lds = false;  // the pending row and A_p staged in LDS (16 L bytes)
    // k_pbox_vtb: a function of m alone (the result must not depend on tuning options)
    int vtb_grid_x = 0;       // column slabs of PBOX_VTB_WAVES 1 KiB chunks
    int vtb_blocks = 0;       // row blocks
    int vsum_grid = 0;
};

constexpr int PBOX_BLOCK = 512;  // threads per workgroup of k_pbox_price / k_pbox_update
constexpr int PBOX_WAVES = PBOX_BLOCK / 64;
constexpr int PBOX_VTB_BLOCK = 256;  // k_pbox_vtb / k_pbox_vtb_sum
constexpr int PBOX_VTB_WAVES = PBOX_VTB_BLOCK / 64;
constexpr int PBOX_VTB_ROWS = 64;    // rows of S per k_pbox_vtb workgroup

// geometry: price_grid_opt > 0 fixes the pricing grid, global_y keeps y in global memory; lds_cap_opt > 0 lowers
// the bytes of LDS a staged layout may take (tests: SPX_PBOX_LDS_CAP), it never raises them
hipError_t pbox_prepare(const Params& P, int cus, int price_grid_opt, bool global_y, size_t lds_cap_opt, PboxCfg* cfg);
hipError_t launch_pbox_price(const Params& P, const PboxArgs& D, const PboxCfg& c, hipStream_t s, hipEvent_t e0,
                             hipEvent_t e1);
hipError_t launch_pbox_update(const Params& P, const PboxArgs& D, const PboxCfg& c, hipStream_t s, hipEvent_t e0,
                              hipEvent_t e1);
hipError_t launch_pbox_step(const Params& P, const PboxArgs& D, hipStream_t s);
// rbuf = row st->q of S where a pivot is pending (entry from another loop, whose
// last launch does not leave it staged)
hipError_t launch_pbox_stage(const Params& P, hipStream_t s);

// Phase 1.  A pass enqueued while the host last saw ninf > 0 or
// y stale is four steps, again ordered by kernel boundaries only:
//   k_pbox_vtb + k_pbox_vtb_sum   ninf > 0: yp = w B^-1; ninf == 0 and y stale:
//                  y = c_B B^-1; else nothing.  B^-1 = S with the pending pivot:
//                  v B^-1 = v' S, v' = v but v'_q = v_q + sum_i v_i E_i (one
//                  m-dot, computed by the workgroups whose row block holds q).
//                  Workgroup (x, y) owns PBOX_VTB_WAVES 1 KiB column chunks of
//                  row block y; it lists the block's rows with v'_i != 0 (one
//                  ballot) and streams those only, lanes own columns (dbl2).
//                  k_pbox_vtb_sum adds the row blocks' partial vectors in a
//                  fixed order (four ascending quarters, then lane-wise):
//                  no floating-point atomics.
//   k_pbox_price1 / k_pbox_update1 / k_pbox_step1   k_pbox_price / _update /
//                  _step with the phase read from PboxPhase::ninf.  Phase 1:
//                  d_j = yp.A_j (no c_j); no candidate: ST_INFEASIBLE; a below
//                  row blocks only for ahat_i < -piv_tol at x_b / ahat_i (side
//                  0), an above row only for ahat_i > piv_tol at (x_b - u_k) /
//                  ahat_i (side 1); no row and u_p = +inf: ST_BREAKDOWN; y is
//                  not updated by a pivot (y_stale = 1); the commit classifies
//                  all rows again (w, ninf) and bumps the counters.  Phase 2
//                  (ninf == 0): the arithmetic of the three plain kernels, so a
//                  batch enqueued in phase 1 runs on through the switch; the
//                  first such pass's k_pbox_step1 clears y_stale.
// k_pbox_classify (one workgroup): w and ninf from x_b and ub_B, at entry (also
// ninf0) and after a reinversion.
hipError_t launch_pbox_vtb(const Params& P, const Pbox1Args& X, const PboxCfg& c, hipStream_t s, hipEvent_t e0,
                           hipEvent_t e1);
hipError_t launch_pbox_price1(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxCfg& c, hipStream_t s,
                              hipEvent_t e0, hipEvent_t e1);
hipError_t launch_pbox_update1(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxCfg& c, hipStream_t s,
                               hipEvent_t e0, hipEvent_t e1);
hipError_t launch_pbox_step1(const Params& P, const PboxArgs& D, const Pbox1Args& X, hipStream_t s);
hipError_t launch_pbox_classify(const Params& P, const PboxArgs& D, const Pbox1Args& X, bool entry, hipStream_t s);

// Free columns: -inf < x_j < +inf.  A context that holds one runs
// every pass on the *_f kernels: k_pbox_price1 / _update1 / _step1 (which read
// the phase from the device, so one set covers both phases) with two more
// facts, "column j is free" and "row i's basic column is free":
//   k_pbox_price_f   is_free[j] read per column beside at_upper[j], ahead of the
//                  column's stream; a non-basic free column sits at 0, is a
//                  candidate when |d_j| > eps and its key is -|d_j|.  The dot is
//                  k_pbox_price's: d_j does not depend on the grid or on where y
//                  is read from.
//   k_pbox_update_f  sigma_p of a free entering column is +1 for d_p < 0, else -1
//                  (d_p from the merged partial).  lb_B[i] is requested ahead of
//                  the stream with x_b[i], ub_B[i] and w[i]; a feasible row
//                  enters the ratio test to its lower bound only where lb_B[i] is
//                  finite, so a row whose basic column is free (ub_B = +inf too)
//                  never blocks.
//   k_pbox_step_f    a free entering column has u_p = +inf: it never flips, no row
//                  is ST_UNBOUNDED (phase 1: ST_BREAKDOWN), a pivot puts x_b[q] =
//                  sigma_p theta.  The commit stores lb_B[q] (-inf for a free
//                  entering column, else 0) beside ub_B[q]; rows are classified
//                  with both, so a free basic row has w_i = 0 and is not counted.
//                  A leaving column is never free.
//   k_pbox_classify_f  k_pbox_classify with lb_B.
// Same grids and LDS sizes as the kernels they derive from (pbox_prepare's
// PboxCfg); ordering by kernel boundaries only, no floating-point atomics.
struct PboxFreeArgs {
    const int8_t* is_free;  // n: 1 = the column is free
    double* lb_B;           // L: the lower bound of row i's basic column, 0 or -inf (rows m..L-1: 0)
};

hipError_t pbox_free_prepare(const Params& P, const PboxCfg& c);  // the LDS sizes of the staged instantiations
hipError_t launch_pbox_price_f(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxFreeArgs& F,
                               const PboxCfg& c, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
hipError_t launch_pbox_update_f(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxFreeArgs& F,
                                const PboxCfg& c, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
hipError_t launch_pbox_step_f(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxFreeArgs& F,
                              hipStream_t s);
hipError_t launch_pbox_classify_f(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxFreeArgs& F,
                                  bool entry, hipStream_t s);

// Steepest edge: gamma_j = 1 + ||B^-1 A_j||^2 for the non-basic
// columns, entering column argmin -d_j^2 / gamma_j over the candidates.  A pass
// is four steps, ordered by kernel boundaries only:
//   k_pbox_price_se  k_pbox_price's stream with three operands: per streamed
//                  column y.A_j, rho.A_j and tau.A_j (same per-lane order, one
//                  butterfly each).  While PboxSeRec::pend is set the wave
//                  first applies the last pivot's recurrence g = (rho.A_j) /
//                  alpha_q, gamma_j = max(gamma_j - 2 g (tau.A_j) + g^2 gamma_p,
//                  1 + g^2) and stores gamma_j (one owner per column; the
//                  leaving column, whose weight the commit wrote, is skipped);
//                  then key = -d_j^2 / gamma_j.  The partial is (key, j, d_j):
//                  k_pbox_update merges it unchanged.
//   k_pbox_update  as in a Dantzig pass.
//   k_pbox_step_se k_pbox_step; a pivot also reduces gamma_p = 1 + ||alpha||^2
//                  in a fixed order, writes gamma_leave = max(gamma_p /
//                  alpha_q^2, 1), and records the pending update with its own
//                  copy of rho (rbuf is not kept across a reinversion): alpha_q,
//                  gamma_p, the leaving column, pend = 1, need_tau = 1.  A flip,
//                  an unbounded pass and an optimum clear pend; a pass cut off
//                  by the limit leaves it for the next spx_iterate.
//   k_pbox_tau + k_pbox_tau_sum   tau = alpha^T S, k_pbox_vtb's geometry and
//                  summation order (a function of m alone) with v = the alpha
//                  k_pbox_update wrote and no pending correction: after
//                  k_pbox_update S is B^-1 before the pivot just committed.
//                  Both return at once unless need_tau is set.
// k_pbox_se_init: gamma_j = 1 + ||A_j||^2, one wave per column in the pricing
// dots' summation order.  launch_pbox_price_se(apply = true) applies a pending
// recurrence outside a pass (weight readback) whatever the status; the host
// clears pend behind it with a stream-ordered memset.
struct alignas(16) PboxSeRec {
    int32_t pend;      // 1: gamma awaits the recurrence of the pivot recorded here
    int32_t need_tau;  // 1: the last k_pbox_step_se made a pivot (k_pbox_tau runs)
    int64_t leave;     // the pivot's leaving column
    double aq;         // alpha_q
    double gp;         // gamma_p = 1 + ||alpha||^2
};

struct PboxSeArgs {
    PboxSeRec* se;
    double* gamma;       // n
    double* rho;         // L: row q of B^-1 before the pending pivot
    double* tau;         // L: alpha^T B^-1, the same B^-1
    double* tparts;      // vtb_blocks x L: k_pbox_tau's per-row-block partial vectors
    int32_t vtb_blocks;
    int32_t apply;       // 1: apply a pending recurrence only (ignores status and limit, no pricing)
};

struct PboxSeCfg {
    int lds_vecs = 0;  // vectors of k_pbox_price_se staged in LDS: 0 none, 1 y (rho and tau from L2), 3 all
    int price_grid = 0;
    int init_grid = 0;
};

// lds_vecs_opt: -1 the default (3), else 0 / 1 / 3; lowered to 1, then 0, when the vectors do not fit, and 0
// under global_y; price_grid as PboxCfg's, lds_cap_opt as pbox_prepare's
hipError_t pbox_se_prepare(const Params& P, int cus, int price_grid, bool global_y, int lds_vecs_opt, size_t lds_cap_opt,
                           PboxSeCfg* cfg);
hipError_t launch_pbox_se_init(const Params& P, const PboxSeArgs& E, const PboxSeCfg& c, hipStream_t s);
hipError_t launch_pbox_price_se(const Params& P, const PboxArgs& D, const PboxSeArgs& E, const PboxSeCfg& c, bool apply,
                                hipStream_t s, hipEvent_t e0, hipEvent_t e1);
hipError_t launch_pbox_step_se(const Params& P, const PboxArgs& D, const PboxSeArgs& E, hipStream_t s);
hipError_t launch_pbox_tau(const Params& P, const PboxSeArgs& E, const PboxCfg& c, hipStream_t s, hipEvent_t e0,
                           hipEvent_t e1);

// Steepest edge through phase 1 (opt-in, spx_set_primal_phase_one_pricing).
// The weights depend on the basis alone, so a phase-1 pass keys its candidates
// with them and every pivot of either phase records the same update.  A pass
// enqueued while the host last saw ninf > 0 or y stale is five steps, ordered by
// kernel boundaries only:
//   k_pbox_vtb + k_pbox_vtb_sum   as in a phase-1 Dantzig pass (yp, or y at the switch).
//   k_pbox_price_se1 k_pbox_price_se with the phase read from PboxPhase::ninf:
//                  phase 1 takes yp as its first operand and no c_j, phase 2 y
//                  and c_j; rho.A_j, tau.A_j, the recurrence under the pending
//                  word, the one owner's store of gamma_j, the skipped leaving
//                  column, the per-lane order and the three LDS layouts
//                  (PboxSeCfg::lds_vecs) are k_pbox_price_se's.  No apply-only
//                  mode: a weight readback launches k_pbox_price_se.
//   k_pbox_update1 unchanged, on the steepest-edge pricing grid (it merges on
//                  (key, column) only).
//   k_pbox_step_se1  k_pbox_step1's decisions and commit (classification, ninf,
//                  y_stale, the counters) with k_pbox_step_se's extras on a
//                  pivot: gamma_p in the same fixed order, gamma_leave, the
//                  record with its own rho, pend and need_tau.  pend is cleared
//                  by a flip, ST_INFEASIBLE, ST_BREAKDOWN, ST_UNBOUNDED and an
//                  optimum; a pass cut off by the limit leaves it.
//   k_pbox_tau + k_pbox_tau_sum   unchanged.
// With ninf == 0 and y current the two kernels do the arithmetic of
// k_pbox_price_se and k_pbox_step_se, so a batch enqueued in phase 1 runs on
// through the switch; the host returns to §7h's four-step pass afterwards.
hipError_t pbox_se1_prepare(const Params& P, const PboxSeCfg& c);  // the LDS sizes of the staged instantiations
hipError_t launch_pbox_price_se1(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxSeArgs& E,
                                 const PboxSeCfg& c, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
hipError_t launch_pbox_step_se1(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxSeArgs& E,
                                hipStream_t s);

// Steepest edge with free columns (opt-in, spx_set_primal_free_pricing).
// gamma_j depends on the basis alone and the recurrence reads no bound, so §7j's
// free rule changes only who is a candidate.  A pass enqueued while the host
// last saw ninf > 0 or y stale is vtb -> price_se_f -> update_f -> step_se_f ->
// tau, else the same without vtb; ordered by kernel boundaries only:
//   k_pbox_price_se_f  k_pbox_price_se1 with is_free[j] read per column beside
//                  at_upper[j], ahead of the column's stream: the candidate test
//                  is k_pbox_price_f's ((fr ? -|d| : sigma d) < -eps), the key is
//                  -d_j^2 / gamma_j.  The dots, the recurrence under the pending
//                  word, the one owner's store of gamma_j, the skipped leaving
//                  column, the slack shortcut, the per-lane order and the three
//                  LDS layouts are k_pbox_price_se1's.  The phase word is 0 on a
//                  context without phase 1: one kernel serves both.
//   k_pbox_update_f  unchanged, on the steepest-edge pricing grid: it derives a
//                  free entering column's sigma_p from the partial's d.
//   k_pbox_step_se_f k_pbox_step_f's decisions and commit (lb_B[q], row_class_f,
//                  ninf, y_stale, the counters; a free entering column never
//                  flips) with k_pbox_step_se1's extras on a pivot and its
//                  clearing of pend.  The leaving column is never free.
//   k_pbox_tau + k_pbox_tau_sum   unchanged.
hipError_t pbox_se_f_prepare(const Params& P, const PboxSeCfg& c);  // the LDS sizes of the staged instantiations
hipError_t launch_pbox_price_se_f(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxSeArgs& E,
                                  const PboxFreeArgs& F, const PboxSeCfg& c, hipStream_t s, hipEvent_t e0,
                                  hipEvent_t e1);
hipError_t launch_pbox_step_se_f(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxSeArgs& E,
                                 const PboxFreeArgs& F, hipStream_t s);

// Phase 1's long-step ratio test (opt-in,
// spx_set_primal_phase_one_ratio).  A pass enqueued while the host last saw
// ninf > 0 or y stale gets one more launch between the update and the step
// kernel, under any of the four phase-1 capable pass shapes:
//   k_pbox_long1<FREE>  one workgroup.  Returns at once under the step kernels'
//                  return conditions and when ninf == 0.  Reads this pass's
//                  alpha, x_b, ub_B (FREE: lb_B), w, the pass record and
//                  at_upper[p]; forms every row's soft breakpoint (an infeasible
//                  row reaches the bound it violates: the update kernels' entry)
//                  and hard breakpoint (a feasible row's entry, or the far bound
//                  of a row with a soft one), h = the hard minimum, and walks the
//                  soft breakpoints before h in (t, 2 row + side) order from
//                  slope = sigma_p d_p, adding |ahat_i|: the first with slope >=
//                  -eps leaves, else h, else the last soft one.  The soft
//                  breakpoints are compacted into LDS (PBOX_LONG_CAP entries of
//                  (t, idx, |ahat|), 48 KiB), sorted by rank and summed by thread
//                  0 in sorted order; a longer list (or a lower
//                  PboxLongArgs::cap: SPX_PBOX_LONG_CAP) is walked by rounds of
//                  argmin over global memory, with the same entries, order and
//                  sums.  The leaving entry goes to rparts[0], "none" to the
//                  other update_grid slots: the step kernels run unchanged.
//                  Thread 0 keeps the counters.
constexpr int PBOX_LONG_BLOCK = 1024;
constexpr int PBOX_LONG_CAP = 2048;  // soft breakpoints kept in LDS

struct alignas(16) PboxLongRec {  // counted by the walk, whether the pass then flips or pivots
    int64_t passed;    // rows the walk passed since create / spx_reset
    int64_t passes;    // passes that passed at least one
    int64_t max_pass;  // the most in one pass
    int64_t pad;
};

struct PboxLongArgs {
    PboxLongRec* lrec;
    int32_t cap;  // list capacity, 1 .. PBOX_LONG_CAP
    int32_t pad;
};

// F: the free-column arrays of a context that runs the *_f kernels, else nullptr
hipError_t launch_pbox_long1(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxFreeArgs* F,
                             const PboxLongArgs& G, hipStream_t s);

// Exact weights of a warm basis (spx_pbox_wexact.hip): gamma_j =
// 1 + ||B^-1 A_j||^2 for every column on nb_list, from W.S = the true B^-1 of the
// current basis (m x L row-major, nothing pending: the host materialises it
// first; no kernel here applies an eta).  Three launches, ordered by kernel
// boundaries only:
//   k_pbox_wexact        V = S A_N tile by tile with v_mfma_f64_16x16x4_f64, kept
//                  as column norms only.  Workgroup (x, y) owns rows [128 x, 128 x
//                  + 128) of S and list slots [128 y, 128 y + 128); its four waves
//                  own 64 x 64 quadrants (4 x 4 accumulator tiles in registers).
//                  The K loop runs over 16-wide chunks of S rows and A columns
//                  (both contiguous along k), staged through two LDS buffers with
//                  the next chunk's global loads in flight.  Rows >= m, k >= m
//                  and slots past the list read as zeros (nothing outside S, A or
//                  the list is addressed); with Params::slack_unit a listed slack
//                  column is not streamed (k_pbox_wexact_slack has its norm).
//                  Epilogue: per column the squares of the wave's 64 rows in a
//                  fixed order (tile, register, then the four row groups of the
//                  accumulator layout), the two row halves added through LDS;
//                  one partial per (row block, slot), plain stores.
//   k_pbox_wexact_slack  slack_unit only: column k of S squared and summed per row
//                  block, rows ascending, one lane per column; one partial per
//                  (row block, k).
//   k_pbox_wexact_sum    gamma_j = 1 + the row blocks' partials in ascending
//                  row-block order (a unit slack column from the slack partials).
// The geometry is a function of m and n alone: no tuning option reaches it, so
// the weights are the same bits from run to run and across those options.
constexpr int PBOX_WX_BLOCK = 256;  // threads per workgroup of the three kernels
constexpr int PBOX_WX_TILE = 128;   // rows of S and list slots per k_pbox_wexact workgroup
constexpr int PBOX_WX_KC = 16;      // doubles of k per staged chunk
constexpr int PBOX_WX_LD = PBOX_WX_KC + 2;  // LDS row pitch (doubles): conflict-free fragment reads

struct PboxWexactCfg {
    int row_blocks = 0;  // blocks of PBOX_WX_TILE rows of S: ceil(m / 128)
    int col_tiles = 0;   // tiles of PBOX_WX_TILE list slots: ceil((n - m) / 128)
    int slack_grid = 0;  // k_pbox_wexact_slack: blocks of PBOX_WX_BLOCK columns of S
    int sum_grid = 0;    // k_pbox_wexact_sum: blocks of PBOX_WX_BLOCK list slots
    int64_t cap = 0;     // list slots: n - m (the non-basic count never changes)
    size_t parts = 0;    // doubles of the product's partials: row_blocks x cap
    size_t sparts = 0;   // doubles of the slack partials: row_blocks x L
};

// first and one-past-last list slot of column tile t for a list of cnt entries
struct PboxWexactSlice {
    int64_t lo, hi;
};

inline PboxWexactCfg pbox_wexact_geometry(int64_t m, int64_t n, int64_t L) {
    PboxWexactCfg c;
    c.cap = n - m;
    c.row_blocks = (int)((m + PBOX_WX_TILE - 1) / PBOX_WX_TILE);
    c.col_tiles = (int)((c.cap + PBOX_WX_TILE - 1) / PBOX_WX_TILE);
    c.slack_grid = (int)((m + PBOX_WX_BLOCK - 1) / PBOX_WX_BLOCK);
    c.sum_grid = (int)((c.cap + PBOX_WX_BLOCK - 1) / PBOX_WX_BLOCK);
    c.parts = (size_t)c.row_blocks * (size_t)c.cap;
    c.sparts = (size_t)c.row_blocks * (size_t)L;
    return c;
}

inline PboxWexactSlice pbox_wexact_slice(int64_t t, int64_t cnt) {
    const int64_t lo = t * PBOX_WX_TILE;
    const int64_t hi = lo + PBOX_WX_TILE < cnt ? lo + PBOX_WX_TILE : cnt;
    return PboxWexactSlice{lo < cnt ? lo : cnt, hi};
}

struct PboxWexactArgs {
    const double* S;  // m x L: the true B^-1
    double* parts;    // row_blocks x cap
    double* sparts;   // row_blocks x L
    double* gamma;    // n (PboxSeArgs::gamma)
    int64_t cap;
    int32_t row_blocks;
    int32_t pad;
};

hipError_t pbox_wexact_prepare();  // once per process and device: the product kernel's LDS size
hipError_t launch_pbox_wexact(const Params& P, const PboxWexactArgs& W, const PboxWexactCfg& c, hipStream_t s);

}  // namespace spx
