/*
 * simplex.h — C-ABI of libsimplex, the MI355X (gfx950) dense revised-simplex
 * hot loop.  Plain pointers and sizes only; no HIP, torch or C++ types.
 *
 * What it replaces in the reference (Girjoaba/simplex_method_gpu):
 *   spx_create + spx_solve + spx_destroy
 *        <- std::pair<real,SolveStatus> solve(real* A, real* b, real* c,
 *              real* x_b, int* b_ixs, int m, int n, TimeStruct&)
 *              src/v4_cub_reduction.cu:219-380 (host buffers in, x_b/b_ixs out)
 *   spx_price   <- pricing Sgemm + entering ArgMin + optimality test
 *              src/v4_cub_reduction.cu:288-302
 *   spx_pivot   <- FTRAN Sgemv, compute_theta, leaving ArgMin, E_q, Sger,
 *              basis bookkeeping, x_b and y updates
 *              src/v4_cub_reduction.cu:306-357 (kernels :195-215)
 *   status codes <- enum class SolveStatus, src/v4_cub_reduction.cu:49-54
 * The `./solver <file>` CLI built on top of this header replaces main()
 * (src/v4_cub_reduction.cu:384-473).
 *
 * Conventions
 *   - A is m x n COLUMN-major (column j at A + j*m), as the reference's R2C
 *     (src/v4_cub_reduction.cu:59-60); the last m columns must be the slack
 *     identity and, for the primal loop, b >= 0 (the reference's unchecked
 *     assumption, v4:272-277); b of any sign with SPX_ALGO_DUAL.
 *   - Everything is fp64.  Indices are 0-based int64.
 *   - Every function returns SPX_OK (0) or a negative SPX_ERR_* code; nothing
 *     exits or throws across the ABI.  spx_last_error() gives a message.
 *   - The caller owns host buffers; the context owns device memory.  One
 *     context per host thread; a context is not re-entrant.
 *   - Multi-GPU: one process per GPU.  Pricing columns are sharded over
 *     opts.nranks ranks (structural and slack columns each split in
 *     contiguous blocks); B^-1, x_b, y are replicated.  After spx_create,
 *     every rank calls spx_attach_comm with the id rank 0 obtained from
 *     spx_comm_unique_id (exchange it out of band, e.g. torch.distributed).
 */
#ifndef SIMPLEX_MI355X_H
#define SIMPLEX_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPX_ABI_VERSION 8

/* SolveStatus of the reference (v4_cub_reduction.cu:49-54), same numbering. */
#define SPX_STATUS_MAX_ITER       0
#define SPX_STATUS_OPTIMUM_FOUND  1
#define SPX_STATUS_UNBOUNDED      2
#define SPX_STATUS_THETA_OVERFLOW 3 /* the reference's status, unreachable there since
                                       v2; here: a numerical breakdown of the bounded
                                       primal loop's phase 1 (no blocking row and no
                                       bound on the entering column, which exact
                                       arithmetic excludes)                          */
#define SPX_STATUS_INFEASIBLE     4 /* dual loop: a basic variable is negative and its
                                       row has no dual ratio-test candidate; bounded
                                       primal loop, phase 1: no column lowers the sum
                                       of bound violations.  Either way no 0 <= x <= u
                                       satisfies the constraints                     */

#define SPX_OK             0
#define SPX_ERR_ARG       -1  /* bad argument (m > n, m <= 0, NULL, ...)     */
#define SPX_ERR_HIP       -2  /* a HIP runtime call failed                     */
#define SPX_ERR_OOM       -3  /* device allocation failed                      */
#define SPX_ERR_RCCL      -4  /* an RCCL call failed                           */
#define SPX_ERR_STATE     -5  /* call not valid in the context's state         */
#define SPX_ERR_NO_DEVICE -6  /* no HIP device visible                         */
#define SPX_ERR_SINGULAR  -7  /* spx_reinvert / spx_set_basis: the basis matrix
                                 is singular (no pivot above tolerance)        */

typedef struct spx_ctx spx_ctx;

typedef struct spx_opts {
    double  eps;          /* optimality tolerance on reduced costs: optimum when
                             min_j e_j >= -eps (reference EPS, v4:18: 1e-4 f32);
                             default 1e-7 (fp64)                */
    int32_t device;       /* HIP device ordinal; -1 = keep the current device  */
    int32_t rank;         /* pricing shard of this process (default 0)         */
    int32_t nranks;       /* number of shards (default 1)                      */
    int32_t graph_batch;  /* iterations per captured hipGraph; 0 = auto (16,
                             RCCL calls captured too; a capture RCCL refuses
                             falls back to eager), -1 = eager launches       */
    int32_t price_block;  /* tuning: threads per pricing workgroup, 0 = auto   */
    int32_t update_rows;  /* tuning: B^-1 rows per wave in the update, 0 = auto */
    int32_t price_grid;   /* tuning: pricing workgroups, 0 = auto              */
    int32_t flags;        /* SPX_FLAG_* bits                                   */
    int32_t update_block; /* tuning: threads per update workgroup, 0 = auto    */
    int32_t window;       /* B^-1 representation: 0 = auto
                             (window 64 at m >= 2048, else explicit),
                             -1 = explicit B^-1 rewritten by a rank-1 update
                             every pivot (v4:331-333), 8/16/32/64 = eta window:
                             B^-1 = B_w + U R kept for up to window-1 pivots,
                             then folded by one rank-(window-1) update.  The
                             window is single-shard / replicated-B^-1 only.   */
    int32_t ratio_test;   /* leaving-row rule, SPX_RATIO_* (default REFERENCE)  */
    int32_t refactor_every; /* spx_solve / spx_iterate: rebuild B^-1 from the
                             basis columns (spx_reinvert) every K pivots;
                             0 = never (the reference never does)            */
    double  piv_tol;      /* SPX_RATIO_GUARDED / HARRIS: rows need alpha_i >
                             piv_tol (default 1e-9); SPX_ALGO_DUAL: ratio-test
                             candidates need rho.A_j < -piv_tol               */
    double  feas_tol;     /* SPX_RATIO_HARRIS: primal feasibility tolerance
                             delta of the first pass (default 1e-9);
                             SPX_ALGO_DUAL: rows leave while x_b < -feas_tol  */
    int32_t pricing;      /* entering-column rule, SPX_PRICING_* (default DANTZIG) */
    int32_t loop_block;   /* tuning: threads per workgroup of the persistent loop
                             kernel (512 / 1024), 0 = auto                     */
    int32_t trace_cap;    /* record the first trace_cap pivots' (entering column
                             p, leaving row q) on the device, written by the
                             kernel that commits each pivot (spx_get_trace);
                             0 = off.  The reference prints nothing of the
                             kind; the parity tests compare it with the
                             oracle's pivot sequence.                        */
    int32_t algorithm;    /* SPX_ALGO_PRIMAL (default), _DUAL or _PRIMAL_BOX; the field
                             was `reserved` (0) before, the layout is unchanged */
} spx_opts;

/* Simplex algorithm of spx_iterate / spx_solve.
 * PRIMAL: the loop above; needs a primal feasible basis (b >= 0 at the slack
 *         basis).
 * DUAL:   the dual simplex method, for a basis that is dual
 *         feasible (every non-basic e_j >= -eps; checked before the first dual
 *         pass: SPX_ERR_STATE "basis is not dual feasible") but may have
 *         negative x_b: a covering LP max -c.x, -G x + s = -h with c >= 0 at
 *         its slack basis, or an optimal basis after spx_set_rhs.  Leaving row
 *         q = argmin x_b[i] over x_b[i] < -feas_tol (none: OPTIMUM_FOUND);
 *         with rho = row q of B^-1, a_j = rho.A_j and d_j = y.A_j - c_j the
 *         entering column is the argmin of max(d_j, 0) / -a_j over non-basic
 *         a_j < -piv_tol (none: SPX_STATUS_INFEASIBLE); first index on ties.
 *         One rank, explicit B^-1 (window 0 resolves to -1), opts.pricing (the
 *         primal entering rule) Dantzig; spx_create rejects nranks > 1, an eta
 *         window, the tableau, the Harris ratio test and Devex / steepest-edge
 *         opts.pricing with SPX_ERR_ARG.  spx_price / spx_pivot and
 *         spx_group_iterate return SPX_ERR_STATE under it.  refactor_every works
 *         as in the primal loop.  The leaving-row rule is SPX_DUAL_PRICING_*.
 *         Boxed variables 0 <= x_j <= u_j (spx_set_bounds; all n columns, a
 *         bounded slack is a ranged row) exist under DUAL only.  A non-basic
 *         column sits at 0 (sigma_j = +1) or at u_j (sigma_j = -1) and is dual
 *         feasible with e_j >= -eps at lower, e_j <= eps at upper; before the
 *         first pass every non-basic column is put on its feasible side (e_j <
 *         -eps with no upper bound: SPX_ERR_STATE "basis is not dual feasible",
 *         naming the column).  x_b = B^-1 (b - sum_{j at upper} u_j A_j) and z =
 *         c_B.x_b + sum_{j at upper} c_j u_j.  Row i (basic column k) violates
 *         by delta_i = x_b[i] below -feas_tol, x_b[i] - u_k above u_k +
 *         feas_tol; Dantzig takes argmin -|delta_i|, steepest edge argmin
 *         -delta_i^2 / w_i; s = +1 when the row leaves to its lower bound, -1 to
 *         its upper.  Ratio test over non-basic s sigma_j a_j < -piv_tol with key
 *         max(sigma_j d_j, 0) / -(s sigma_j a_j); theta = delta_q / alpha_q and
 *         the entering column starts from the bound it sat at.  Without a
 *         finite bound the loop and its kernels are the unbounded ones.  Finite
 *         bounds with SPX_ALGO_PRIMAL are SPX_ERR_STATE; the bound-flipping ratio
 *         test is SPX_DUAL_RATIO_LONG_STEP (below).  Finite lower bounds of any
 *         sign run shifted (spx_set_bounds_lu below); no free and no upper-only
 *         columns.
 * PRIMAL_BOX: the primal simplex method with bounded variables 0 <= x_j <= u_j
 *         (DESIGN.md §7e), for a basis that is primal feasible within its
 *         bounds; it shares the bounds, placements and effective right-hand
 *         side with DUAL (spx_set_bounds works under both), so
 *         spx_set_algorithm hands a basis from one to the other.  Before the
 *         first pass after spx_create, spx_reset, spx_set_basis,
 *         spx_set_algorithm, spx_set_bounds, spx_set_rhs or spx_set_cost the
 *         placements are kept (a column at an upper bound that is now +inf goes
 *         to lower), x_b is recomputed from them and -feas_tol <= x_b[i] <= u_k +
 *         feas_tol is checked (k the row's basic column): a violation is
 *         SPX_ERR_STATE "basis is not primal feasible", naming the row and the
 *         column; nothing changes and SPX_ALGO_DUAL can repair it.  One pass:
 *         d_j = y.A_j - c_j over the non-basic columns, candidates sigma_j d_j <
 *         -eps, p = argmin sigma_j d_j (none: OPTIMUM_FOUND); alpha = B^-1 A_p,
 *         ahat = sigma_p alpha; row i with ahat_i > piv_tol leaves to its lower
 *         bound at t_i = max(x_b[i], 0) / ahat_i, row i with ahat_i < -piv_tol and
 *         a finite u_k to its upper bound at t_i = max(u_k - x_b[i], 0) / -ahat_i;
 *         q = argmin t_i; first index on every tie.  u_p finite and (no row, or
 *         u_p <= t_q): a flip, x_b -= u_p ahat and p changes sides; no basis
 *         change, not a pivot.  No row and u_p = +inf: SPX_STATUS_UNBOUNDED.  Else
 *         theta = t_q: x_b -= theta ahat, x_b[q] = (u_p at upper, else 0) +
 *         sigma_p theta, y -= (d_p / alpha_q) rho (rho = row q of B^-1 before the
 *         pivot), and the leaving column becomes non-basic at exactly the bound
 *         it left to.  The pivot count, the trace, refactor_every and
 *         spx_iterate(k) count pivots only.  With every bound +inf this is the
 *         primal loop's Dantzig rule with SPX_RATIO_GUARDED.  Scope and refusals
 *         are DUAL's (spx_create: SPX_ERR_ARG naming the combination; spx_price /
 *         spx_pivot / spx_group_iterate: SPX_ERR_STATE).  The entering rule is
 *         SPX_PRIMAL_PRICING_* (below: Dantzig, or exact steepest edge); no
 *         Devex.  Finite lower bounds of any sign run shifted and free columns
 *         run under Dantzig pricing (spx_set_bounds_lu below), or
 *         under steepest edge where spx_set_primal_free_pricing says so
 *         (DESIGN.md §7m); no upper-only columns.  SPX_ALGO_PRIMAL itself still refuses finite
 *         bounds.
 *         Phase 1 (opt-in: SPX_FLAG_PRIMAL_PHASE1, spx_set_primal_phase1;
 *         DESIGN.md §7f).  With it the entry check refuses nothing: row i is
 *         *below* when x_b[i] < -feas_tol, *above* when x_b[i] > u_k + feas_tol,
 *         feasible otherwise; ninf counts the below and above rows, and a pass
 *         that starts with ninf > 0 is a phase-1 pass: w_i = +1 (below), -1
 *         (above), 0 (feasible), y1 = w.B^-1, d_j = y1.A_j with no cost term,
 *         the same entering rule (none: SPX_STATUS_INFEASIBLE).  Ratio test:
 *         feasible rows block as above; a below row blocks only when ahat_i <
 *         -piv_tol, at t_i = x_b[i] / ahat_i, and leaves to its lower bound; an
 *         above row only when ahat_i > piv_tol, at t_i = (x_b[i] - u_k) / ahat_i,
 *         and leaves to its upper bound; an infeasible row moving away from its
 *         bound does not block.  Flips and pivots are as above, except that y is
 *         not updated; no row and u_p = +inf is SPX_STATUS_THETA_OVERFLOW (a
 *         numerical breakdown).  The rows are classified again after every
 *         phase-1 pass and after every reinversion; no feasible row becomes
 *         infeasible, so ninf never grows.  The first pass that starts with ninf
 *         == 0 recomputes y = c_B.B^-1 once and is an ordinary pass; so does every
 *         readback of y and every spx_set_algorithm in between.  Pivots, the
 *         trace, refactor_every, spx_iterate(k) and spx_get_primal_flips count
 *         both phases.  With phase 1 on and a feasible entry the loop launches
 *         exactly the passes it launches without.  Phase 1 prices with
 *         Dantzig's rule, or with the steepest-edge weights where the loop's
 *         rule is steepest edge and spx_set_primal_phase_one_pricing says so
 *         (below).  The phase-1 ratio test stops at the first row that reaches
 *         a bound, or walks past such rows while the sum of violations still
 *         falls (SPX_PRIMAL_RATIO_LONG_STEP, spx_set_primal_phase_one_ratio,
 *         below).  Still out: phase 1 under SPX_ALGO_PRIMAL, a rule that
 *         differs between the phases. */
#define SPX_ALGO_PRIMAL 0
#define SPX_ALGO_DUAL   1
#define SPX_ALGO_PRIMAL_BOX 2

/* Leaving-row rules of the dual loop (SPX_FLAG_DUAL_STEEPEST at spx_create,
 * spx_set_dual_pricing later; opts.pricing is the primal entering rule and
 * stays Dantzig under SPX_ALGO_DUAL).
 * DANTZIG:  q = argmin x_b[i] over x_b[i] < -feas_tol (above).
 * STEEPEST: dual steepest edge with exact weights w_i = ||row i of B^-1||^2:
 *           q = argmin of -x_b[i]^2 / w_i over x_b[i] < -feas_tol (first index
 *           on ties; none: OPTIMUM_FOUND); the ratio test is unchanged.  The
 *           pass that pivots on row q with alpha = B^-1 A_p reads every row of
 *           the explicit B^-1 anyway and takes w_i = row_i.row_i and tau_i =
 *           row_i.rho (rho = row q) from the same read; with r_i = alpha_i /
 *           alpha_q and w_q = rho.rho the weights after the pivot are
 *           w'_i = max(w_i - 2 r_i tau_i + r_i^2 w_q, 1e-300) for i != q and
 *           w'_q = w_q / alpha_q^2.  w_i is recomputed every pass, so nothing
 *           drifts and there is no reset rule.  Where no pass has kept them
 *           (spx_create, spx_reset, spx_set_basis, spx_reinvert, refactor_every,
 *           spx_set_rhs, spx_set_algorithm, a change of rule) the weights are
 *           recomputed from B^-1 before the next pass. */
#define SPX_DUAL_PRICING_DANTZIG  0
#define SPX_DUAL_PRICING_STEEPEST 1

/* Entering rules of the bounded primal loop (SPX_FLAG_PRIMAL_STEEPEST at
 * spx_create, spx_set_primal_pricing later; opts.pricing is the windowed primal
 * loop's field and stays Dantzig under SPX_ALGO_PRIMAL_BOX and SPX_ALGO_DUAL).
 * DANTZIG:  p = argmin sigma_j d_j over the candidates (above).
 * STEEPEST: exact primal steepest edge with the weights
 *           gamma_j = 1 + ||B^-1 A_j||^2 of the non-basic columns; they do not
 *           depend on the bound a column sits at, and a flip pass changes none.
 *           The candidates are unchanged (sigma_j d_j < -eps; none:
 *           OPTIMUM_FOUND) and p = argmin of -d_j^2 / gamma_j over them, first
 *           column on ties.  The ratio test, the flips, the unbounded exit, the
 *           commit and the y update are DANTZIG's.  After a pivot on row q with
 *           alpha = B^-1 A_p, rho = row q of B^-1 and tau = alpha^T B^-1 (both of
 *           the B^-1 before the pivot, so tau.A_j = A_j.B^-T alpha) and gamma_p =
 *           1 + ||alpha||^2 recomputed exactly, every column j that was
 *           non-basic before the pivot and is not p gets, with g = (rho.A_j) /
 *           alpha_q, gamma_j = max(gamma_j - 2 g (tau.A_j) + g^2 gamma_p, 1 +
 *           g^2), and the leaving column gamma = max(gamma_p / alpha_q^2, 1)
 *           (Goldfarb and Reid's update; no reset rule).  Where no pass has
 *           kept them (spx_create, spx_reset, spx_set_basis, spx_set_algorithm
 *           into the loop, a change of rule) the weights restart: at the
 *           slack basis (spx_create, spx_reset) always at 1 + ||A_j||^2, which is
 *           exact there; for a warm basis as SPX_PRIMAL_WEIGHTS_* says (below:
 *           1 + ||A_j||^2 again, a reference framework and not the exact norm, or
 *           the exact 1 + ||B^-1 A_j||^2 formed on the device).  Dantzig passes
 *           in between keep no weights either.  spx_reinvert, refactor_every,
 *           spx_set_cost, spx_set_rhs and spx_set_bounds keep the basis and the
 *           weights.  Not together with phase 1 (SPX_FLAG_PRIMAL_PHASE1 /
 *           spx_set_primal_phase1): spx_create refuses the two flags with
 *           SPX_ERR_ARG, and whichever setter arrives second returns
 *           SPX_ERR_STATE -- unless phase 1's own rule was set to STEEPEST first
 *           (SPX_FLAG_PRIMAL_PHASE1_STEEPEST / spx_set_primal_phase_one_pricing,
 *           DESIGN.md §7l).  Then a pass that starts with ninf > 0 stays the
 *           phase-1 pass described above (w, y1, d_j without a cost term, the
 *           candidates, the phase-aware ratio test, flips, INFEASIBLE, no y
 *           update) except that p = argmin of -d_j^2 / gamma_j over the
 *           candidates, first column on ties; every pivot of either phase
 *           applies the update above, a flip changes no weight, and the switch
 *           to phase 2 keeps the weights (no restart).  The weights start as
 *           without phase 1; neither start depends on feasibility.  Free columns
 *           stay refused under steepest edge. */
#define SPX_PRIMAL_PRICING_DANTZIG  0
#define SPX_PRIMAL_PRICING_STEEPEST 1

/* How the steepest-edge weights of the bounded primal loop restart for a warm
 * basis, i.e. wherever no pass has kept them and the basis is not the slack
 * basis (SPX_FLAG_PRIMAL_EXACT_WEIGHTS at spx_create, spx_set_primal_weight_init
 * later).  Inert under SPX_PRIMAL_PRICING_DANTZIG and under the
 * other algorithms.
 * REFERENCE: gamma_j = 1 + ||A_j||^2, a reference framework (the default).
 * EXACT:     gamma_j = 1 + ||B^-1 A_j||^2 of every non-basic column, from the
 *            B^-1 spx_get_state would return: one fp64 matrix product on the
 *            device whose result is kept as column norms only.  Its tiling and
 *            summation order depend on m and n alone, so the weights are the
 *            same bits from run to run and under every tuning option.  From the
 *            slack basis both modes start from the same weights and walk the
 *            same passes. */
#define SPX_PRIMAL_WEIGHTS_REFERENCE 0
#define SPX_PRIMAL_WEIGHTS_EXACT     1

/* Ratio tests of the bounded primal loop's phase-1 passes
 * (spx_set_primal_phase_one_ratio).  Phase-2 passes are the same
 * under both.  Notation as above: ahat = sigma_p alpha, only rows with |ahat_i| >
 * piv_tol take part, entries are ordered by (t, 2 row + side), side 1 = the row
 * leaves to its upper bound.
 * TEXTBOOK:  the first row that reaches a bound leaves (above; the default).
 * LONG_STEP: the sum of violations is piecewise linear along the entering
 *            direction: its slope is sigma_p d_p < 0 at t = 0 (-|d_p| for a free
 *            entering column) and gains |ahat_i| where an infeasible row i
 *            reaches the bound it violates.  Such a point is a soft breakpoint:
 *            a below row with ahat_i < 0 at x_b[i] / ahat_i (side 0), an above
 *            row with ahat_i > 0 at (x_b[i] - u_k) / ahat_i (side 1): TEXTBOOK's
 *            entries.  Hard breakpoints must not be passed: every entry of a
 *            feasible row (TEXTBOOK's, the free rule included), and the far
 *            bound of a row that has a soft breakpoint (a below row with a
 *            finite u_k at (x_b[i] - u_k) / ahat_i, side 1; an above row at
 *            x_b[i] / ahat_i, side 0).  With h the smallest hard breakpoint,
 *            the soft breakpoints before h are walked in order, slope +=
 *            |ahat_i| at each: the first at which slope >= -opts.eps leaves, at
 *            its t and side; one with a smaller slope is passed (its row comes
 *            out feasible).  If the walk ends without a leaving row, h leaves,
 *            or with no hard breakpoint the last soft one; with no breakpoint
 *            at all the pass is TEXTBOOK's (a flip, or
 *            SPX_STATUS_THETA_OVERFLOW).  The flip test u_p <= t_q, the commit,
 *            the classification and the counters are TEXTBOOK's with this t_q.
 *            No feasible row leaves its box, so ninf still never grows; a walk
 *            that passes nothing selects TEXTBOOK's row. */
#define SPX_PRIMAL_RATIO_TEXTBOOK  0
#define SPX_PRIMAL_RATIO_LONG_STEP 1

/* Ratio tests of the dual loop's boxed passes (SPX_FLAG_DUAL_LONG_STEP at
 * spx_create, spx_set_dual_ratio later).
 * TEXTBOOK:  the entering column is the first candidate in (key, column) order
 *            (above).
 * LONG_STEP: the bound-flipping (long-step) ratio test.  The candidates are
 *            walked in that order with slope = |delta_q|: a candidate with u_j =
 *            +inf enters; otherwise slope' = slope - u_j (-ahat_j), ahat_j = s
 *            sigma_j a_j; slope' <= 0: it enters (at exactly 0 it enters at its
 *            bound and row q is feasible), else it is flipped to its other
 *            bound, slope = slope' and the walk goes on.  No candidate, or all
 *            flipped and none enters: SPX_STATUS_INFEASIBLE with no flip applied.
 *            With dx_j = +u_j for a flipped column at lower, -u_j at upper, and v
 *            = sum dx_j A_j: x_b -= B^-1 v, the effective right-hand side -= v,
 *            the flipped columns change side, delta_q is taken again from the
 *            new x_b[q] (same s) and the pivot on the entering column is the
 *            textbook one with the walk's d_p.  Flips are not pivots: the pivot
 *            count, the trace and refactor_every count pivots only, and the
 *            steepest-edge weights do not depend on placements.  A pass that
 *            flips nothing is the textbook pass bit for bit; a context with no
 *            finite bound launches the unbounded kernels under either rule. */
#define SPX_DUAL_RATIO_TEXTBOOK  0
#define SPX_DUAL_RATIO_LONG_STEP 1

/* Entering-column rules (README.md:16-17 "steepest edge").
 * DANTZIG: most negative e_j (v4:288-302).
 * DEVEX:   Devex reference weights w_j (1 at the start): after a pivot with
 *          pivot element alpha_q, entering weight w_p and pivot row
 *          alpha_rj = r.A_j (r = row q of B^-1 before the pivot),
 *          w_j = max(w_j, (alpha_rj/alpha_q)^2 w_p) for non-basic j and
 *          w_leave = max(w_p/alpha_q^2, 1); p = argmin of -e_j^2/w_j over
 *          e_j < -eps (first index on ties).  The pivot row comes free from
 *          the eta-window pricing pass (it computes r.A_j for every column),
 *          so DEVEX needs the window (opts.window 0 selects 64).  On a column-
 *          shard group the winner's record carries its reduced cost and weight
 *          (not with SPX_FLAG_SPLIT_TAIL / SPX_RATIO_HARRIS).  spx_price's min_e
 *          is then the entering column's reduced cost. */
#define SPX_PRICING_DANTZIG 0
#define SPX_PRICING_DEVEX   1
/* STEEPEST: steepest edge with a recurrence (README.md:16-17): exact weights
 *          gamma_j = 1 + ||B^-1 A_j||^2, 1 + ||A_j||^2 at the slack basis,
 *          kept by Goldfarb & Reid's update after a pivot with alpha = B^-1 A_p,
 *          pivot element alpha_q, pivot row alpha_rj, g = alpha_rj / alpha_q,
 *          gamma_p = 1 + ||alpha||^2 and d_j = A_j . B^-T alpha (B^-1 before
 *          the pivot): gamma_j = max(gamma_j - 2 g d_j + g^2 gamma_p, 1 + g^2),
 *          gamma_leave = max(gamma_p / alpha_q^2, 1); p = argmin of
 *          -e_j^2/gamma_j over e_j < -eps.  d_j rides on the pricing pass's
 *          A stream as a third dot (B_w^T alpha in LDS beside y_w and the base
 *          row, plus the window terms), so it needs the window, runs two-kernel
 *          passes, and not with the tableau; on a column-shard group as DEVEX
 *          (every rank forms B_w^T alpha from the replicated B^-1).  spx_set_basis
 *          restarts the weights at 1 + ||A_j||^2. */
#define SPX_PRICING_STEEPEST 2

/* Leaving-row rules.
 * REFERENCE: theta_i = x_b_i / alpha_i over alpha_i > 0, first index on ties
 *            (compute_theta + ArgMin, v4:199-208,324); no guard, no filter.
 * GUARDED:   only alpha_i > piv_tol (the pivot-size guard of the thesis code,
 *            archive/thesis/cpu/liblp.c:39, gpu/culiblp.cu:401) and
 *            theta_i = max(x_b_i, 0) / alpha_i (its x_b >= -EPS filter,
 *            liblp.c:18-20; README.md:29-30 "x_b_t < 0", "division by a small
 *            number").
 * HARRIS:    two passes: theta_max = min (max(x_b_i,0) + feas_tol) / alpha_i
 *            over alpha_i > piv_tol, then the largest alpha_i among rows with
 *            max(x_b_i,0) / alpha_i <= theta_max (first index on ties).
 *            Single rank or replicated B^-1 only; runs the pivot tail as its
 *            own launch. */
#define SPX_RATIO_REFERENCE 0
#define SPX_RATIO_GUARDED   1
#define SPX_RATIO_HARRIS    2

#define SPX_FLAG_TIMING 1 /* record per-kernel hipEvents (spx_kernel_times)  */
#define SPX_FLAG_STAMPS 2 /* in-kernel phase stamps (spx_phase_times); diagnostic */
#define SPX_FLAG_GLOBAL_Y 4 /* pricing reads y from global memory instead of LDS
                               (automatic when L*8 bytes do not fit in LDS); the
                               dual loop's ratio test then reads rho and y, and its
                               steepest-edge FTRAN + update kernel its three
                               operands, from global memory                   */
#define SPX_FLAG_SPLIT_TAIL 16 /* tuning: run the pivot tail as its own launch
                                  instead of the update kernel's last workgroup */
#define SPX_FLAG_NO_PERSIST 32 /* tuning: never use the persistent loop kernel */
#define SPX_FLAG_PERSIST 64    /* tuning: use the persistent cooperative loop kernel
                                  (k_loop: one launch per window, two grid
                                  barriers per pass instead of two kernels) where
                                  it applies (window > 0, one rank, no Harris, no
                                  stamps).  Default: only when y_w and the base
                                  row do not both fit in LDS (m > ~9400, e.g. C5:
                                  +7 %); at C3 the two-kernel pass is faster.   */
#define SPX_FLAG_COMM1 128 /* test: with nranks == 1, run the MINLOC exchange through
                              RCCL anyway (spx_attach_comm with a one-rank id), so
                              the communicator path, graph-captured RCCL calls
                              included, can be checked on one GPU            */
#define SPX_FLAG_TABLEAU 256 /* window tableau: with the eta window,
                                also keep T_w = B_w A and dw = y_w A - c in HBM and
                                fold them with B_w (fp64 MFMA), so a pass reads no
                                A column and no B_w row: pricing reads T_w[q, j],
                                dw[j] and the window row of each non-basic column,
                                FTRAN the column T_w[:, p].  Needs the window (0 =
                                auto selects 64) and one rank; twice A's memory. */
#define SPX_FLAG_COUNTED_TAIL 512 /* tuning: the update kernel's workgroups hand
                                     their ratio-test partials (and the pricing
                                     kernel's, where it reduces them itself)
                                     to the tail by drained stores + a
                                     last-arrival count instead of tagged
                                     words polled by the last workgroup (the
                                     default)                                 */
#define SPX_FLAG_PRICE_TAIL 1024 /* tuning: the pricing kernel's last workgroup
                                    merges the entering candidates (default on
                                    one rank with the window: every update
                                    workgroup merges k_price's partials)     */
#define SPX_FLAG_ROW_SHARD 8 /* nranks > 1: B^-1 row-sharded over the ranks
                                (ceil(m/nranks) rows each) instead of
                                replicated; one extra all-gather per pass
                                carries the pivot row.  Readback functions
                                then gather x_b over the communicator
                                (collective: every rank must call them).     */

#define SPX_FLAG_DUAL_STEEPEST 2048 /* the dual loop starts with the leaving-row rule
                                       SPX_DUAL_PRICING_STEEPEST (default DANTZIG);
                                       accepted and inert while the context runs the
                                       primal loop                                */

#define SPX_FLAG_DUAL_LONG_STEP 4096 /* the dual loop starts with the ratio test
                                       SPX_DUAL_RATIO_LONG_STEP (default TEXTBOOK);
                                       accepted and inert while the context runs the
                                       primal loop or has no finite bound          */

#define SPX_FLAG_PRIMAL_PHASE1 8192 /* the bounded primal loop (SPX_ALGO_PRIMAL_BOX)
                                       starts with its phase 1 enabled (default off:
                                       a basis out of its bounds is refused); accepted
                                       and inert under the other algorithms         */

#define SPX_FLAG_PRIMAL_STEEPEST 16384 /* the bounded primal loop starts with the entering
                                         rule SPX_PRIMAL_PRICING_STEEPEST (default
                                         DANTZIG); accepted and inert under the other
                                         algorithms; SPX_ERR_ARG together with
                                         SPX_FLAG_PRIMAL_PHASE1 unless
                                         SPX_FLAG_PRIMAL_PHASE1_STEEPEST is set too   */

#define SPX_FLAG_PRIMAL_PHASE1_STEEPEST 65536 /* the bounded primal loop's phase 1 prices with
                                         the steepest-edge weights where the loop's rule
                                         is SPX_PRIMAL_PRICING_STEEPEST
                                         (spx_set_primal_phase_one_pricing; default
                                         DANTZIG, under which SPX_FLAG_PRIMAL_PHASE1 with
                                         SPX_FLAG_PRIMAL_STEEPEST stays refused); with it
                                         the three flags together are accepted; accepted
                                         and inert without the other two and under the
                                         other algorithms                             */

#define SPX_FLAG_PRIMAL_FREE_STEEPEST 131072 /* the bounded primal loop prices free columns
                                         (spx_set_bounds_lu) with the steepest-edge
                                         weights where the loop's rule is
                                         SPX_PRIMAL_PRICING_STEEPEST
                                         (spx_set_primal_free_pricing; default DANTZIG,
                                         under which free columns with steepest edge
                                         stay refused); accepted and inert on a context
                                         without free columns, under
                                         SPX_PRIMAL_PRICING_DANTZIG and under the other
                                         algorithms                                   */

#define SPX_FLAG_PRIMAL_EXACT_WEIGHTS 32768 /* the bounded primal loop restarts its
                                         steepest-edge weights for a warm basis at
                                         the exact norms (SPX_PRIMAL_WEIGHTS_EXACT;
                                         default REFERENCE); accepted and inert under
                                         SPX_PRIMAL_PRICING_DANTZIG and the other
                                         algorithms                                  */

void spx_default_opts(spx_opts* opts);

/* Allocate device state, upload A (column-major, ld = m), b, c and set the
 * slack basis (B^-1 = I, x_b = b, y = c_B; v4:268-280). */
int spx_create(spx_ctx** out, int64_t m, int64_t n, const double* A_colmajor,
               const double* b, const double* c, const spx_opts* opts);

/* Same, but A, b, c are produced on the device by the seeded generator of
 * SURVEY.md §8(d) (bit-identical to oracle/simplex_oracle.c orc_generate). */
int spx_create_generated(spx_ctx** out, int64_t m, int64_t n, uint64_t seed,
                         const spx_opts* opts);

void spx_destroy(spx_ctx* ctx);

/* RCCL plumbing for opts.nranks > 1 (no-ops returning SPX_OK when nranks == 1). */
#define SPX_COMM_ID_BYTES 128
int spx_comm_unique_id(uint8_t id[SPX_COMM_ID_BYTES]);
int spx_attach_comm(spx_ctx* ctx, const uint8_t id[SPX_COMM_ID_BYTES]);

/* Evidence of what actually joined the exchange (no reference counterpart:
 * the reference is one process on one GPU).  out[0] = ranks the attached RCCL
 * communicator reports (ncclCommCount; -1 when none is attached), out[1] =
 * this rank in it (ncclCommUserRank; -1), out[2] = the HIP device RCCL bound
 * (ncclCommCuDevice; -1), out[3] = the context's HIP device ordinal, out[4] =
 * 1 when loop passes replay captured hipGraphs (the all-gathers inside them),
 * 0 when they run eagerly, out[5] = 1 when a capture with RCCL calls failed
 * and the context fell back to eager passes, out[6] = opts.nranks, out[7] =
 * opts.rank.  bus_id: the context device's PCI bus id (hipDeviceGetPCIBusId,
 * NUL-terminated).  Whether graphs are used is known once the first batch
 * has been captured (the first spx_iterate long enough for one). */
#define SPX_COMM_INFO_FIELDS 8
#define SPX_BUS_ID_BYTES 64
int spx_comm_info(spx_ctx* ctx, int32_t out[SPX_COMM_INFO_FIELDS], char bus_id[SPX_BUS_ID_BYTES]);

/* Peer mailboxes: the pricing MINLOC exchange (the RCCL all-gather of the
 * candidate records after src/v4_cub_reduction.cu:294-302's argmin) as direct
 * stores into every rank's device mailbox over xGMI, one small kernel per pass
 * (k_exchange), instead of ncclAllGather.  Every rank calls spx_mbox_export,
 * gathers all handles in rank order out of band (e.g. torch.distributed
 * all_gather_object) and calls spx_mbox_attach with them; from then on the
 * MINLOC exchange goes through the mailboxes.  The row-sharded B^-1 still
 * needs spx_attach_comm (its ratio-test exchange is RCCL).  Collective in
 * effect: all ranks must attach before any of them iterates.  Handles are
 * hipIpcMemHandle_t bytes; a rank's own handle is not opened (its mailbox is
 * used directly), so one rank (SPX_FLAG_COMM1) runs the same kernel alone.
 * Ranks may share a device (several processes on one GPU). */
#define SPX_MBOX_HANDLE_BYTES 64
int spx_mbox_export(spx_ctx* ctx, uint8_t handle[SPX_MBOX_HANDLE_BYTES]);
int spx_mbox_attach(spx_ctx* ctx, const uint8_t* handles /* nranks x SPX_MBOX_HANDLE_BYTES */);

/* In-process shard group: G contexts created with nranks = G and ranks
 * 0..G-1 (any devices, no communicator) run k lockstep iterations with the
 * MINLOC candidates exchanged by device-to-device copies instead of RCCL
 * (one host thread drives all shards; single-process multi-GPU, and the
 * way the sharded path is validated on one GPU).  status/pivots: rank 0's. */
int spx_group_iterate(spx_ctx** ctxs, int32_t G, int64_t k, int32_t* status,
                      int64_t* pivots);

/* Row-sharded groups (SPX_FLAG_ROW_SHARD, no communicator): flush every
 * member and copy each member's x_b rows to all members, so per-context
 * readback (spx_get_state x_b / spx_objective / spx_solve) is complete.
 * spx_get_state's B^-1 then still holds only the member's own rows. */
int spx_group_sync(spx_ctx** ctxs, int32_t G);

/* Back to the slack basis (keeps A, b, c). */
int spx_reset(spx_ctx* ctx);

/* Rebuild B^-1 from the current basis columns of A on the device (pivot-in
 * reinversion, 64-column MFMA blocks; procedure: oracle/simplex_oracle.h
 * orc_reinvert) and recompute x_b = B^-1 b, y = c_B B^-1 (the v2 formulas,
 * v2_quadratic_B_inv.cu:337-338,396-397).  The basis order is kept.  Also
 * run every opts.refactor_every pivots by spx_iterate / spx_solve.  Replicated
 * B^-1 only (not with SPX_FLAG_ROW_SHARD).  SPX_ERR_SINGULAR when the basis
 * matrix has no pivot above 1e-11 of a column's largest entry.  With
 * nranks > 1 every rank must call it (no communication; the results are
 * bit-identical). */
int spx_reinvert(spx_ctx* ctx);

/* Warm start: make basis[0..m) (distinct column indices, basis order) the
 * current basis, B^-1 by reinversion, status back to running (pivot count
 * kept).  The primal simplex needs x_b = B^-1 b >= 0: read x_b back to check.
 * On SPX_ERR_SINGULAR the context has no valid basis until spx_reset. */
int spx_set_basis(spx_ctx* ctx, const int64_t* basis);

/* Switch the context between the primal and the dual loop (SPX_ALGO_*); the
 * basis, B^-1, x_b, y and the pivot count are kept and the status goes back to
 * running, so the new loop re-tests its own stopping rule.  SPX_ERR_STATE when
 * the context cannot run the dual loop: an eta window or tableau context,
 * nranks > 1, Harris ratio test, Devex / steepest-edge pricing (the message
 * names the combination). */
int spx_set_algorithm(spx_ctx* ctx, int32_t algorithm);

/* Leaving-row rule of the dual loop (SPX_DUAL_PRICING_*), between any two
 * calls; takes effect with the next dual pass.  Valid while the context runs
 * the primal loop too (e.g. before spx_set_algorithm(SPX_ALGO_DUAL) repairs a
 * primal solve after spx_set_rhs).  SPX_ERR_ARG for NULL or an unknown rule. */
int spx_set_dual_pricing(spx_ctx* ctx, int32_t rule);

/* Ratio test of the dual loop's boxed passes (SPX_DUAL_RATIO_*), between any
 * two calls; takes effect with the next dual pass and invalidates nothing (the
 * feasibility check and the steepest-edge weights stay).  Valid while the
 * context runs the primal loop too.  SPX_ERR_ARG for NULL or an unknown rule. */
int spx_set_dual_ratio(spx_ctx* ctx, int32_t rule);

/* Bound flips of the long-step ratio test since spx_create or spx_reset:
 * out[0] columns flipped, out[1] passes that flipped at least one column,
 * out[2] the largest flip count of one pass.  Counted on the device by the
 * kernel that walks the candidates. */
int spx_get_dual_flips(spx_ctx* ctx, int64_t out[3]);

/* Dual steepest-edge weights w[0..m) of the current basis (squared row norms
 * of B^-1, basis order), recomputed first where no pass has kept them.
 * SPX_ERR_STATE when the rule is SPX_DUAL_PRICING_DANTZIG or the context runs
 * the primal loop. */
int spx_get_dual_weights(spx_ctx* ctx, double* w /* m */);

/* New right-hand side b[0..m), any signs: uploaded, then x_b = B^-1 b for the
 * current basis (through spx_reinvert), status back to running, pivot count
 * kept.  The basis stays dual feasible, so after an optimal solve
 * spx_set_algorithm(SPX_ALGO_DUAL) + spx_solve re-optimises from it.  One rank,
 * replicated B^-1 (SPX_ERR_STATE otherwise). */
int spx_set_rhs(spx_ctx* ctx, const double* b);

/* New objective c[0..n): uploaded, then c_B and y = c_B B^-1 for the current
 * basis (through spx_reinvert), status back to running; the pivot count, the
 * basis, the placements and x_b are kept.  The basis stays primal feasible, so
 * after an optimal boxed dual solve spx_set_algorithm(SPX_ALGO_PRIMAL_BOX) +
 * spx_solve re-optimises from it; under SPX_ALGO_DUAL the feasibility check
 * (boxed: the normalisation) runs again before the next pass.  One rank,
 * replicated B^-1 (SPX_ERR_STATE otherwise). */
int spx_set_cost(spx_ctx* ctx, const double* c /* n */);

/* Counters of the bounded primal loop since spx_create or spx_reset: out[0]
 * flip passes, out[1] pivots whose leaving column went to its upper bound.
 * Counted on the device by the kernel that commits the pass. */
int spx_get_primal_flips(spx_ctx* ctx, int64_t out[2]);

/* Phase 1 of the bounded primal loop on (non-zero) or off, between any two
 * calls and under any algorithm (it takes effect when the context runs
 * SPX_ALGO_PRIMAL_BOX).  The entry check runs again before the next pass. */
int spx_set_primal_phase1(spx_ctx* ctx, int32_t on);

/* Entering rule of the bounded primal loop (SPX_PRIMAL_PRICING_*), between any
 * two calls and under any algorithm; takes effect with the next bounded primal
 * pass.  A change of rule restarts the steepest-edge weights.  SPX_ERR_ARG for
 * NULL or an unknown rule; SPX_ERR_STATE for STEEPEST while phase 1 is on
 * (unless spx_set_primal_phase_one_pricing chose STEEPEST for phase 1). */
int spx_set_primal_pricing(spx_ctx* ctx, int32_t rule);

/* Entering rule of the bounded primal loop's phase-1 passes where the loop's
 * rule is steepest edge: SPX_PRIMAL_PRICING_DANTZIG (the default: phase 1 and
 * steepest edge stay refused together, as above) or SPX_PRIMAL_PRICING_STEEPEST
 * (SPX_FLAG_PRIMAL_PHASE1_STEEPEST at spx_create).  Between any
 * two calls and under any algorithm.  Consulted only when phase 1 is on and the
 * loop's rule is STEEPEST; otherwise accepted and inert (a loop whose rule is
 * Dantzig prices both phases with Dantzig).  With it at STEEPEST,
 * spx_set_primal_phase1(on) under steepest edge and
 * spx_set_primal_pricing(STEEPEST) under phase 1 are accepted.  It restarts no
 * weights.  SPX_ERR_ARG for NULL or an unknown rule; SPX_ERR_STATE for DANTZIG
 * while phase 1 is on and the loop's rule is STEEPEST (the call would re-create
 * the refused state: switch one of the two off first).  (The name spells the
 * digit out: the bindings' header scan reads [a-z_] names.) */
int spx_set_primal_phase_one_pricing(spx_ctx* ctx, int32_t rule);

/* Entering rule of the bounded primal loop on a context that holds free columns
 * (spx_set_bounds_lu with -inf, +inf) where the loop's rule is steepest edge:
 * SPX_PRIMAL_PRICING_DANTZIG (the default: free columns and steepest edge stay
 * refused together) or SPX_PRIMAL_PRICING_STEEPEST
 * (SPX_FLAG_PRIMAL_FREE_STEEPEST at spx_create).  Between any two
 * calls and under any algorithm.  Consulted only where the context holds a free
 * column and the loop's rule is STEEPEST; otherwise accepted and inert.  With it
 * at STEEPEST, spx_set_bounds_lu with free columns under steepest edge and
 * spx_set_primal_pricing(STEEPEST) on a context that holds free columns are
 * accepted (with phase 1 on, spx_set_primal_phase_one_pricing(STEEPEST) is still
 * required).  It restarts no weights.  SPX_ERR_ARG for NULL or an unknown rule;
 * SPX_ERR_STATE for DANTZIG while the context holds a free column and the loop's
 * rule is STEEPEST (the call would re-create the refused state: set
 * SPX_PRIMAL_PRICING_DANTZIG with spx_set_primal_pricing first). */
int spx_set_primal_free_pricing(spx_ctx* ctx, int32_t rule);

/* Ratio test of the bounded primal loop's phase-1 passes from the next pass on:
 * SPX_PRIMAL_RATIO_TEXTBOOK (the default) or SPX_PRIMAL_RATIO_LONG_STEP (above;
 * DESIGN.md §7o).  Between any two calls and under any algorithm; inert outside
 * phase 1 (phase 1 off, a feasible basis, phase-2 passes, the other loops).  It
 * restarts and invalidates nothing: the basis, x_b, y, the weights, the counters
 * and the status stay.  Under any entering rule and with free columns.  A context
 * that never sets LONG_STEP allocates and launches nothing for it.  SPX_ERR_ARG
 * for NULL or an unknown rule.  (The name spells the digit out: the bindings'
 * header scan reads [a-z_] names.) */
int spx_set_primal_phase_one_ratio(spx_ctx* ctx, int32_t rule);

/* Counters of the long-step walk, kept on the device by the kernel that walks
 * (whether the pass then flips or pivots): out[0] rows passed since spx_create or
 * spx_reset, out[1] passes that passed at least one, out[2] the most in one
 * pass, out[3] the current rule (SPX_PRIMAL_RATIO_*). */
int spx_get_primal_long_steps(spx_ctx* ctx, int64_t out[4]);

/* Steepest-edge weights w[0..n) of the current basis, by column: the non-basic
 * entries are live (1 + ||B^-1 A_j||^2 as the recurrence keeps it, a pending
 * update applied first), a basic column's entry is unspecified.  SPX_ERR_STATE
 * under SPX_PRIMAL_PRICING_DANTZIG or outside SPX_ALGO_PRIMAL_BOX. */
int spx_get_primal_weights(spx_ctx* ctx, double* w /* n */);

/* How the bounded primal loop's steepest-edge weights restart for a warm basis
 * (SPX_PRIMAL_WEIGHTS_*), between any two calls and under any algorithm; takes
 * effect with the next restart and marks nothing stale.  SPX_ERR_ARG for NULL or
 * an unknown mode. */
int spx_set_primal_weight_init(spx_ctx* ctx, int32_t mode);

/* Recomputes the steepest-edge weights of the current basis exactly now (the
 * kernels of SPX_PRIMAL_WEIGHTS_EXACT), in either mode and at any basis.  A
 * recurrence still pending from the last pivot is dropped, not applied.  The
 * basis, x_b, y, the pivot count and the status are kept.  SPX_ERR_STATE under
 * SPX_PRIMAL_PRICING_DANTZIG or outside SPX_ALGO_PRIMAL_BOX. */
int spx_refresh_primal_weights(spx_ctx* ctx);

/* Sensitivity ranging at the optimum (bounds and the objective at
 * the range ends: spx_ranging_bound and spx_ranging_objective below, §7n): how
 * far one cost coefficient or one right-hand side may move, everything else
 * fixed, before the optimal basis changes, and what blocks it.  Conventions are the bounded
 * loops': maximise c.x, d = y.A - c, sigma_k = +1 for a non-basic column at its
 * lower bound and -1 at its upper bound, optimal means sigma_k d_k >= 0; tol =
 * opts.piv_tol, s_k = max(sigma_k d_k, 0).  Every result is a non-negative delta
 * (c_j may go down by down[j] and up by up[j]), +inf where nothing blocks, with
 * the index of what blocks (-1: nothing).  The index arrays may be NULL.
 *
 * spx_ranging_cost, n entries each.  Non-basic column j at lower: up = s_j, down
 * = +inf; at upper: down = s_j, up = +inf; free: both 0; the blocking column is
 * j itself.  Basic in row i: with T_ik = (row i of B^-1).A_k over the non-basic
 * k and g_k = sigma_k T_ik, up = min s_k / -g_k over g_k < -tol and down = min
 * s_k / g_k over g_k > tol; a free non-basic k with |T_ik| > tol blocks both at
 * 0; block_* is the entering column k, the smallest k on equal ratios.
 *
 * spx_ranging_rhs, m entries each.  With beta = column r of B^-1, x_i the basic
 * values clamped into [0, ub_B[i]] (general bounds: the shifted problem's values
 * and ranges): beta_i > tol blocks down at x_i / beta_i and, ub_B[i] finite, up at
 * (ub_B[i] - x_i) / beta_i; beta_i < -tol blocks up at x_i / -beta_i and, ub_B[i]
 * finite, down at (ub_B[i] - x_i) / -beta_i; a row whose basic column is free
 * never blocks.  leave_* = 2 row + side of the leaving row, side 1 = it leaves to
 * its upper bound; the smallest 2 row + side on equal ratios.
 *
 * Both run under SPX_ALGO_DUAL and SPX_ALGO_PRIMAL_BOX, one rank, explicit
 * replicated B^-1, with any bounds and pricing rule those loops take.
 * SPX_ERR_STATE, with nothing changed, unless the context's last status is
 * SPX_STATUS_OPTIMUM_FOUND and nothing was set since (spx_set_rhs / _cost /
 * _bounds / _bounds_lu / _basis / _algorithm and spx_reset all clear it), under
 * SPX_ALGO_PRIMAL (switch with spx_set_algorithm and solve), with more than one
 * rank or row-sharded B^-1.  A call changes nothing a later pass reads: basis,
 * placements, x_b, y, B^-1 and its pending pivot, steepest-edge weights and their
 * pending recurrence, pivot count and status are kept.  Buffers are allocated
 * by the first call; a context that never asks allocates and launches nothing. */
int spx_ranging_cost(spx_ctx* ctx, double* down, double* up, int64_t* block_down, int64_t* block_up);
int spx_ranging_rhs(spx_ctx* ctx, double* down, double* up, int64_t* leave_down, int64_t* leave_up);

/* Bound ranging, n entries each: how far one bound of column j
 * may move, everything else fixed, before the optimal basis changes.  The
 * conventions, the refusals and the promises are those of the two calls above;
 * leave_* = 2 row + side of the row that leaves (side 1: to its upper bound),
 * the smallest on equal ratios, -1 where nothing blocks, SPX_RANGING_OWN_BOUND
 * where the moving bound meets the column's own other bound first.
 *
 * Non-basic and not free (at lower or at upper alike): the bound the column sits
 * at moves by t and the column with it, x_B(t) = x_B - t alpha, alpha = B^-1 A_j.
 * up (t > 0): alpha_i > tol blocks at x_i / alpha_i (side 0), alpha_i < -tol with
 * ub_B[i] finite at (ub_B[i] - x_i) / -alpha_i (side 1).  down (t < 0): alpha_i <
 * -tol blocks at x_i / -alpha_i (side 0), alpha_i > tol with ub_B[i] finite at
 * (ub_B[i] - x_i) / alpha_i (side 1).  A row whose basic column is free never
 * blocks.  At lower, up is also capped by the column's range ub_j = u_j - l_j, at
 * upper down is: SPX_RANGING_OWN_BOUND, only where strictly smaller than every
 * row's ratio (a fixed column, ub_j = 0, by the same rule).  Non-basic and free:
 * no bound to move, both +inf with -1.  Basic in row i: up = x_i, how far its
 * lower bound may rise (2 i; a free column: +inf, -1); down = ub_B[i] - x_i, how
 * far its upper bound may fall (2 i + 1; no upper bound: +inf, -1).  For a
 * non-basic slack of row r at lower, up is spx_ranging_rhs's down[r] and down
 * its up[r], values and indices bit for bit. */
#define SPX_RANGING_OWN_BOUND (-2)
int spx_ranging_bound(spx_ctx* ctx, double* down, double* up, int64_t* leave_down, int64_t* leave_up);

/* The objective at the two ends of every range: down / up are the arrays the
 * matching call returned (what = SPX_RANGING_COST: n entries, _RHS: m, _BOUND: n).
 * Host arithmetic in fp64 from the context's own readbacks; z is spx_objective's,
 * in the caller's variables.  Cost: obj_up = z + up x_j, obj_down = z - down x_j,
 * x as spx_get_primal gives it.  Right-hand side: z +- delta y_r.  Bound, a
 * non-basic column that is not free: obj_up = z - up d_j, obj_down = z + down d_j
 * with d = y.A - c; basic or free: z both ways.  A multiplier that is exactly 0
 * gives z even where the delta is +inf; otherwise +inf propagates with its sign.
 * The refusals of the ranging calls apply; SPX_ERR_ARG for an unknown `what`. */
#define SPX_RANGING_COST  0
#define SPX_RANGING_RHS   1
#define SPX_RANGING_BOUND 2
int spx_ranging_objective(spx_ctx* ctx, int32_t what, const double* down, const double* up, double* obj_down,
                          double* obj_up);

/* Phase-1 counters of the bounded primal loop, kept on the device by the kernel
 * that commits the pass: out[0] phase-1 passes since spx_create or spx_reset
 * (flip passes included), out[1] phase-1 pivots, out[2] rows out of their
 * bounds at the last entry check, out[3] rows out of their bounds now (as of
 * the last classification). */
int spx_get_primal_phase1(spx_ctx* ctx, int64_t out[4]);

/* Upper bounds ub[0..n) of all columns, slacks included (+inf = none, NULL =
 * none at all); lower bounds are 0 (other lower bounds: spx_set_bounds_lu below;
 * this call clears them).  The basis and the pivot count are kept and
 * the status is back to running: a non-basic column at an upper bound that
 * became infinite goes to lower, every non-basic column is put on its dual
 * feasible side and x_b is recomputed, so spx_solve re-optimises from the old
 * basis.  B^-1 is untouched: steepest-edge weights stay valid.  SPX_ERR_ARG for
 * a NaN or negative bound (the message names the column); SPX_ERR_STATE unless
 * one rank, replicated B^-1, SPX_ALGO_DUAL or SPX_ALGO_PRIMAL_BOX and not
 * between spx_price and spx_pivot, and (DUAL) when a column with e_j < -eps has
 * no upper bound.  Under SPX_ALGO_PRIMAL_BOX the placements are kept as they
 * are (no dual normalisation), and the entry check runs before the next pass. */
int spx_set_bounds(spx_ctx* ctx, const double* ub /* n, +inf = none */);
int spx_get_bounds(spx_ctx* ctx, double* ub /* n */);

/* General bounds lb[j] <= x_j <= ub[j] of all columns, slacks included
 * (DESIGN.md §7j).  lb NULL = all 0, ub NULL = all +inf.  Accepted per column:
 *   shifted  lb[j] finite of any sign, ub[j] >= lb[j] or +inf (lb[j] == ub[j]: a
 *            fixed column).  The device keeps x'_j = x_j - lb[j] in [0, ub[j] -
 *            lb[j]] and the effective right-hand side b - A.lb - sum_{j at upper}
 *            (ub[j] - lb[j]) A_j; both bounded loops, every pricing rule, phase 1
 *            and the long-step ratio test run unchanged on the shifted problem.
 *   free     lb[j] = -inf and ub[j] = +inf: SPX_ALGO_PRIMAL_BOX with
 *            SPX_PRIMAL_PRICING_DANTZIG, or with SPX_PRIMAL_PRICING_STEEPEST after
 *            spx_set_primal_free_pricing(STEEPEST).  A non-basic free column sits
 *            at 0 and is a candidate when |d_j| > eps (key -|d_j|, under steepest
 *            edge -d_j^2 / gamma_j; it moves up when d_j < 0, down otherwise); it never flips; a row whose basic column
 *            is free never blocks, is never out of its bounds and never leaves.
 * Every readback is in the caller's variables: spx_get_primal gives lb[j] or
 * ub[j] exactly for a non-basic column, spx_get_state's x_b includes the basic
 * column's lower bound, spx_objective and spx_solve's z include sum_j c_j lb[j]
 * (summed on the host over ascending j with the current c).  y, reduced costs,
 * traces, weights and counters are those of the shifted problem, which has the
 * same ones.  Otherwise as spx_set_bounds, whose refusals apply; in addition
 * SPX_ERR_ARG for NaN, lb[j] = +inf, lb[j] > ub[j] and for an upper-only column
 * (lb[j] = -inf with a finite ub[j]); SPX_ERR_STATE for a free column on a
 * context that runs SPX_ALGO_DUAL (spx_set_algorithm(SPX_ALGO_DUAL) on a context
 * holding one is refused in the same way: a non-basic free column has no dual
 * feasible side unless d_j = 0) or whose entering rule is
 * SPX_PRIMAL_PRICING_STEEPEST (spx_set_primal_pricing refuses that rule on a
 * context holding one) unless spx_set_primal_free_pricing chose STEEPEST.  A
 * refused call changes nothing.  With lb NULL or all 0
 * the call is spx_set_bounds(ctx, ub): the same kernels and the same bits.
 * spx_set_bounds(ctx, ub) on a context that had lower bounds clears them;
 * spx_get_bounds returns the caller's ub. */
int spx_set_bounds_lu(spx_ctx* ctx, const double* lb /* n; NULL = all 0; -inf = no lower bound */,
                      const double* ub /* n; NULL = all +inf */);
int spx_get_bounds_lu(spx_ctx* ctx, double* lb /* n */, double* ub /* n */);

/* The full primal vector x[0..n): basic values, u_j for a non-basic column at
 * its upper bound (at_upper[j] = 1), its lower bound otherwise (0 without
 * spx_set_bounds_lu, and for a free column). */
int spx_get_primal(spx_ctx* ctx, double* x /* n */, int8_t* at_upper /* n, may be NULL */);

/* Whole solve, device-resident: at most max_iter loop passes (reference
 * MAX_ITER, v4:19, do/while at v4:286-359).  Writes z, x_b[m], b_ixs[m] (basis
 * order) for every status (the reference writes them only on optimum);
 * pivots = pivots made (the reference's loop counter).  Any output may be
 * NULL.  Continues from the current basis (call spx_reset to restart). */
int spx_solve(spx_ctx* ctx, int64_t max_iter, double* z, int64_t* b_ixs,
              double* x_b, int32_t* status, int64_t* pivots);

/* Run up to k further pivots with no host synchronisation between them; one
 * sync at the end.  status: SPX_STATUS_MAX_ITER while the loop can go on. */
int spx_iterate(spx_ctx* ctx, int64_t k, int32_t* status, int64_t* pivots);

/* Step-wise API (tests/debugging; each call synchronises).
 * spx_price: pricing + entering argmin (+ cross-rank MINLOC).  p = entering
 *   column (first index on ties), min_e = its reduced cost, optimal = 1 when
 *   min_e >= -eps.
 * spx_pivot: apply the pending rank-1 update of B^-1 fused with FTRAN
 *   (alpha = B^-1 A_p), ratio test + leaving argmin, E_q, x_b, y, c_B, basis
 *   bookkeeping.  Requires a preceding spx_price.  status after the pivot. */
int spx_price(spx_ctx* ctx, int64_t* p, double* min_e, int32_t* optimal);
int spx_pivot(spx_ctx* ctx, int64_t* q, int32_t* status);

/* Current state (any pointer may be NULL).  binv_rowmajor: m*m, B^-1[i][k] at
 * i*m + k (with the pending rank-1 update applied). */
int spx_get_state(spx_ctx* ctx, double* x_b, int64_t* b_ixs, double* y,
                  double* c_b, double* binv_rowmajor, int32_t* status,
                  int64_t* pivots);

/* Reduced costs e_j = -c_j + y.A_j for all n columns from the current y
 * (debug/parity; basic columns included, like v4:288-290). */
int spx_reduced_costs(spx_ctx* ctx, double* e);

/* Objective z = c_B . x_b (v4:365), computed on the device. */
int spx_objective(spx_ctx* ctx, double* z);

/* Pivot trace (opts.trace_cap > 0): copies the first min(pivots made,
 * trace_cap, cap) pivots' entering columns into p[] and leaving rows into q[]
 * (either may be NULL) and stores that count in *count.  Indexed by pivot
 * number, so a spx_reset / re-solve overwrites it. */
int spx_get_trace(spx_ctx* ctx, int64_t* p, int64_t* q, int64_t cap, int64_t* count);

/* Devex / steepest-edge pricing weights w_j of every column (n entries; the
 * non-basic ones are the live weights, as updated by the last pricing pass).
 * SPX_ERR_STATE under Dantzig pricing. */
int spx_get_weights(spx_ctx* ctx, double* w);

/* With SPX_FLAG_TIMING: total device milliseconds and launch counts of the
 * pricing kernel and of the fused update kernel since the last call (resets).
 * Dual loop: the dual ratio-test kernel and the FTRAN + update kernel. */
int spx_kernel_times(spx_ctx* ctx, double* price_ms, int64_t* price_launches,
                     double* update_ms, int64_t* update_launches);

/* With SPX_FLAG_TIMING, bounded primal loop with phase 1 on: total device
 * milliseconds and count of the v.B^-1 step (k_pbox_vtb and its reduction) of
 * the four-step passes since the last call (resets); a step that found nothing
 * to do (phase 2, y current) is counted with its near-zero time.  Under
 * SPX_PRIMAL_PRICING_STEEPEST the same counters carry the tau = alpha^T B^-1
 * step of every pass (a pass without a pivot with its near-zero time); a
 * phase-1 pass under steepest edge (spx_set_primal_phase_one_pricing) has both
 * steps and counts two. */
int spx_pbox_vtb_times(spx_ctx* ctx, double* ms, int64_t* launches);

/* With SPX_FLAG_TIMING: total device milliseconds and count of the exact weight
 * recomputations (SPX_PRIMAL_WEIGHTS_EXACT restarts and
 * spx_refresh_primal_weights; B^-1 brought current, the product, the slack
 * norms and the sum) since the last call (resets). */
int spx_pbox_wexact_times(spx_ctx* ctx, double* ms, int64_t* launches);

/* With SPX_FLAG_TIMING: total device milliseconds and count, since the last call
 * (resets), of [0] the cost rangings (reduced costs, B^-1 brought current, the
 * gather, the product and the merge) and [1] the right-hand-side rangings (B^-1
 * brought current, the stream and the merge). */
int spx_ranging_times(spx_ctx* ctx, double ms[2], int64_t launches[2]);

/* With SPX_FLAG_TIMING: total device milliseconds and count of the bound
 * rangings (B^-1 brought current, the gather, the product, the merge and the
 * basic columns) since the last call (resets). */
int spx_ranging_bound_times(spx_ctx* ctx, double* ms, int64_t* launches);

/* With SPX_FLAG_TIMING: device milliseconds summed since the last call (resets)
 * of out[0] the pricing kernel, out[1] pricing + the cross-rank MINLOC
 * exchange (RCCL all-gather; == out[0] at one rank), out[2] the update kernel;
 * passes = timed passes. */
int spx_pass_times(spx_ctx* ctx, double out[3], int64_t* passes);

/* With SPX_FLAG_STAMPS: microseconds summed since the last call of, per
 * kernel, the body (earliest workgroup start -> last workgroup's ticket) and
 * the last-workgroup tail (final reduction; for the update kernel also E_q,
 * r, x_b, y and the basis bookkeeping).  out[0..3] = price body, price tail,
 * update body, update tail; out[4..8] = update-tail sub-phases (partials ->
 * q, s_y dot, block sum, bookkeeping, -); out[9..12] = update prologue
 * (earliest workgroup start -> earliest row stream start), update drain
 * (latest stream end -> last ticket), price prologue, price drain;
 * out[13..17] = the update kernel's workgroup 0, from its start to: status
 * read, entering column known, row stream start, its wave 0's stream end,
 * partial published.  Resets.
 * Loop passes that defer the pricing tail (window passes and explicit passes
 * at m <= 2048 on one rank, Params::defer_price) have no pricing ticket, so
 * out[0], out[1], out[11] and out[12] stay 0 for them; the per-workgroup
 * clocks of spx_wg_times cover those passes.  The step-wise API
 * (spx_price / spx_pivot) keeps the pricing tail and fills every slot. */
#define SPX_PHASES 18
int spx_phase_times(spx_ctx* ctx, double out[SPX_PHASES]);

/* With SPX_FLAG_STAMPS: the compact fold's (k_cfold) per-workgroup clocks of
 * its last launch, 8 words per workgroup (up to 1024 workgroups): entry,
 * coefficients staged, R in LDS, tiles done, the y / xw updates done, the
 * arrival counted (s_memrealtime, 100 MHz).  count = words written. */
int spx_fold_times(spx_ctx* ctx, uint64_t* out, int64_t cap, int64_t* count);

/* Diagnostic (SPX_FLAG_STAMPS, compact window passes): the clocks of the
 * last two passes, s_memrealtime ticks (100 MHz), one block per pass parity
 * (iteration & 1, parity 0 first).  A block holds, per workgroup g of that
 * pass's FTRAN launch (k_ftran_bc), 4 ticks at k = 0 entry, 1 entering column
 * known, 2 A_p on the column list in LDS (the p-dependent round trip done),
 * 3 partial published (4 grid values); then per workgroup h of its pricing
 * launch (k_price) 4 ticks: start, end of its column loop, the deferred
 * ratio-test tail reduced, the staging in LDS (4 price grid values); then
 * the tick at which the FTRAN tail had issued the pivot's
 * bookkeeping (1 value), then the tick at which the diagnostic one-wave
 * kernel launched before the FTRAN pass started (SPX_DIAG_MARK=1; 1 value),
 * then the tick k_price's workgroup 0 had issued the deferred tail's
 * bookkeeping (1 value).
 * Copies min(cap, 2 (4 grid + 4 price grid + 3)) values; *count = grid. */
int spx_wg_times(spx_ctx* ctx, uint64_t* out, int64_t cap, int64_t* count);

/* With SPX_FLAG_TIMING and the persistent loop kernel (spx_config out[8]
 * = 1): out[0] device milliseconds of the loop launches (hipEvents) and out[1]
 * the passes they ran, since the last call; out[2..4] microseconds summed
 * over passes of the in-kernel phases seen by workgroup 0 (s_memrealtime):
 * pricing to grid barrier 1, FTRAN + ratio test to barrier 2, tail to the
 * next pass; passes = passes with a phase split; out[5] device milliseconds
 * of the window folds launched between loop launches (hipEvents) and out[6]
 * their count.  Resets. */
#define SPX_LOOP_FIELDS 7
int spx_loop_times(spx_ctx* ctx, double out[SPX_LOOP_FIELDS], int64_t* passes);

/* Geometry and algorithmic bytes.  bytes_price: one pricing launch on this
 * rank (8*(m+1)*local non-basic columns), bytes_update: the B^-1 bytes per
 * pivot — 16*m*m for the explicit rank-1 update, or
 * 8*m*m*(1 + 2/(window-1)) for the eta window (stream + amortised fold).
 * With compact pricing (spx_config [16]) bytes_price is the mean pricing
 * launch of a window under the anchor period P (spx_dispatch_stats [11]): the
 * compact passes, and one dense stream per P windows; the dw carry's
 * 8*n*(window+2) bytes per carried window join the fold in bytes_update. */
int spx_info(spx_ctx* ctx, int64_t* m, int64_t* n, int64_t* ld,
             int64_t* local_nonbasic, double* bytes_price, double* bytes_update);

/* Resolved configuration: out[0] window (0 = explicit B^-1), [1] pricing
 * threads per workgroup, [2] pricing workgroups, [3] pricing LDS mode (0 y
 * in global, 1 y in LDS, 2 y and the window base row in LDS), [4] update
 * threads per workgroup, [5] update rows per wave, [6] update workgroups,
 * [7] passes per captured hipGraph (0 = eager), [8] persistent loop kernel
 * in use (1) or not (0), [9] its threads per workgroup, [10] window tableau
 * (SPX_FLAG_TABLEAU) in use, [11] workgroups of the persistent loop kernel,
 * [12] the ratio-test tail deferred into the next pricing pass (1; compact
 * window passes on one rank, SPX_DEFER_TAIL=0 turns it off) or run by the
 * FTRAN pass's last workgroup (0), [13] the window fold updates only B_w's
 * listed (non-unit) columns (1: k_cfold; SPX_DENSE_FOLD=1 turns it off) or
 * the dense B_w (0), [14] k_ftran_bc rows per wave (0: not in use), [15]
 * (after spx_mbox_attach) loop passes exchange through the mailboxes inside
 * k_price and k_ftran_bc (1: the fused exchange; SPX_MBOX_FUSED=0 turns it
 * off) or with a k_exchange launch per pass (0), [16] the window's passes
 * after its first price from the listed rows of A (1: compact pricing, one
 * rank over the compact operand, Dantzig or Devex; SPX_DENSE_PRICE=1 turns it
 * off) or stream A (0: also once the list has outgrown the stored rows,
 * SPX_CPRICE_CAP).  With [16] = 1 the first pass of a window is compact too
 * wherever dw was carried across the fold (spx_dispatch_stats [10], [11];
 * SPX_DW_ANCHOR). */
#define SPX_CONFIG_FIELDS 17
int spx_config(spx_ctx* ctx, int32_t out[SPX_CONFIG_FIELDS]);

/* Where the dual and the bounded primal loop keep the vectors their kernels
 * read, as their setup resolved it from L = round_up(m, 128) against 150 KiB
 * of LDS: 24 L bytes fit up to L = 6400, 16 L up to L = 9600, 8 L up to L =
 * 19200.  1 = staged in LDS, 0 = read from global memory, -1 = that loop's
 * setup has not run yet (it runs on first use).
 *   out[0] dual loop: rho and y of the ratio test (16 L bytes)
 *   out[1] dual loop: the pending row and A_p of the update (16 L)
 *   out[2] dual loop, steepest edge: the update's operands (24 L must fit)
 *   out[3] ... rho among them (1), or read from global memory (0:
 *          SPX_DUAL_RHO_LDS=0, and wherever out[2] is 0)
 *   out[4] bounded primal loop: y of the pricing pass (8 L)
 *   out[5] bounded primal loop: the pending row and A_p of the update (16 L)
 *   out[6] bounded primal loop, steepest edge: vectors of the pricing pass in
 *          LDS, 3 (y, rho, tau), 1 (y) or 0 (SPX_PBOX_SE_LDS asks for fewer);
 *          -1 until the first steepest-edge pass or weight readback
 *   out[7] 1: a slack column is priced from its one entry (A[:, n-m:] = I),
 *          0: streamed like any column (SPX_DENSE_SLACKS=1, or other slacks)
 * SPX_FLAG_GLOBAL_Y turns out[0], [2], [4] and [6] to 0.  SPX_DUAL_LDS_CAP and
 * SPX_PBOX_LDS_CAP (bytes; tests) stand in for the 150 KiB where they are
 * smaller, so the layouts of a large m can be run at a small one; they are
 * read when the loop's setup runs and never raise the cap. */
#define SPX_LOOP_LAYOUT_FIELDS 8
int spx_loop_layout(spx_ctx* ctx, int32_t out[SPX_LOOP_LAYOUT_FIELDS]);

/* Columns of B^-1 the FTRAN stream reads per row: m, or with the eta window's
 * compact operand (A[:, n-m:] = I, two-kernel passes; SPX_DENSE_FTRAN=1 turns
 * it off) the non-unit columns of B_w as of the last fold: B_w is I except in
 * the columns of rows whose slack has left the basis. */
int spx_ftran_cols(spx_ctx* ctx, int32_t* cols);

/* Compact pricing's row form (DESIGN.md §4 "Compact pricing"): out[0] = the
 * longest list of rows whose columns a compact pass reads as coalesced rows
 * handed to the lanes through LDS (SPX_CPRICE_ROWS, 512 by default, clamped
 * to the rows of the compact copy of A; 0 = every pass gathers term by term,
 * as a pass with a longer list does), out[1] = the bytes of LDS each wave of
 * the pass holds for it.  Both 0 where the context does not price compactly.
 * Either form computes the same bits. */
int spx_cprice_rows(spx_ctx* ctx, int32_t out[2]);

/* What the loop has enqueued since spx_create (monotone counters, so a
 * caller can difference them around a timed region): out[0] passes launched
 * eagerly (step-wise spx_price/spx_pivot included), [1] captured-hipGraph
 * replays, [2] passes inside those replays, [3] persistent loop-kernel
 * launches, [4] passes inside them, [5] eta-window folds (k_fold) enqueued,
 * [6] the window position (pivots since the last fold + 1; a fold is due
 * before the next pass when it equals [7]), [7] the window size KW (0 =
 * explicit B^-1), [8] persistent launches whose grid was found not
 * co-resident (another stream or process held CUs; the context then
 * switched to two-kernel passes and made those pivots that way), [9] times
 * the batch hipGraph was built (captured, instantiated and uploaded; 0 or 1
 * per context, rebuilt once after spx_mbox_attach).  A context that prices
 * compactly (spx_config [16]) builds every batch it can replay in that one go
 * (dense pricing, compact pricing opening with an anchor, compact pricing
 * carrying dw), so that a solve crossing into dense pricing builds nothing.
 * [10] compact-priced windows opened by an anchor: the dense pricing pass that
 * also stores dw[j] = y_w.A_j - c_j, with k_dw_basic.  The first window, the
 * one after a reset, rebuild, reinversion, spx_set_basis, state readback or
 * switch of pricing mode, and every P-th fold since the last anchor open so;
 * every other fold carries dw to the new y_w from the stored Wt rows and
 * opens its window with a compact pass.  [11] that period P (default 32;
 * SPX_DW_ANCHOR=N sets it: 1 = every fold anchors, nothing is carried; 0 =
 * no fold anchors, reported as -1), or 0 where dw is not carried (dense
 * pricing, the dense fold, P = 1).  A setting, not a count: spx_config keeps
 * its 17 fields under this ABI version, so the period is reported here. */
#define SPX_DISPATCH_FIELDS 12
int spx_dispatch_stats(spx_ctx* ctx, int64_t out[SPX_DISPATCH_FIELDS]);

/* Capture, instantiate and upload the batch hipGraph now, so that no later
 * spx_iterate pays for it.  spx_create does this itself on one rank; with a
 * communicator or mailboxes the graph can only be captured once they are
 * attached (spx_attach_comm / spx_mbox_attach), and spx_iterate would
 * otherwise build it on its first call that spans a whole batch.  A no-op
 * when the graph exists, for eager dispatch (graph_batch < 0, timing) and for
 * the persistent loop kernel.  If RCCL refuses the capture the context runs
 * eager passes (spx_comm_info's graph_fallback). */
int spx_prepare(spx_ctx* ctx);

/* Host-only helpers (no device needed), shared with the device code:
 * spx_shard_range: this rank's column shard — structural columns
 *   [out[0], out[1]) and slack columns [out[2], out[3]) (global indices).
 * spx_minloc_merge: the cross-rank MINLOC rule applied to the all-gathered
 *   candidates — smallest value, then smallest global index (CUB ArgMin's
 *   first-index semantics, v4:294). */
int spx_shard_range(int64_t m, int64_t n, int32_t rank, int32_t nranks, int64_t out[4]);
int spx_minloc_merge(const double* vals, const int64_t* idx, int32_t count,
                     double* best_val, int64_t* best_idx);

const char* spx_last_error(void);
const char* spx_status_string(int32_t status);
int spx_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
