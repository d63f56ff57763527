// spx_api_dual.cpp — the dual simplex loop's host side (kernels: spx_dual.h):
// its state (DualState, spx_ctx.h, with the invariants), the pass loop, the
// feasibility check and boxed entry normalisation, the hooks through which the
// rest of the runtime (spx_api.cpp) touches any of it, and the entry points
// that are the dual loop's alone.
#include <cmath>
#include <cstring>

#include "spx_ctx.h"

using namespace spx;

namespace spx_host {

namespace {

// The only writers of DualState::checked and ::w_stale.  Who calls them:
//   event                                  checked          w_stale
//   dual_setup (first use)                 -                true
//   do_reset                               false            true
//   reinvert_basis (spx_reinvert,          kept             true
//     spx_set_rhs, refactor_every)
//   spx_set_basis                          false            true (its reinversion)
//   spx_set_algorithm, either way          false            true
//   spx_set_dual_pricing, another rule     kept             true
//   iterate_dual under Dantzig             -                true
//   spx_set_bounds past its early return   false, then true kept
//                                          (normalisation)
//   dual_check_feasible / box_normalise ok true             -
//   dual_refresh_weights                   -                false
//   spx_set_dual_ratio                     kept             kept
void feasibility_unknown(spx_ctx* x) { x->dual.checked = false; }  // the basis or its bounds were set from outside
void feasibility_verified(spx_ctx* x) { x->dual.checked = true; }  // the check (boxed: the normalisation) passed
void weights_lost(spx_ctx* x) { x->dual.w_stale = true; }          // B^-1 or the rule changed with no steepest pass keeping w
void weights_recomputed(spx_ctx* x) { x->dual.w_stale = false; }   // k_dual_norms enqueued

// e_j = y.A_j - c_j of every column and nb_pos (>= 0: non-basic) on the host
int fetch_reduced_costs(spx_ctx* x, std::vector<double>& e, std::vector<int32_t>& pos) {
    const size_t n = (size_t)x->n;
    HIP_TRY(launch_reduced_costs(x->P, x->dual.e, x->stream));
    e.resize(n);
    pos.resize(n);
    HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipMemcpy(e.data(), x->dual.e, n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pos.data(), x->P.nb_pos, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SPX_OK;
}

// a non-basic column with e_j < -eps and no upper bound has no dual feasible side
int no_feasible_side(const spx_ctx* x, double e_j, size_t j) {
    return fail(SPX_ERR_STATE, "basis is not dual feasible (reduced cost %g at column %lld, eps %g): the "
                "column has no upper bound to sit at, and the dual simplex loop needs e_j >= -eps at a "
                "lower bound", e_j, (long long)j, x->opts.eps);
}

// up[j] = 1: column j is non-basic at its upper bound (all 0 when not boxed; the
// stream is drained).  stale: the device's at_upper marked some basic column
// (spx_set_basis of a column that sat at upper).
int fetch_placements(spx_ctx* x, std::vector<int8_t>& up, bool* stale = nullptr) {
    const size_t n = (size_t)x->n;
    up.assign(n, 0);
    if (stale) *stale = false;
    if (!x->dual.boxed) return SPX_OK;
    std::vector<int32_t> pos(n);
    HIP_TRY(hipMemcpy(up.data(), x->dual.args.at_upper, n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pos.data(), x->P.nb_pos, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t j = 0; j < n; ++j) {
        if (stale && up[j] && pos[j] < 0) *stale = true;
        up[j] = (up[j] && pos[j] >= 0) ? 1 : 0;
    }
    return SPX_OK;
}

// ... and x_b = B^-1 b_eff from the effective right-hand side (B^-1 untouched)
int box_recompute_xb(spx_ctx* x) {
    SPX_TRY(box_sync(x));
    HIP_TRY(launch_box_xb(x->P, x->dual.cfg, x->stream));
    return SPX_OK;
}

// Boxed entry normalisation: every non-basic column on the side where its
// reduced cost is dual feasible (e_j >= -eps at lower, e_j <= eps at upper;
// |e_j| <= eps keeps its side); x_b recomputed when a placement changed (or
// `force`).  A column with e_j < -eps and no upper bound has no such side.
int box_normalise(spx_ctx* x, bool force) {
    std::vector<double> e;
    std::vector<int32_t> pos;
    std::vector<int8_t> up;
    bool changed = false;
    SPX_TRY(fetch_reduced_costs(x, e, pos));
    SPX_TRY(fetch_placements(x, up, &changed));  // (a basic column has no placement)
    const size_t n = (size_t)x->n;
    const double eps = x->opts.eps;
    for (size_t j = 0; j < n; ++j) {
        if (pos[j] < 0) continue;
        if (e[j] < -eps) {
            if (!std::isfinite(x->dual.ub[j])) return no_feasible_side(x, e[j], j);
            if (!up[j]) { up[j] = 1; changed = true; }
        } else if (e[j] > eps && up[j]) {
            up[j] = 0;
            changed = true;
        }
    }
    if (changed) HIP_TRY(hipMemcpy(x->dual.args.at_upper, up.data(), n, hipMemcpyHostToDevice));
    if (changed || force) SPX_TRY(box_recompute_xb(x));
    feasibility_verified(x);
    return SPX_OK;
}

// min over the non-basic columns of e_j = y.A_j - c_j must be >= -eps (x_b and
// y are current: nothing of theirs is pending when the dual loop starts)
int dual_check_feasible(spx_ctx* x) {
    if (x->dual.boxed) return box_normalise(x, false);
    std::vector<double> e;
    std::vector<int32_t> pos;
    SPX_TRY(fetch_reduced_costs(x, e, pos));
    double worst = INFINITY;
    int64_t at = -1;
    for (int64_t j = 0; j < x->n; ++j)
        if (pos[(size_t)j] >= 0 && !(e[(size_t)j] >= worst)) {
            worst = e[(size_t)j];
            at = j;
        }
    if (at >= 0 && !(worst >= -x->opts.eps))
        return fail(SPX_ERR_STATE, "basis is not dual feasible (reduced cost %g at column %lld, eps %g): the dual "
                    "simplex loop needs every non-basic e_j >= -eps", worst, (long long)at, x->opts.eps);
    feasibility_verified(x);
    return SPX_OK;
}

// Steepest edge: the weights of the current basis from scratch where no pass
// has kept them (k_dual_norms; between passes, nothing of the dual loop's in flight)
int dual_refresh_weights(spx_ctx* x) {
    if (!x->dual.w_stale) return SPX_OK;
    HIP_TRY(launch_dual_norms(x->P, x->dual.args, x->dual.cfg, x->stream));
    weights_recomputed(x);
    return SPX_OK;
}

// the bound-flipping ratio test runs where there is something to flip
bool long_step(const spx_ctx* x) { return x->dual.boxed && x->dual.ratio == SPX_DUAL_RATIO_LONG_STEP; }

// its buffers, on first use (n list slots: the non-basic count never exceeds n)
int long_setup(spx_ctx* x) {
    DualState& d = x->dual;
    if (d.args.lrec) return SPX_OK;
    const size_t n = (size_t)x->n;
    SPX_TRY(x->alloc(&d.args.rkey, n));
    SPX_TRY(x->alloc(&d.args.rcd, 2 * n));
    SPX_TRY(x->alloc(&d.args.flist, n));
    SPX_TRY(x->alloc(&d.args.v, (size_t)x->L));
    SPX_TRY(x->alloc(&d.args.fl, (size_t)x->L));
    SPX_TRY(x->alloc(&d.args.lrec, 1));
    d.args.walk_global = env_on("SPX_DUAL_LONG_GLOBAL") ? 1 : 0;  // (test: the walk's path for more than 16,384 list slots)
    return SPX_OK;
}

// the launch that commits the last pass's pivot (and its flips)
int enqueue_dual_finish(spx_ctx* x) {
    const DualState& d = x->dual;
    const bool se = d.rule == SPX_DUAL_PRICING_STEEPEST;
    if (long_step(x)) HIP_TRY(launch_dual_step_long(x->P, d.args, se, true, x->stream));
    else HIP_TRY(launch_dual_step(x->P, d.args, se, d.boxed, true, x->stream));
    return SPX_OK;
}

// One dual pass: leaving row + pivot row, ratio test, FTRAN + update; five
// launches with the bound-flipping ratio test (spx_dual.h).
int enqueue_dual_pass(spx_ctx* x, hipEvent_t p0, hipEvent_t p1, hipEvent_t u0, hipEvent_t u1) {
    const DualState& d = x->dual;
    const bool se = d.rule == SPX_DUAL_PRICING_STEEPEST;
    if (long_step(x)) {
        HIP_TRY(launch_dual_step_long(x->P, d.args, se, false, x->stream));
        HIP_TRY(launch_dual_price_long(x->P, d.args, d.cfg, x->stream, p0, p1));
        HIP_TRY(launch_dual_long(x->P, d.args, x->stream));
        HIP_TRY(launch_dual_flips(x->P, d.args, x->b, x->stream));
        // (timing: the "exchange end" event closes the walk and the flips, so
        // spx_pass_times' out[1] - out[0] is k_dual_long + k_dual_flips)
        if (p0) HIP_TRY(hipEventRecord(x->ev_xend[x->n_price - 1], x->stream));
        HIP_TRY(launch_dual_update_long(x->P, d.args, d.cfg, se, x->stream, u0, u1));
        return SPX_OK;
    }
    HIP_TRY(launch_dual_step(x->P, d.args, se, d.boxed, false, x->stream));
    HIP_TRY(launch_dual_price(x->P, d.args, d.cfg, d.boxed, x->stream, p0, p1));
    if (p0) HIP_TRY(hipEventRecord(x->ev_xend[x->n_price - 1], x->stream));
    HIP_TRY(launch_dual_update(x->P, d.args, d.cfg, se, x->stream, u0, u1));
    return SPX_OK;
}

}  // namespace

// The dual simplex loop's scope (spx_dual.h): one rank, explicit B^-1, Dantzig
// pricing, no Harris pass.
const char* dual_conflict(const spx_opts& o, int win) {
    if (o.nranks > 1) return "on more than one rank (nranks > 1: no column or row sharding)";
    if (o.flags & SPX_FLAG_COMM1) return "through a communicator (SPX_FLAG_COMM1)";
    if (o.flags & SPX_FLAG_TABLEAU) return "with the window tableau (SPX_FLAG_TABLEAU)";
    if (win > 0) return "on an eta window (it needs the explicit B^-1: window -1)";
    if (o.ratio_test == SPX_RATIO_HARRIS) return "with the Harris ratio test";
    if (o.pricing != SPX_PRICING_DANTZIG) return "with Devex or steepest-edge pricing";
    return nullptr;
}

void dual_on_create(spx_ctx* x) {
    x->dual.rule = (x->opts.flags & SPX_FLAG_DUAL_STEEPEST) ? SPX_DUAL_PRICING_STEEPEST : SPX_DUAL_PRICING_DANTZIG;
    x->dual.ratio = (x->opts.flags & SPX_FLAG_DUAL_LONG_STEP) ? SPX_DUAL_RATIO_LONG_STEP : SPX_DUAL_RATIO_TEXTBOOK;
}

// (spx_create with SPX_ALGO_DUAL, spx_set_algorithm, or the first entry point that needs a buffer)
int dual_setup(spx_ctx* x) {
    DualState& d = x->dual;
    if (d.args.rho) return SPX_OK;
    // steepest edge, k_dual_update's third operand rho: staged in LDS, or (SPX_DUAL_RHO_LDS=0) read from global memory;
    // SPX_DUAL_LDS_CAP (tests): fewer bytes of LDS than the built-in cap, so that the layouts of a large m run at a small one
    HIP_TRY(dual_prepare(x->P, x->cus, x->opts.price_grid, (x->opts.flags & SPX_FLAG_GLOBAL_Y) != 0,
                         !env_off("SPX_DUAL_RHO_LDS"), env_bytes("SPX_DUAL_LDS_CAP"), &d.cfg));
    SPX_TRY(x->alloc(&d.args.tau, (size_t)x->L));
    SPX_TRY(x->alloc(&d.args.wex, (size_t)x->L));
    SPX_TRY(x->alloc(&d.args.w, (size_t)x->L));
    weights_lost(x);  // (a fresh buffer)
    SPX_TRY(x->alloc(&d.args.rho, (size_t)x->L));
    SPX_TRY(x->alloc(&d.args.parts, (size_t)d.cfg.price_grid));
    SPX_TRY(x->alloc(&d.args.rec, 1));
    SPX_TRY(x->alloc(&d.e, (size_t)x->n));
    d.args.price_grid = d.cfg.price_grid;
    d.args.feas_tol = x->opts.feas_tol;
    d.args.piv_tol = x->opts.piv_tol;
    return SPX_OK;
}

int box_sync(spx_ctx* x) {
    if (!x->dual.boxed) return SPX_OK;
    if (x->dual.shifted)  // some lower bound is not 0: the A.l term too
        HIP_TRY(launch_box_rhs_lu(x->P, x->dual.args, x->dual.d_lsh, x->dual.b_user, x->b, x->stream));
    else
        HIP_TRY(launch_box_rhs(x->P, x->dual.args, x->dual.b_user, x->b, x->stream));
    return SPX_OK;
}

void box_unshift_xb(const spx_ctx* x, double* x_b, const int64_t* b_ixs) {
    const std::vector<double>& lb = x->dual.lb;
    if (lb.empty()) return;
    for (size_t i = 0; i < (size_t)x->m; ++i) {
        const double l = lb[(size_t)b_ixs[i]];
        if (std::isfinite(l)) x_b[i] += l;
    }
}

int box_buffers(spx_ctx* x) {
    DualState& d = x->dual;
    if (d.args.ub) return SPX_OK;
    const size_t n = (size_t)x->n, L = (size_t)x->L;
    double* d_ub = nullptr;
    SPX_TRY(x->alloc(&d_ub, n));
    d.args.ub = d_ub;
    SPX_TRY(x->alloc(&d.args.ub_B, L));
    SPX_TRY(x->alloc(&d.args.at_upper, n));
    SPX_TRY(x->alloc(&d.b_user, L));
    const std::vector<double> inf(std::max(n, L), INFINITY);
    HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipMemcpy(d_ub, inf.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.args.ub_B, inf.data(), L * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.b_user, x->b, L * sizeof(double), hipMemcpyDeviceToDevice));
    return SPX_OK;
}

int box_replace_xb(spx_ctx* x) {
    DualState& d = x->dual;
    if (d.boxed) {
        const size_t n = (size_t)x->n;
        std::vector<int8_t> up(n);
        bool changed = false;
        HIP_TRY(hipStreamSynchronize(x->stream));
        HIP_TRY(hipMemcpy(up.data(), d.args.at_upper, n, hipMemcpyDeviceToHost));
        for (size_t j = 0; j < n; ++j)
            if (up[j] && !std::isfinite(d.ub[j])) {
                up[j] = 0;
                changed = true;
            }
        if (changed) HIP_TRY(hipMemcpy(d.args.at_upper, up.data(), n, hipMemcpyHostToDevice));
    }
    SPX_TRY(box_sync(x));
    HIP_TRY(launch_box_xb(x->P, d.cfg, x->stream));
    return SPX_OK;
}

// k dual passes, eager launches, one host synchronisation at the end.  Every
// kernel returns at once when the device status is not running or the limit is
// reached; the closing k_dual_step only commits the last pass's pivot.
// (Replaying the passes from a captured hipGraph was measured at C3's shape:
// 7,675 against 7,641 it/s, so the passes stay eager)
int iterate_dual(spx_ctx* x, int64_t k) {
    SPX_TRY(dual_setup(x));
    if (!x->dual.checked) SPX_TRY(dual_check_feasible(x));
    const bool se = x->dual.rule == SPX_DUAL_PRICING_STEEPEST;
    if (se) SPX_TRY(dual_refresh_weights(x));
    else weights_lost(x);  // Dantzig passes keep no weights
    if (long_step(x)) SPX_TRY(long_setup(x));
    SPX_TRY(set_limit(x, x->pivots + k));
    for (int64_t i = 0; i < k; ++i) {
        hipEvent_t p0 = nullptr, p1 = nullptr, u0 = nullptr, u1 = nullptr;
        if (x->timing) SPX_TRY(pass_events(x, &p0, &p1, &u0, &u1));
        SPX_TRY(enqueue_dual_pass(x, p0, p1, u0, u1));
        ++x->n_eager;
    }
    // (steepest edge: the last pivot's weights too)
    SPX_TRY(enqueue_dual_finish(x));
    return read_state(x);
}

int dual_on_reset(spx_ctx* x) {
    DualState& d = x->dual;
    if (d.boxed) {  // every column back at its lower bound: b_eff = b
        HIP_TRY(hipMemsetAsync(d.args.at_upper, 0, (size_t)x->n, x->stream));
        if (d.shifted) SPX_TRY(box_sync(x));  // b_eff = b - A.l (launch_reset reads it; ub_B follows in do_reset)
        else HIP_TRY(hipMemcpyAsync(x->b, d.b_user, (size_t)x->L * sizeof(double), hipMemcpyDeviceToDevice, x->stream));
    }
    if (d.args.rec) HIP_TRY(hipMemsetAsync(d.args.rec, 0, sizeof(DualRec), x->stream));
    if (d.args.lrec) HIP_TRY(hipMemsetAsync(d.args.lrec, 0, sizeof(DualLongRec), x->stream));  // the flip counters too
    feasibility_unknown(x);
    weights_lost(x);
    return SPX_OK;
}

void dual_on_reinvert(spx_ctx* x) { weights_lost(x); }

void dual_on_new_basis(spx_ctx* x) {
    feasibility_unknown(x);
    pbox_on_change(x);
}

// (rows m..L-1 stay 0; boxed: the caller's b, reinvert_basis forms b_eff from it)
double* dual_rhs_target(spx_ctx* x) { return x->dual.boxed ? x->dual.b_user : x->b; }

int dual_switch_algorithm(spx_ctx* x, int32_t algo) {
    if (algo == SPX_ALGO_PRIMAL && x->dual.boxed)
        return fail(SPX_ERR_STATE, "the primal loop does not run with finite upper bounds (spx_set_bounds): bounded "
                    "variables are the dual simplex loop's and the bounded primal loop's (SPX_ALGO_PRIMAL_BOX); remove "
                    "the bounds first");
    if (algo == SPX_ALGO_DUAL && x->dual.nfree > 0)
        return fail(SPX_ERR_STATE, "the dual simplex loop does not run free columns (%lld of them, spx_set_bounds_lu): a "
                    "non-basic free column has no dual feasible side unless d_j = 0; SPX_ALGO_PRIMAL_BOX runs them",
                    (long long)x->dual.nfree);
    // the bounded primal loop's phase 1 does not maintain y: whichever loop takes the
    // basis gets y = c_B B^-1 (the primal loop would go on updating a stale y)
    SPX_TRY(pbox_fresh_y(x));
    if (algo == SPX_ALGO_DUAL || algo == SPX_ALGO_PRIMAL_BOX) {
        if (const char* why = dual_conflict(x->opts, x->P.win))
            return fail(SPX_ERR_STATE, "the %s does not run %s",
                        algo == SPX_ALGO_DUAL ? "dual simplex loop" : "bounded primal simplex loop", why);
        if (algo == SPX_ALGO_PRIMAL_BOX && (!(x->opts.piv_tol >= 0.0) || !(x->opts.feas_tol >= 0.0)))
            return fail(SPX_ERR_STATE, "piv_tol and feas_tol must be >= 0");
        SPX_TRY(dual_setup(x));
        if (algo == SPX_ALGO_PRIMAL_BOX) SPX_TRY(pbox_setup(x));
        // the primal loop's pending y / x_b updates applied; its pending rank-1
        // update of B^-1 is the form the dual kernels continue from
        SPX_TRY(flush(x));
    } else {
        // the dual loop leaves y and x_b current and B^-1 in the primal loop's
        // pending form; the next pricing pass runs at a new iteration count
        SPX_TRY(clear_tickets(x));
    }
    feasibility_unknown(x);
    weights_lost(x);  // (primal passes keep no dual weights)
    pbox_on_change(x);
    pbox_weights_lost(x);
    return SPX_OK;
}

int dual_objective_offset(spx_ctx* x, double* zu) {
    *zu = 0.0;
    if (!x->dual.boxed) return SPX_OK;
    const size_t n = (size_t)x->n;
    std::vector<double> c(n);
    std::vector<int8_t> up;
    HIP_TRY(hipMemcpy(c.data(), x->c, n * sizeof(double), hipMemcpyDeviceToHost));
    SPX_TRY(fetch_placements(x, up));
    for (size_t j = 0; j < n; ++j)  // ascending j
        if (up[j]) *zu += c[j] * x->dual.ub[j];
    if (!x->dual.lb.empty()) {  // shifted variables: + sum_j c_j l_j, ascending j, its own sum
        double zl = 0.0;
        for (size_t j = 0; j < n; ++j)
            if (std::isfinite(x->dual.lb[j])) zl += c[j] * x->dual.lb[j];
        *zu += zl;
    }
    return SPX_OK;
}

}  // namespace spx_host

using namespace spx_host;

extern "C" {

int spx_set_dual_pricing(spx_ctx* x, int32_t rule) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    if (rule != SPX_DUAL_PRICING_DANTZIG && rule != SPX_DUAL_PRICING_STEEPEST)
        return fail(SPX_ERR_ARG, "bad dual pricing rule %d", rule);
    if (rule != x->dual.rule) weights_lost(x);
    x->dual.rule = rule;
    return SPX_OK;
}

int spx_set_dual_ratio(spx_ctx* x, int32_t rule) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    if (rule != SPX_DUAL_RATIO_TEXTBOOK && rule != SPX_DUAL_RATIO_LONG_STEP)
        return fail(SPX_ERR_ARG, "bad dual ratio test %d", rule);
    x->dual.ratio = rule;  // (x_b, b_eff and at_upper are consistent between calls under either rule)
    return SPX_OK;
}

int spx_get_dual_flips(spx_ctx* x, int64_t out[3]) {
    if (!x || !out) return fail(SPX_ERR_ARG, "NULL argument");
    out[0] = out[1] = out[2] = 0;
    if (!x->dual.args.lrec) return SPX_OK;  // no long-step pass yet
    DualLongRec r;
    HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipMemcpy(&r, x->dual.args.lrec, sizeof r, hipMemcpyDeviceToHost));
    out[0] = r.flips;
    out[1] = r.passes;
    out[2] = r.max_pass;
    return SPX_OK;
}

int spx_get_dual_weights(spx_ctx* x, double* w) {
    if (!x || !w) return fail(SPX_ERR_ARG, "NULL argument");
    if (x->dual.rule != SPX_DUAL_PRICING_STEEPEST)
        return fail(SPX_ERR_STATE, "no dual pricing weights: the dual leaving-row rule is Dantzig");
    if (x->algo != SPX_ALGO_DUAL)
        return fail(SPX_ERR_STATE, "no dual pricing weights: the context runs the primal loop");
    if (x->broken) return fail(SPX_ERR_STATE, "no valid basis (a failed spx_set_basis): call spx_reset");
    SPX_TRY(dual_setup(x));
    SPX_TRY(dual_refresh_weights(x));
    HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipMemcpy(w, x->dual.args.w, sizeof(double) * (size_t)x->m, hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spx_set_bounds(spx_ctx* x, const double* ub) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    const size_t n = (size_t)x->n;
    bool finite = false;
    for (size_t j = 0; ub && j < n; ++j) {
        if (std::isnan(ub[j])) return fail(SPX_ERR_ARG, "upper bound of column %lld is NaN", (long long)j);
        if (ub[j] < 0.0)
            return fail(SPX_ERR_ARG, "upper bound %g of column %lld is negative (lower bounds are 0)", ub[j], (long long)j);
        finite = finite || std::isfinite(ub[j]);
    }
    if (x->opts.nranks > 1 || x->P.row_shard)
        return fail(SPX_ERR_STATE, "spx_set_bounds needs one rank and replicated B^-1 (nranks %d%s)", x->opts.nranks,
                    x->P.row_shard ? ", row-sharded" : "");
    const bool pbox = x->algo == SPX_ALGO_PRIMAL_BOX;  // placements kept, no normalisation: its entry check follows
    if (x->algo != SPX_ALGO_DUAL && !pbox)
        return fail(SPX_ERR_STATE, "upper bounds need the dual simplex loop (SPX_ALGO_DUAL) or the bounded primal loop "
                    "(SPX_ALGO_PRIMAL_BOX): the primal loop does not run bounded variables");
    if (x->broken) return fail(SPX_ERR_STATE, "no valid basis (a failed spx_set_basis): call spx_reset");
    if (x->stepped_price) return fail(SPX_ERR_STATE, "spx_set_bounds between spx_price and spx_pivot");
    SPX_TRY(dual_setup(x));
    DualState& d = x->dual;
    pbox_on_change(x);
    if (!pbox) {  // refused before anything changes: a column that would have no dual feasible side
        std::vector<double> e;
        std::vector<int32_t> pos;
        SPX_TRY(fetch_reduced_costs(x, e, pos));
        for (size_t j = 0; j < n; ++j)
            if (pos[j] >= 0 && e[j] < -x->opts.eps && !(ub && std::isfinite(ub[j]))) return no_feasible_side(x, e[j], j);
    }
    // lower bounds are 0 from here on: a context that had others (spx_set_bounds_lu) is boxed, so b_eff is
    // formed again below from b_user without the A.l term
    d.lb.clear();
    d.ub_user.clear();
    d.shifted = false;
    d.nfree = 0;
    if (!finite && !d.boxed) {  // nothing to keep: today's kernels, today's state
        d.ub.assign(n, INFINITY);
        return set_running(x);
    }
    SPX_TRY(box_buffers(x));
    HIP_TRY(hipStreamSynchronize(x->stream));
    if (!d.boxed) {  // P.b is still the caller's b, every column at lower
        HIP_TRY(hipMemcpy(d.b_user, x->b, (size_t)x->L * sizeof(double), hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemset(d.args.at_upper, 0, n));
    }
    d.ub.assign(n, INFINITY);
    if (ub) d.ub.assign(ub, ub + n);
    HIP_TRY(hipMemcpy(const_cast<double*>(d.args.ub), d.ub.data(), n * sizeof(double), hipMemcpyHostToDevice));
    // a column at an upper bound that no longer exists goes to lower
    std::vector<int8_t> up(n);
    HIP_TRY(hipMemcpy(up.data(), d.args.at_upper, n, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < n; ++j)
        if (up[j] && !std::isfinite(d.ub[j])) up[j] = 0;
    HIP_TRY(hipMemcpy(d.args.at_upper, up.data(), n, hipMemcpyHostToDevice));
    d.boxed = true;  // (the normalisation and b_eff below run on the boxed state either way)
    feasibility_unknown(x);
    SPX_TRY(set_running(x));
    const int rc = pbox ? box_recompute_xb(x) : box_normalise(x, true);
    if (!finite && rc == SPX_OK) {  // no bound left: P.b is b again (no column at upper), the plain kernels run
        HIP_TRY(hipStreamSynchronize(x->stream));
        d.boxed = false;
    }
    return rc;
}

int spx_get_bounds(spx_ctx* x, double* ub) {
    if (!x || !ub) return fail(SPX_ERR_ARG, "NULL argument");
    const std::vector<double>& u = x->dual.lb.empty() ? x->dual.ub : x->dual.ub_user;  // the caller's, not the range
    for (size_t j = 0; j < (size_t)x->n; ++j) ub[j] = u.empty() ? INFINITY : u[j];
    return SPX_OK;
}

int spx_get_bounds_lu(spx_ctx* x, double* lb, double* ub) {
    if (!x || !lb || !ub) return fail(SPX_ERR_ARG, "NULL argument");
    for (size_t j = 0; j < (size_t)x->n; ++j) lb[j] = x->dual.lb.empty() ? 0.0 : x->dual.lb[j];
    return spx_get_bounds(x, ub);
}

int spx_set_bounds_lu(spx_ctx* x, const double* lb, const double* ub) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    const size_t n = (size_t)x->n;
    bool general = false;
    int64_t nfree = 0;
    for (size_t j = 0; j < n; ++j) {
        const double l = lb ? lb[j] : 0.0, u = ub ? ub[j] : INFINITY;
        if (std::isnan(l) || std::isnan(u)) return fail(SPX_ERR_ARG, "a bound of column %lld is NaN", (long long)j);
        if (l == INFINITY) return fail(SPX_ERR_ARG, "lower bound of column %lld is +inf", (long long)j);
        if (l > u || u == -INFINITY)
            return fail(SPX_ERR_ARG, "lower bound %g of column %lld is above its upper bound %g", l, (long long)j, u);
        if (l == -INFINITY && std::isfinite(u))
            return fail(SPX_ERR_ARG, "column %lld has an upper bound %g and no lower bound: upper-only columns are not "
                        "supported (substitute x = -x', or give a finite lower bound)", (long long)j, u);
        general = general || l != 0.0;
        nfree += l == -INFINITY;
    }
    if (!general) return spx_set_bounds(x, ub);  // lower bounds 0: the same call, the same kernels, the same bits
    if (x->opts.nranks > 1 || x->P.row_shard)
        return fail(SPX_ERR_STATE, "spx_set_bounds_lu needs one rank and replicated B^-1 (nranks %d%s)", x->opts.nranks,
                    x->P.row_shard ? ", row-sharded" : "");
    const bool pbox = x->algo == SPX_ALGO_PRIMAL_BOX;
    if (x->algo != SPX_ALGO_DUAL && !pbox)
        return fail(SPX_ERR_STATE, "bounds need the dual simplex loop (SPX_ALGO_DUAL) or the bounded primal loop "
                    "(SPX_ALGO_PRIMAL_BOX): the primal loop does not run bounded variables");
    if (x->broken) return fail(SPX_ERR_STATE, "no valid basis (a failed spx_set_basis): call spx_reset");
    if (x->stepped_price) return fail(SPX_ERR_STATE, "spx_set_bounds_lu between spx_price and spx_pivot");
    if (nfree > 0 && !pbox)
        return fail(SPX_ERR_STATE, "the dual simplex loop does not run free columns (%lld of them): a non-basic free "
                    "column has no dual feasible side unless d_j = 0; SPX_ALGO_PRIMAL_BOX runs them", (long long)nfree);
    if (nfree > 0 && x->pbox.rule == SPX_PRIMAL_PRICING_STEEPEST && x->pbox.frrule != SPX_PRIMAL_PRICING_STEEPEST)
        return fail(SPX_ERR_STATE, "free columns (%lld of them) do not run with steepest-edge pricing "
                    "(spx_set_primal_pricing); set SPX_PRIMAL_PRICING_DANTZIG first", (long long)nfree);
    SPX_TRY(dual_setup(x));
    DualState& d = x->dual;
    std::vector<double> range(n), lsh(n);
    bool shifted = false;
    for (size_t j = 0; j < n; ++j) {
        const double l = lb[j], u = ub ? ub[j] : INFINITY;  // (general: lb is not NULL)
        lsh[j] = std::isfinite(l) ? l : 0.0;
        range[j] = std::isfinite(u) ? u - lsh[j] : INFINITY;
        shifted = shifted || lsh[j] != 0.0;
    }
    if (!pbox) {  // refused before anything changes: a column that would have no dual feasible side
        std::vector<double> e;
        std::vector<int32_t> pos;
        SPX_TRY(fetch_reduced_costs(x, e, pos));
        for (size_t j = 0; j < n; ++j)
            if (pos[j] >= 0 && e[j] < -x->opts.eps && !std::isfinite(range[j])) return no_feasible_side(x, e[j], j);
    }
    pbox_on_change(x);
    SPX_TRY(box_buffers(x));
    if (!d.d_lsh) SPX_TRY(x->alloc(&d.d_lsh, n));
    HIP_TRY(hipStreamSynchronize(x->stream));
    if (!d.boxed) {  // P.b is still the caller's b, every column at lower
        HIP_TRY(hipMemcpy(d.b_user, x->b, (size_t)x->L * sizeof(double), hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemset(d.args.at_upper, 0, n));
    }
    d.lb.assign(lb, lb + n);
    d.ub_user.assign(n, INFINITY);
    if (ub) d.ub_user.assign(ub, ub + n);
    d.ub = range;
    d.shifted = shifted;
    d.nfree = nfree;
    HIP_TRY(hipMemcpy(const_cast<double*>(d.args.ub), d.ub.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.d_lsh, lsh.data(), n * sizeof(double), hipMemcpyHostToDevice));
    // a column at an upper bound that no longer exists goes to lower
    std::vector<int8_t> up(n);
    HIP_TRY(hipMemcpy(up.data(), d.args.at_upper, n, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < n; ++j)
        if (up[j] && !std::isfinite(d.ub[j])) up[j] = 0;
    HIP_TRY(hipMemcpy(d.args.at_upper, up.data(), n, hipMemcpyHostToDevice));
    d.boxed = true;  // the boxed kernels and b_user / b_eff, whatever the ranges are
    feasibility_unknown(x);
    SPX_TRY(set_running(x));
    return pbox ? box_recompute_xb(x) : box_normalise(x, true);
}

int spx_get_primal(spx_ctx* x, double* xv, int8_t* at_upper) {
    if (!x || !xv) return fail(SPX_ERR_ARG, "NULL argument");
    const size_t n = (size_t)x->n, m = (size_t)x->m;
    std::vector<double> xb(m);
    std::vector<int64_t> bix(m);
    SPX_TRY(spx_get_state(x, xb.data(), bix.data(), nullptr, nullptr, nullptr, nullptr, nullptr));
    std::vector<int8_t> up;
    SPX_TRY(fetch_placements(x, up));
    if (x->dual.lb.empty()) {
        for (size_t j = 0; j < n; ++j) xv[j] = up[j] ? x->dual.ub[j] : 0.0;
    } else {  // exactly the caller's bound (not l + (u - l)); a free column sits at 0; x_b came back unshifted
        const DualState& d = x->dual;
        for (size_t j = 0; j < n; ++j) xv[j] = up[j] ? d.ub_user[j] : (std::isfinite(d.lb[j]) ? d.lb[j] : 0.0);
    }
    for (size_t i = 0; i < m; ++i) xv[(size_t)bix[i]] = xb[i];
    if (at_upper) std::memcpy(at_upper, up.data(), n);
    return SPX_OK;
}

}  // extern "C"
