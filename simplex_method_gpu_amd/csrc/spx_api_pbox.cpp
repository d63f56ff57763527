// spx_api_pbox.cpp — the bounded primal simplex loop's host side (kernels:
// spx_pbox.h): its state (PboxState, spx_ctx.h, with the invariants), the entry
// check, the pass loop, the hooks through which the rest of the runtime touches
// any of it, and the entry point that is this loop's alone.  The bounds and
// placements are the dual loop's state, reached through spx_api_dual.cpp's hooks.
#include <cmath>
#include <cstdlib>

#include "spx_ctx.h"

using namespace spx;

namespace spx_host {

namespace {

// Entry check, before the first pass after anything set the basis, the bounds,
// b, c or the algorithm from outside: placements kept (a column at an upper
// bound that no longer exists goes to lower), x_b recomputed from them, and
// -feas_tol <= x_b[i] <= ub_B[i] + feas_tol on the host.  No normalisation by
// reduced-cost sign: that is the dual loop's.  With phase 1 on
// nothing is refused: k_pbox_classify writes w, ninf and ninf0, and the passes
// are the four-step ones while rows are out of their bounds.
int read_phase(spx_ctx* x) {
    PboxPhase ph;
    HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipMemcpy(&ph, x->pbox.p1.ph, sizeof ph, hipMemcpyDeviceToHost));
    x->pbox.ninf = ph.ninf;
    x->pbox.y_stale = ph.y_stale;
    if (!ph.y_stale && ph.ninf == 0) x->pbox.y_dirty = false;
    return SPX_OK;
}

// free columns: the two arrays on first use, then is_free from the
// bounds and lb_B from the basis (k_pbox_step_f keeps lb_B from there on)
int pbox_free_sync(spx_ctx* x) {
    PboxState& s = x->pbox;
    const size_t n = (size_t)x->n, m = (size_t)x->m, L = (size_t)x->L;
    if (!s.fr.lb_B) {
        SPX_TRY(x->alloc(&s.fr_flags, n));
        s.fr.is_free = s.fr_flags;
        SPX_TRY(x->alloc(&s.fr.lb_B, L));
        HIP_TRY(pbox_free_prepare(x->P, s.cfg));
    }
    const std::vector<double>& lb = x->dual.lb;
    std::vector<int8_t> fr(n);
    for (size_t j = 0; j < n; ++j) fr[j] = lb[j] == -INFINITY ? 1 : 0;
    std::vector<int64_t> bix(m);
    std::vector<double> lbB(L, 0.0);
    HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipMemcpy(bix.data(), x->P.b_ixs, m * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < m; ++i) lbB[i] = fr[(size_t)bix[i]] ? -INFINITY : 0.0;
    HIP_TRY(hipMemcpy(s.fr_flags, fr.data(), n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s.fr.lb_B, lbB.data(), L * sizeof(double), hipMemcpyHostToDevice));
    return SPX_OK;
}

int pbox_check_entry(spx_ctx* x) {
    const size_t m = (size_t)x->m;
    const bool fr = x->dual.nfree > 0;
    SPX_TRY(pbox_fresh_y(x));  // (a phase 1 that was switched off mid-way: the plain passes need y)
    SPX_TRY(box_replace_xb(x));
    if (fr) SPX_TRY(pbox_free_sync(x));
    if (x->pbox.phase1) {
        // phase 1: a row out of its bounds is not an error; the device classifies and the passes start there
        if (fr) HIP_TRY(launch_pbox_classify_f(x->P, x->pbox.args, x->pbox.p1, x->pbox.fr, true, x->stream));
        else HIP_TRY(launch_pbox_classify(x->P, x->pbox.args, x->pbox.p1, true, x->stream));
        HIP_TRY(launch_pbox_stage(x->P, x->stream));
        SPX_TRY(read_phase(x));
        x->pbox.checked = true;
        return SPX_OK;
    }
    std::vector<double> xb(m), ubB(m);
    std::vector<int64_t> bix(m);
    HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipMemcpy(xb.data(), x->P.x_b, m * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ubB.data(), x->pbox.args.ub_B, m * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(bix.data(), x->P.b_ixs, m * sizeof(int64_t), hipMemcpyDeviceToHost));
    const double tol = x->opts.feas_tol;
    if (fr) {  // the *_f kernels read the phase from the device: phase 2 (the rows below pass, or nothing runs)
        HIP_TRY(hipMemsetAsync(&x->pbox.p1.ph->ninf, 0, sizeof(int32_t), x->stream));
        x->pbox.ninf = 0;
    }
    for (size_t i = 0; i < m; ++i) {
        if (fr && x->dual.lb[(size_t)bix[i]] == -INFINITY) continue;  // a free basic column is within its bounds
        if (xb[i] >= -tol && xb[i] <= ubB[i] + tol) continue;
        return fail(SPX_ERR_STATE, "basis is not primal feasible (x_b %g in row %lld, basic column %lld with bounds "
                    "[0, %g], feas_tol %g): the bounded primal loop has no phase 1; SPX_ALGO_DUAL repairs it",
                    xb[i], (long long)i, (long long)bix[i], ubB[i], tol);
    }
    // a loop that ended elsewhere leaves its pending pivot's row unstaged
    HIP_TRY(launch_pbox_stage(x->P, x->stream));
    x->pbox.checked = true;
    return SPX_OK;
}

}  // namespace

int pbox_setup(spx_ctx* x) {
    PboxState& s = x->pbox;
    if (s.args.rec) return SPX_OK;
    SPX_TRY(dual_setup(x));  // (k_box_xb's geometry; a switch to the dual loop finds its buffers)
    SPX_TRY(box_buffers(x));
    // SPX_PBOX_LDS_CAP (tests): fewer bytes of LDS than the built-in cap (also pbox_se_prepare's below)
    HIP_TRY(pbox_prepare(x->P, x->cus, x->opts.price_grid, (x->opts.flags & SPX_FLAG_GLOBAL_Y) != 0,
                         env_bytes("SPX_PBOX_LDS_CAP"), &s.cfg));
    SPX_TRY(x->alloc(&s.args.parts, (size_t)s.cfg.price_grid));
    SPX_TRY(x->alloc(&s.args.rparts, (size_t)s.cfg.update_grid));
    s.args.ub = x->dual.args.ub;
    s.args.ub_B = x->dual.args.ub_B;
    s.args.at_upper = x->dual.args.at_upper;
    s.args.b_eff = x->b;
    s.args.price_grid = s.cfg.price_grid;
    s.args.update_grid = s.cfg.update_grid;
    s.args.piv_tol = x->opts.piv_tol;
    s.p1.vtb_blocks = s.cfg.vtb_blocks;
    s.p1.force = 0;
    s.p1.feas_tol = x->opts.feas_tol;
    SPX_TRY(x->alloc(&s.p1.w, (size_t)x->L));
    SPX_TRY(x->alloc(&s.p1.yp, (size_t)x->L));
    SPX_TRY(x->alloc(&s.p1.vparts, (size_t)s.cfg.vtb_blocks * (size_t)x->L));
    SPX_TRY(x->alloc(&s.p1.ph, 1));
    SPX_TRY(x->alloc(&s.args.rec, 1));
    return SPX_OK;
}

namespace {

// the steepest-edge buffers and geometry, on first use (after pbox_setup)
int pbox_se_setup(spx_ctx* x) {
    PboxState& s = x->pbox;
    if (s.se.se) return SPX_OK;
    // experiment (SPX_PBOX_SE_LDS): vectors of k_pbox_price_se staged in LDS -- 0, 1 or 3
    const char* ev = std::getenv("SPX_PBOX_SE_LDS");
    HIP_TRY(pbox_se_prepare(x->P, x->cus, s.cfg.price_grid, (x->opts.flags & SPX_FLAG_GLOBAL_Y) != 0,
                            ev ? std::atoi(ev) : -1, env_bytes("SPX_PBOX_LDS_CAP"), &s.secfg));
    s.se.vtb_blocks = s.cfg.vtb_blocks;
    s.se.apply = 0;
    SPX_TRY(x->alloc(&s.se.gamma, (size_t)x->n));
    SPX_TRY(x->alloc(&s.se.rho, (size_t)x->L));
    SPX_TRY(x->alloc(&s.se.tau, (size_t)x->L));
    SPX_TRY(x->alloc(&s.se.tparts, (size_t)s.cfg.vtb_blocks * (size_t)x->L));
    SPX_TRY(x->alloc(&s.se.se, 1));
    s.se_stale = true;
    return SPX_OK;
}

// the exact-weight buffers and geometry, on first use (after pbox_se_setup)
int pbox_wexact_setup(spx_ctx* x) {
    PboxState& s = x->pbox;
    if (s.wx.parts) return SPX_OK;
    s.wxcfg = pbox_wexact_geometry(x->m, x->n, x->L);
    HIP_TRY(pbox_wexact_prepare());
    SPX_TRY(pbox_binv_copy(x));
    SPX_TRY(x->alloc(&s.wx.sparts, s.wxcfg.sparts));
    SPX_TRY(x->alloc(&s.wx.parts, s.wxcfg.parts));
    s.wx.S = s.wx_S;
    s.wx.gamma = s.se.gamma;
    s.wx.cap = s.wxcfg.cap;
    s.wx.row_blocks = s.wxcfg.row_blocks;
    return SPX_OK;
}

// gamma_j = 1 + ||B^-1 A_j||^2 for the non-basic columns of the current basis:
// B^-1 brought current into wx_S (the pending pivot applied, as spx_get_state
// does; the loop's own S and its pending record are left alone), then the
// product, the slack norms and the sum
int pbox_wexact_run(spx_ctx* x) {
    PboxState& s = x->pbox;
    SPX_TRY(pbox_wexact_setup(x));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (x->timing) {
        while (s.ev_wx.size() < 2 * (s.n_wx + 1)) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            s.ev_wx.push_back(e);
        }
        e0 = s.ev_wx[2 * s.n_wx];
        e1 = s.ev_wx[2 * s.n_wx + 1];
        ++s.n_wx;
        HIP_TRY(hipEventRecord(e0, x->stream));
    }
    HIP_TRY(launch_materialize(x->P, s.wx_S, x->stream));
    HIP_TRY(launch_pbox_wexact(x->P, s.wx, s.wxcfg, x->stream));
    if (e1) HIP_TRY(hipEventRecord(e1, x->stream));
    return SPX_OK;
}

// weights nobody kept, and nothing pending: gamma_j = 1 + ||A_j||^2 (exact at
// the slack basis, a reference framework elsewhere), or under
// SPX_PRIMAL_WEIGHTS_EXACT for a warm basis the exact norms
int pbox_se_restart(spx_ctx* x) {
    PboxState& s = x->pbox;
    if (!s.se_stale) return SPX_OK;
    HIP_TRY(hipMemsetAsync(s.se.se, 0, sizeof(PboxSeRec), x->stream));
    const bool slack_basis = !s.warm && x->pivots == 0;
    if (s.winit == SPX_PRIMAL_WEIGHTS_EXACT && !slack_basis) SPX_TRY(pbox_wexact_run(x));
    else HIP_TRY(launch_pbox_se_init(x->P, s.se, s.secfg, x->stream));
    s.se_stale = false;
    return SPX_OK;
}

// the long-step ratio test's counters and list capacity, on first use (after pbox_setup)
int pbox_long_setup(spx_ctx* x) {
    PboxState& s = x->pbox;
    if (s.lg.lrec) return SPX_OK;
    // SPX_PBOX_LONG_CAP (tests): fewer soft breakpoints in LDS than PBOX_LONG_CAP, so small shapes walk by rounds
    const size_t cap = env_bytes("SPX_PBOX_LONG_CAP");
    s.lg.cap = cap > 0 && cap < (size_t)PBOX_LONG_CAP ? (int32_t)cap : PBOX_LONG_CAP;
    SPX_TRY(x->alloc(&s.lg.lrec, 1));
    return SPX_OK;
}

// timing: the next event pair around the vtb / tau step
int vtb_events(spx_ctx* x, hipEvent_t* v0, hipEvent_t* v1) {
    PboxState& s = x->pbox;
    while (s.ev_vtb.size() < 2 * (s.n_vtb + 1)) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        s.ev_vtb.push_back(e);
    }
    *v0 = s.ev_vtb[2 * s.n_vtb];
    *v1 = s.ev_vtb[2 * s.n_vtb + 1];
    ++s.n_vtb;
    return SPX_OK;
}

}  // namespace

// k pivots or a terminal status.  A pass is three eager launches and makes a
// pivot or a flip; the host enqueues as many passes as pivots are missing,
// synchronises once, and goes round again for the flips' share.  Every kernel
// returns at once when the device status is not running or the limit is reached.
// Phase 1: while the host last saw ninf > 0 or y stale a pass is the four-step
// one (k_pbox_vtb first, then the kernels that read the phase from the device),
// which runs on through the switch inside a round; the readback that shows
// ninf == 0 and y current brings the three-launch pass back.
// Steepest edge: a pass is price_se -> update -> step_se -> tau,
// after the weights were restarted where nobody kept them; the pending weight
// update lives on the device with its own operands, so nothing here tracks it.
// Steepest edge through phase 1 (opt-in): while the host last saw
// ninf > 0 or y stale the pass is vtb -> price_se1 -> update1 -> step_se1 -> tau;
// the same readback brings §7h's four-step pass back, with the weights it finds.
// Steepest edge with free columns (opt-in): every pass is [vtb ->]
// price_se_f -> update_f -> step_se_f -> tau, vtb under the same host condition.
// Phase 1's long-step ratio test (opt-in): a pass that k_pbox_vtb
// opens gets k_pbox_long1 between its update and its step kernel, in all four
// phase-1 capable shapes; it rewrites the ratio partials and nothing else.
int iterate_pbox(spx_ctx* x, int64_t k) {
    SPX_TRY(pbox_setup(x));
    if (!x->pbox.checked) SPX_TRY(pbox_check_entry(x));
    PboxState& s = x->pbox;
    const bool steep = s.rule == SPX_PRIMAL_PRICING_STEEPEST;
    const bool fr = x->dual.nfree > 0;  // free columns: every pass on the *_f kernels
    if (fr && steep && s.frrule != SPX_PRIMAL_PRICING_STEEPEST)  // (both setters refuse the combination)
        return fail(SPX_ERR_STATE, "free columns do not run with steepest-edge pricing");
    PboxArgs se_args = s.args;
    if (steep) {
        if (s.phase1 && s.p1rule != SPX_PRIMAL_PRICING_STEEPEST)  // (create and the setters refuse the state)
            return fail(SPX_ERR_STATE, "steepest-edge pricing does not run with the bounded primal loop's phase 1");
        SPX_TRY(pbox_se_setup(x));
        if (s.phase1 && !s.se1_ready) {
            HIP_TRY(pbox_se1_prepare(x->P, s.secfg));
            s.se1_ready = true;
        }
        if (fr && !s.sef_ready) {
            HIP_TRY(pbox_se_f_prepare(x->P, s.secfg));
            s.sef_ready = true;
        }
        SPX_TRY(pbox_se_restart(x));
        se_args.price_grid = s.secfg.price_grid;  // k_pbox_update / k_pbox_update1 merges this pass's partials
    } else {
        s.se_stale = true;  // a Dantzig pass keeps no weights
    }
    // phase 1's long-step ratio test: k_pbox_long1 between the update and the step kernel of every
    // pass that k_pbox_vtb opens
    const bool lng = s.phase1 && s.p1ratio == SPX_PRIMAL_RATIO_LONG_STEP;
    if (lng) SPX_TRY(pbox_long_setup(x));
    const int64_t target = x->pivots + k;
    SPX_TRY(set_limit(x, target));
    while (x->status == SPX_STATUS_MAX_ITER && x->pivots < target) {
        const int64_t round = target - x->pivots;
        for (int64_t i = 0; i < round; ++i) {
            const bool p1pass = s.phase1 && (s.ninf > 0 || s.y_stale);
            hipEvent_t p0 = nullptr, p1 = nullptr, u0 = nullptr, u1 = nullptr;
            if (x->timing) SPX_TRY(pass_events(x, &p0, &p1, &u0, &u1));
            if (steep && fr) {
                // [vtb ->] price_se_f -> update_f -> step_se_f -> tau: the phase is the device's
                hipEvent_t v0 = nullptr, v1 = nullptr, t0 = nullptr, t1 = nullptr;
                if (s.phase1 && (s.ninf > 0 || s.y_stale)) {
                    s.y_dirty = true;
                    if (x->timing) SPX_TRY(vtb_events(x, &v0, &v1));
                    HIP_TRY(launch_pbox_vtb(x->P, s.p1, s.cfg, x->stream, v0, v1));
                }
                if (x->timing) SPX_TRY(vtb_events(x, &t0, &t1));
                HIP_TRY(launch_pbox_price_se_f(x->P, se_args, s.p1, s.se, s.fr, s.secfg, x->stream, p0, p1));
                if (p0) HIP_TRY(hipEventRecord(x->ev_xend[x->n_price - 1], x->stream));
                HIP_TRY(launch_pbox_update_f(x->P, se_args, s.p1, s.fr, s.cfg, x->stream, u0, u1));
                if (lng && p1pass) HIP_TRY(launch_pbox_long1(x->P, se_args, s.p1, &s.fr, s.lg, x->stream));
                HIP_TRY(launch_pbox_step_se_f(x->P, se_args, s.p1, s.se, s.fr, x->stream));
                HIP_TRY(launch_pbox_tau(x->P, s.se, s.cfg, x->stream, t0, t1));
                ++x->n_eager;
                continue;
            }
            if (steep && s.phase1 && (s.ninf > 0 || s.y_stale)) {
                // vtb -> price_se1 -> update1 -> step_se1 -> tau: the phase is the device's
                s.y_dirty = true;
                hipEvent_t v0 = nullptr, v1 = nullptr, t0 = nullptr, t1 = nullptr;
                if (x->timing) {
                    SPX_TRY(vtb_events(x, &v0, &v1));
                    SPX_TRY(vtb_events(x, &t0, &t1));
                }
                HIP_TRY(launch_pbox_vtb(x->P, s.p1, s.cfg, x->stream, v0, v1));
                HIP_TRY(launch_pbox_price_se1(x->P, se_args, s.p1, s.se, s.secfg, x->stream, p0, p1));
                if (p0) HIP_TRY(hipEventRecord(x->ev_xend[x->n_price - 1], x->stream));
                HIP_TRY(launch_pbox_update1(x->P, se_args, s.p1, s.cfg, x->stream, u0, u1));
                if (lng) HIP_TRY(launch_pbox_long1(x->P, se_args, s.p1, nullptr, s.lg, x->stream));
                HIP_TRY(launch_pbox_step_se1(x->P, se_args, s.p1, s.se, x->stream));
                HIP_TRY(launch_pbox_tau(x->P, s.se, s.cfg, x->stream, t0, t1));
                ++x->n_eager;
                continue;
            }
            if (steep) {  // price -> update -> step -> tau
                hipEvent_t v0 = nullptr, v1 = nullptr;
                if (x->timing) SPX_TRY(vtb_events(x, &v0, &v1));
                HIP_TRY(launch_pbox_price_se(x->P, se_args, s.se, s.secfg, false, x->stream, p0, p1));
                if (p0) HIP_TRY(hipEventRecord(x->ev_xend[x->n_price - 1], x->stream));
                HIP_TRY(launch_pbox_update(x->P, se_args, s.cfg, x->stream, u0, u1));
                HIP_TRY(launch_pbox_step_se(x->P, se_args, s.se, x->stream));
                HIP_TRY(launch_pbox_tau(x->P, s.se, s.cfg, x->stream, v0, v1));
                ++x->n_eager;
                continue;
            }
            if (fr) {  // k_pbox_vtb in front while the host last saw phase 1 or a stale y, as below
                if (s.phase1 && (s.ninf > 0 || s.y_stale)) {
                    s.y_dirty = true;
                    hipEvent_t v0 = nullptr, v1 = nullptr;
                    if (x->timing) SPX_TRY(vtb_events(x, &v0, &v1));
                    HIP_TRY(launch_pbox_vtb(x->P, s.p1, s.cfg, x->stream, v0, v1));
                }
                HIP_TRY(launch_pbox_price_f(x->P, s.args, s.p1, s.fr, s.cfg, x->stream, p0, p1));
                if (p0) HIP_TRY(hipEventRecord(x->ev_xend[x->n_price - 1], x->stream));
                HIP_TRY(launch_pbox_update_f(x->P, s.args, s.p1, s.fr, s.cfg, x->stream, u0, u1));
                if (lng && p1pass) HIP_TRY(launch_pbox_long1(x->P, s.args, s.p1, &s.fr, s.lg, x->stream));
                HIP_TRY(launch_pbox_step_f(x->P, s.args, s.p1, s.fr, x->stream));
                ++x->n_eager;
                continue;
            }
            if (s.phase1 && (s.ninf > 0 || s.y_stale)) {
                s.y_dirty = true;
                hipEvent_t v0 = nullptr, v1 = nullptr;
                if (x->timing) {
                    while (s.ev_vtb.size() < 2 * (s.n_vtb + 1)) {
                        hipEvent_t e;
                        HIP_TRY(hipEventCreate(&e));
                        s.ev_vtb.push_back(e);
                    }
                    v0 = s.ev_vtb[2 * s.n_vtb];
                    v1 = s.ev_vtb[2 * s.n_vtb + 1];
                    ++s.n_vtb;
                }
                HIP_TRY(launch_pbox_vtb(x->P, s.p1, s.cfg, x->stream, v0, v1));
                HIP_TRY(launch_pbox_price1(x->P, s.args, s.p1, s.cfg, x->stream, p0, p1));
                if (p0) HIP_TRY(hipEventRecord(x->ev_xend[x->n_price - 1], x->stream));
                HIP_TRY(launch_pbox_update1(x->P, s.args, s.p1, s.cfg, x->stream, u0, u1));
                if (lng) HIP_TRY(launch_pbox_long1(x->P, s.args, s.p1, nullptr, s.lg, x->stream));
                HIP_TRY(launch_pbox_step1(x->P, s.args, s.p1, x->stream));
                ++x->n_eager;
                continue;
            }
            HIP_TRY(launch_pbox_price(x->P, s.args, s.cfg, x->stream, p0, p1));
            if (p0) HIP_TRY(hipEventRecord(x->ev_xend[x->n_price - 1], x->stream));
            HIP_TRY(launch_pbox_update(x->P, s.args, s.cfg, x->stream, u0, u1));
            HIP_TRY(launch_pbox_step(x->P, s.args, x->stream));
            ++x->n_eager;
        }
        SPX_TRY(read_state(x));
        if (s.phase1) SPX_TRY(read_phase(x));
    }
    return SPX_OK;
}

int pbox_on_reset(spx_ctx* x) {
    if (x->pbox.args.rec) {
        HIP_TRY(hipMemsetAsync(x->pbox.args.rec, 0, sizeof(PboxRec), x->stream));
        HIP_TRY(hipMemsetAsync(x->pbox.p1.ph, 0, sizeof(PboxPhase), x->stream));  // (launch_reset rebuilds y)
    }
    if (x->pbox.lg.lrec) HIP_TRY(hipMemsetAsync(x->pbox.lg.lrec, 0, sizeof(PboxLongRec), x->stream));
    x->pbox.checked = false;
    x->pbox.y_dirty = false;
    x->pbox.ninf = x->pbox.y_stale = 0;
    x->pbox.se_stale = true;
    x->pbox.warm = false;  // the slack basis again
    return SPX_OK;
}

int pbox_binv_copy(spx_ctx* x) {
    if (x->pbox.wx_S) return SPX_OK;
    return x->alloc(&x->pbox.wx_S, (size_t)x->m * (size_t)x->L);
}

void pbox_weights_lost(spx_ctx* x) { x->pbox.se_stale = true; }

void pbox_basis_set(spx_ctx* x) { x->pbox.warm = true; }

void pbox_on_change(spx_ctx* x) { x->pbox.checked = false; }

int pbox_on_create(spx_ctx* x) {
    x->pbox.phase1 = (x->opts.flags & SPX_FLAG_PRIMAL_PHASE1) != 0;
    x->pbox.rule = (x->opts.flags & SPX_FLAG_PRIMAL_STEEPEST) ? SPX_PRIMAL_PRICING_STEEPEST : SPX_PRIMAL_PRICING_DANTZIG;
    x->pbox.winit = (x->opts.flags & SPX_FLAG_PRIMAL_EXACT_WEIGHTS) ? SPX_PRIMAL_WEIGHTS_EXACT : SPX_PRIMAL_WEIGHTS_REFERENCE;
    x->pbox.p1rule = (x->opts.flags & SPX_FLAG_PRIMAL_PHASE1_STEEPEST) ? SPX_PRIMAL_PRICING_STEEPEST : SPX_PRIMAL_PRICING_DANTZIG;
    x->pbox.frrule = (x->opts.flags & SPX_FLAG_PRIMAL_FREE_STEEPEST) ? SPX_PRIMAL_PRICING_STEEPEST : SPX_PRIMAL_PRICING_DANTZIG;
    if (x->pbox.phase1 && x->pbox.rule == SPX_PRIMAL_PRICING_STEEPEST && x->pbox.p1rule != SPX_PRIMAL_PRICING_STEEPEST)
        return fail(SPX_ERR_ARG, "SPX_FLAG_PRIMAL_STEEPEST with SPX_FLAG_PRIMAL_PHASE1: steepest-edge pricing does not "
                    "run during the bounded primal loop's phase 1");
    return SPX_OK;
}

// a reinversion has rebuilt y from c_B: nothing stale; x_b is new, so the rows
// are classified again (the entry check does it itself when one is due)
int pbox_on_reinvert(spx_ctx* x) {
    PboxState& s = x->pbox;
    if (!s.p1.ph) return SPX_OK;
    HIP_TRY(hipMemsetAsync(&s.p1.ph->y_stale, 0, sizeof(int32_t), x->stream));
    s.y_stale = 0;
    s.y_dirty = false;
    if (s.phase1 && s.checked && x->algo == SPX_ALGO_PRIMAL_BOX) {
        // (checked: lb_B is that of this basis)
        if (x->dual.nfree > 0) HIP_TRY(launch_pbox_classify_f(x->P, s.args, s.p1, s.fr, false, x->stream));
        else HIP_TRY(launch_pbox_classify(x->P, s.args, s.p1, false, x->stream));
        SPX_TRY(read_phase(x));
    }
    return SPX_OK;
}

// y = c_B B^-1 where phase-1 pivots left y behind (the device decides: the
// launches do nothing when its mark is clear), then the mark is cleared
int pbox_fresh_y(spx_ctx* x) {
    PboxState& s = x->pbox;
    if (!s.p1.ph || !s.y_dirty) return SPX_OK;
    Pbox1Args a = s.p1;
    a.force = 1;
    HIP_TRY(launch_pbox_vtb(x->P, a, s.cfg, x->stream, nullptr, nullptr));
    HIP_TRY(hipMemsetAsync(&s.p1.ph->y_stale, 0, sizeof(int32_t), x->stream));
    s.y_stale = 0;
    s.y_dirty = false;
    return SPX_OK;
}

}  // namespace spx_host

using namespace spx_host;

extern "C" {

int spx_get_primal_flips(spx_ctx* x, int64_t out[2]) {
    if (!x || !out) return fail(SPX_ERR_ARG, "NULL argument");
    out[0] = out[1] = 0;
    if (!x->pbox.args.rec) return SPX_OK;  // no bounded primal pass yet
    PboxRec r;
    HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipMemcpy(&r, x->pbox.args.rec, sizeof r, hipMemcpyDeviceToHost));
    out[0] = r.flips;
    out[1] = r.to_upper;
    return SPX_OK;
}

int spx_set_primal_phase1(spx_ctx* x, int32_t on) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    if (x->stepped_price) return fail(SPX_ERR_STATE, "spx_set_primal_phase1 between spx_price and spx_pivot");
    if (on && x->pbox.rule == SPX_PRIMAL_PRICING_STEEPEST && x->pbox.p1rule != SPX_PRIMAL_PRICING_STEEPEST)
        return fail(SPX_ERR_STATE, "spx_set_primal_phase1: phase 1 does not run with steepest-edge pricing "
                    "(spx_set_primal_pricing); set SPX_PRIMAL_PRICING_DANTZIG first");
    SPX_TRY(pbox_fresh_y(x));
    x->pbox.phase1 = on != 0;
    x->pbox.checked = false;  // the entry check decides again (and classifies)
    return SPX_OK;
}

int spx_set_primal_pricing(spx_ctx* x, int32_t rule) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    if (rule != SPX_PRIMAL_PRICING_DANTZIG && rule != SPX_PRIMAL_PRICING_STEEPEST)
        return fail(SPX_ERR_ARG, "bad primal pricing rule %d", rule);
    if (rule == SPX_PRIMAL_PRICING_STEEPEST && x->pbox.phase1 && x->pbox.p1rule != SPX_PRIMAL_PRICING_STEEPEST)
        return fail(SPX_ERR_STATE, "spx_set_primal_pricing: steepest-edge pricing does not run with the bounded primal "
                    "loop's phase 1 (spx_set_primal_phase1); switch phase 1 off first");
    if (rule == SPX_PRIMAL_PRICING_STEEPEST && x->dual.nfree > 0 && x->pbox.frrule != SPX_PRIMAL_PRICING_STEEPEST)
        return fail(SPX_ERR_STATE, "spx_set_primal_pricing: steepest-edge pricing does not run with free columns (%lld of "
                    "them, spx_set_bounds_lu)", (long long)x->dual.nfree);
    if (rule != x->pbox.rule) x->pbox.se_stale = true;  // a change of rule restarts the weights
    x->pbox.rule = rule;
    return SPX_OK;
}

int spx_set_primal_phase_one_pricing(spx_ctx* x, int32_t rule) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    if (rule != SPX_PRIMAL_PRICING_DANTZIG && rule != SPX_PRIMAL_PRICING_STEEPEST)
        return fail(SPX_ERR_ARG, "bad primal phase-1 pricing rule %d", rule);
    if (rule == SPX_PRIMAL_PRICING_DANTZIG && x->pbox.phase1 && x->pbox.rule == SPX_PRIMAL_PRICING_STEEPEST)
        return fail(SPX_ERR_STATE, "spx_set_primal_phase_one_pricing: SPX_PRIMAL_PRICING_DANTZIG in phase 1 does not run "
                    "with steepest-edge pricing (spx_set_primal_pricing) while phase 1 is on (spx_set_primal_phase1); "
                    "switch phase 1 off or set SPX_PRIMAL_PRICING_DANTZIG first");
    x->pbox.p1rule = rule;  // (the weights do not depend on the phase: nothing restarts)
    return SPX_OK;
}

int spx_set_primal_phase_one_ratio(spx_ctx* x, int32_t rule) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    if (rule != SPX_PRIMAL_RATIO_TEXTBOOK && rule != SPX_PRIMAL_RATIO_LONG_STEP)
        return fail(SPX_ERR_ARG, "bad primal phase-1 ratio rule %d", rule);
    x->pbox.p1ratio = rule;  // (read per pass: nothing restarts, nothing is invalidated)
    return SPX_OK;
}

int spx_get_primal_long_steps(spx_ctx* x, int64_t out[4]) {
    if (!x || !out) return fail(SPX_ERR_ARG, "NULL argument");
    out[0] = out[1] = out[2] = 0;
    out[3] = x->pbox.p1ratio;
    if (!x->pbox.lg.lrec) return SPX_OK;  // no long-step pass yet
    PboxLongRec r;
    HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipMemcpy(&r, x->pbox.lg.lrec, sizeof r, hipMemcpyDeviceToHost));
    out[0] = r.passed;
    out[1] = r.passes;
    out[2] = r.max_pass;
    return SPX_OK;
}

int spx_set_primal_free_pricing(spx_ctx* x, int32_t rule) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    if (rule != SPX_PRIMAL_PRICING_DANTZIG && rule != SPX_PRIMAL_PRICING_STEEPEST)
        return fail(SPX_ERR_ARG, "bad primal free-column pricing rule %d", rule);
    if (rule == SPX_PRIMAL_PRICING_DANTZIG && x->dual.nfree > 0 && x->pbox.rule == SPX_PRIMAL_PRICING_STEEPEST)
        return fail(SPX_ERR_STATE, "spx_set_primal_free_pricing: SPX_PRIMAL_PRICING_DANTZIG with free columns (%lld of "
                    "them, spx_set_bounds_lu) does not run with steepest-edge pricing (spx_set_primal_pricing); set "
                    "SPX_PRIMAL_PRICING_DANTZIG there first", (long long)x->dual.nfree);
    x->pbox.frrule = rule;  // (the weights do not depend on the bounds: nothing restarts)
    return SPX_OK;
}

int spx_get_primal_weights(spx_ctx* x, double* w) {
    if (!x || !w) return fail(SPX_ERR_ARG, "NULL argument");
    if (x->pbox.rule != SPX_PRIMAL_PRICING_STEEPEST)
        return fail(SPX_ERR_STATE, "no primal pricing weights: the bounded primal loop's entering rule is Dantzig");
    if (x->algo != SPX_ALGO_PRIMAL_BOX)
        return fail(SPX_ERR_STATE, "no primal pricing weights: the context does not run SPX_ALGO_PRIMAL_BOX");
    if (x->broken) return fail(SPX_ERR_STATE, "no valid basis (a failed spx_set_basis): call spx_reset");
    PboxState& s = x->pbox;
    SPX_TRY(pbox_setup(x));
    SPX_TRY(pbox_se_setup(x));
    SPX_TRY(pbox_se_restart(x));
    // a recurrence the next pricing pass would have applied: the same kernel applies it now (the device decides)
    HIP_TRY(launch_pbox_price_se(x->P, s.args, s.se, s.secfg, true, x->stream, nullptr, nullptr));
    HIP_TRY(hipMemsetAsync(&s.se.se->pend, 0, sizeof(int32_t), x->stream));
    HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipMemcpy(w, s.se.gamma, sizeof(double) * (size_t)x->n, hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spx_set_primal_weight_init(spx_ctx* x, int32_t mode) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    if (mode != SPX_PRIMAL_WEIGHTS_REFERENCE && mode != SPX_PRIMAL_WEIGHTS_EXACT)
        return fail(SPX_ERR_ARG, "bad primal weight start mode %d", mode);
    x->pbox.winit = mode;
    return SPX_OK;
}

int spx_refresh_primal_weights(spx_ctx* x) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    if (x->pbox.rule != SPX_PRIMAL_PRICING_STEEPEST)
        return fail(SPX_ERR_STATE, "no primal pricing weights: the bounded primal loop's entering rule is Dantzig");
    if (x->algo != SPX_ALGO_PRIMAL_BOX)
        return fail(SPX_ERR_STATE, "no primal pricing weights: the context does not run SPX_ALGO_PRIMAL_BOX");
    if (x->broken) return fail(SPX_ERR_STATE, "no valid basis (a failed spx_set_basis): call spx_reset");
    if (x->stepped_price) return fail(SPX_ERR_STATE, "spx_refresh_primal_weights between spx_price and spx_pivot");
    PboxState& s = x->pbox;
    SPX_TRY(pbox_setup(x));
    SPX_TRY(pbox_se_setup(x));
    SPX_TRY(pbox_wexact_run(x));
    // the weights are those of the current basis: a recurrence recorded for the last pivot is dropped
    HIP_TRY(hipMemsetAsync(&s.se.se->pend, 0, sizeof(int32_t), x->stream));
    s.se_stale = false;
    return SPX_OK;
}

int spx_loop_layout(spx_ctx* x, int32_t out[SPX_LOOP_LAYOUT_FIELDS]) {
    if (!x || !out) return fail(SPX_ERR_ARG, "NULL argument");
    for (int i = 0; i < SPX_LOOP_LAYOUT_FIELDS; ++i) out[i] = -1;
    if (x->dual.args.rho) {  // dual_setup ran
        const DualCfg& c = x->dual.cfg;
        out[0] = c.price_lds ? 1 : 0;
        out[1] = c.update_lds ? 1 : 0;
        out[2] = c.se_update_lds ? 1 : 0;
        out[3] = (c.se_update_lds && c.se_rho_lds) ? 1 : 0;
    }
    if (x->pbox.args.rec) {  // pbox_setup ran
        out[4] = x->pbox.cfg.price_lds ? 1 : 0;
        out[5] = x->pbox.cfg.update_lds ? 1 : 0;
    }
    if (x->pbox.se.se) out[6] = x->pbox.secfg.lds_vecs;  // pbox_se_setup ran
    out[7] = x->P.slack_unit ? 1 : 0;
    return SPX_OK;
}

int spx_pbox_wexact_times(spx_ctx* x, double* ms, int64_t* launches) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    if (!x->timing) return fail(SPX_ERR_STATE, "context created without SPX_FLAG_TIMING");
    HIP_TRY(hipStreamSynchronize(x->stream));
    double t = 0.0;
    for (size_t i = 0; i < x->pbox.n_wx; ++i) {
        float e = 0.f;
        HIP_TRY(hipEventElapsedTime(&e, x->pbox.ev_wx[2 * i], x->pbox.ev_wx[2 * i + 1]));
        t += e;
    }
    if (ms) *ms = t;
    if (launches) *launches = (int64_t)x->pbox.n_wx;
    x->pbox.n_wx = 0;
    return SPX_OK;
}

int spx_pbox_vtb_times(spx_ctx* x, double* ms, int64_t* launches) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    if (!x->timing) return fail(SPX_ERR_STATE, "context created without SPX_FLAG_TIMING");
    HIP_TRY(hipStreamSynchronize(x->stream));
    double t = 0.0;
    for (size_t i = 0; i < x->pbox.n_vtb; ++i) {
        float e = 0.f;
        HIP_TRY(hipEventElapsedTime(&e, x->pbox.ev_vtb[2 * i], x->pbox.ev_vtb[2 * i + 1]));
        t += e;
    }
    if (ms) *ms = t;
    if (launches) *launches = (int64_t)x->pbox.n_vtb;
    x->pbox.n_vtb = 0;
    return SPX_OK;
}

int spx_get_primal_phase1(spx_ctx* x, int64_t out[4]) {
    if (!x || !out) return fail(SPX_ERR_ARG, "NULL argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!x->pbox.p1.ph) return SPX_OK;  // no bounded primal pass yet
    PboxPhase r;
    HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipMemcpy(&r, x->pbox.p1.ph, sizeof r, hipMemcpyDeviceToHost));
    out[0] = r.passes;
    out[1] = r.pivots;
    out[2] = r.ninf0;
    out[3] = r.ninf;
    return SPX_OK;
}

}  // extern "C"
