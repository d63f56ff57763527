// spx_api_pbox.cpp — the bounded primal simplex loop's host side (kernels:
// spx_pbox.h): its state (PboxState, spx_ctx.h, with the invariants), the entry
// check, the pass loop, the hooks through which the rest of the runtime touches
// any of it, and the entry point that is this loop's alone.  The bounds and
// placements are the dual loop's state, reached through spx_api_dual.cpp's hooks.
#include <cmath>

#include "spx_ctx.h"

using namespace spx;

namespace spx_host {

namespace {

// Entry check, before the first pass after anything set the basis, the bounds,
// b, c or the algorithm from outside: placements kept (a column at an upper
// bound that no longer exists goes to lower), x_b recomputed from them, and
// -feas_tol <= x_b[i] <= ub_B[i] + feas_tol on the host.  No normalisation by
// reduced-cost sign: that is the dual loop's.
int pbox_check_entry(spx_ctx* x) {
    const size_t m = (size_t)x->m;
    SPX_TRY(box_replace_xb(x));
    std::vector<double> xb(m), ubB(m);
    std::vector<int64_t> bix(m);
    HIP_TRY(hipStreamSynchronize(x->stream));
    HIP_TRY(hipMemcpy(xb.data(), x->P.x_b, m * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ubB.data(), x->pbox.args.ub_B, m * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(bix.data(), x->P.b_ixs, m * sizeof(int64_t), hipMemcpyDeviceToHost));
    const double tol = x->opts.feas_tol;
    for (size_t i = 0; i < m; ++i) {
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
    HIP_TRY(pbox_prepare(x->P, x->cus, x->opts.price_grid, (x->opts.flags & SPX_FLAG_GLOBAL_Y) != 0, &s.cfg));
    SPX_TRY(x->alloc(&s.args.parts, (size_t)s.cfg.price_grid));
    SPX_TRY(x->alloc(&s.args.rparts, (size_t)s.cfg.update_grid));
    s.args.ub = x->dual.args.ub;
    s.args.ub_B = x->dual.args.ub_B;
    s.args.at_upper = x->dual.args.at_upper;
    s.args.b_eff = x->b;
    s.args.price_grid = s.cfg.price_grid;
    s.args.update_grid = s.cfg.update_grid;
    s.args.piv_tol = x->opts.piv_tol;
    SPX_TRY(x->alloc(&s.args.rec, 1));
    return SPX_OK;
}

// k pivots or a terminal status.  A pass is three eager launches and makes a
// pivot or a flip; the host enqueues as many passes as pivots are missing,
// synchronises once, and goes round again for the flips' share.  Every kernel
// returns at once when the device status is not running or the limit is reached.
int iterate_pbox(spx_ctx* x, int64_t k) {
    SPX_TRY(pbox_setup(x));
    if (!x->pbox.checked) SPX_TRY(pbox_check_entry(x));
    const PboxState& s = x->pbox;
    const int64_t target = x->pivots + k;
    SPX_TRY(set_limit(x, target));
    while (x->status == SPX_STATUS_MAX_ITER && x->pivots < target) {
        const int64_t round = target - x->pivots;
        for (int64_t i = 0; i < round; ++i) {
            hipEvent_t p0 = nullptr, p1 = nullptr, u0 = nullptr, u1 = nullptr;
            if (x->timing) SPX_TRY(pass_events(x, &p0, &p1, &u0, &u1));
            HIP_TRY(launch_pbox_price(x->P, s.args, s.cfg, x->stream, p0, p1));
            if (p0) HIP_TRY(hipEventRecord(x->ev_xend[x->n_price - 1], x->stream));
            HIP_TRY(launch_pbox_update(x->P, s.args, s.cfg, x->stream, u0, u1));
            HIP_TRY(launch_pbox_step(x->P, s.args, x->stream));
            ++x->n_eager;
        }
        SPX_TRY(read_state(x));
    }
    return SPX_OK;
}

int pbox_on_reset(spx_ctx* x) {
    if (x->pbox.args.rec) HIP_TRY(hipMemsetAsync(x->pbox.args.rec, 0, sizeof(PboxRec), x->stream));
    x->pbox.checked = false;
    return SPX_OK;
}

void pbox_on_change(spx_ctx* x) { x->pbox.checked = false; }

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

}  // extern "C"
