// spx_api_ranging.cpp — sensitivity ranging's host side (kernels: spx_ranging.h,
// spx_bndrange.h): its state (RangingState and
// BoundRangingState, spx_ctx.h), the refusals, and the entry points.  A call reads the context and writes only its own
// buffers: the basis, the placements, x_b, y, S, the pending pivot record, the
// steepest-edge record and weights, the pivot count and the status stay as they
// are (flush is the readbacks': a y left stale by phase 1 is refreshed first).
#include <cmath>
#include <vector>

#include "spx_ctx.h"

using namespace spx;

namespace spx_host {

namespace {

int ranging_refusal(spx_ctx* x, const char* who) {
    if (x->algo == SPX_ALGO_PRIMAL)
        return fail(SPX_ERR_STATE, "%s: no ranging under SPX_ALGO_PRIMAL: it runs at an optimum of SPX_ALGO_DUAL or "
                    "SPX_ALGO_PRIMAL_BOX (spx_set_algorithm, then solve)", who);
    if (x->opts.nranks > 1 || x->P.row_shard)
        return fail(SPX_ERR_STATE, "%s needs one rank and replicated B^-1 (nranks %d%s)", who, x->opts.nranks,
                    x->P.row_shard ? ", row-sharded" : "");
    if (x->P.win) return fail(SPX_ERR_STATE, "%s needs the explicit B^-1 (eta window %d)", who, (int)x->P.win);
    if (x->broken) return fail(SPX_ERR_STATE, "no valid basis (a failed spx_set_basis): call spx_reset");
    if (x->stepped_price) return fail(SPX_ERR_STATE, "%s between spx_price and spx_pivot", who);
    if (x->status != SPX_STATUS_OPTIMUM_FOUND)
        return fail(SPX_ERR_STATE, "%s: the context is not at an optimum (status %d: %s): ranging describes the optimal "
                    "basis, so solve first, and again after spx_set_rhs / spx_set_cost / spx_set_bounds / spx_set_basis "
                    "/ spx_reset", who, (int)x->status, spx_status_string(x->status));
    return SPX_OK;
}

// the buffers and the geometry, on first use
int ranging_setup(spx_ctx* x) {
    RangingState& g = x->rng;
    if (g.args.cparts) return SPX_OK;
    const size_t n = (size_t)x->n, m = (size_t)x->m;
    g.cfg = rng_geometry(x->m, x->n);
    HIP_TRY(rng_prepare());
    SPX_TRY(pbox_binv_copy(x));
    SPX_TRY(x->alloc(&g.d, n));
    SPX_TRY(x->alloc(&g.free_flags, n));
    SPX_TRY(x->alloc(&g.args.sk, (size_t)g.cfg.cap));
    SPX_TRY(x->alloc(&g.args.sig, (size_t)g.cfg.cap));
    SPX_TRY(x->alloc(&g.args.col, (size_t)g.cfg.cap));
    SPX_TRY(x->alloc(&g.args.rparts, g.cfg.rparts));
    SPX_TRY(x->alloc(&g.args.c_down, n));
    SPX_TRY(x->alloc(&g.args.c_up, n));
    SPX_TRY(x->alloc(&g.args.c_kdown, n));
    SPX_TRY(x->alloc(&g.args.c_kup, n));
    SPX_TRY(x->alloc(&g.args.r_down, m));
    SPX_TRY(x->alloc(&g.args.r_up, m));
    SPX_TRY(x->alloc(&g.args.r_kdown, m));
    SPX_TRY(x->alloc(&g.args.r_kup, m));
    SPX_TRY(x->alloc(&g.args.cparts, g.cfg.cparts));
    g.args.d = g.d;
    g.args.cap = g.cfg.cap;
    g.args.col_tiles = g.cfg.col_tiles;
    g.args.rhs_blocks = g.cfg.rhs_blocks;
    return SPX_OK;
}

// what a call reads of the context as it is now: the bounds' buffers (absent
// while no bound was ever set), the free columns, the tolerance
int ranging_bind(spx_ctx* x) {
    RangingState& g = x->rng;
    g.args.S = x->pbox.wx_S;
    g.args.at_upper = x->dual.args.at_upper;
    g.args.ub_B = x->dual.args.ub_B;
    g.args.tol = x->opts.piv_tol;
    g.args.is_free = nullptr;
    if (x->dual.nfree > 0) {
        std::vector<int8_t> fr((size_t)x->n);
        for (size_t j = 0; j < fr.size(); ++j) fr[j] = x->dual.lb[j] == -INFINITY ? 1 : 0;
        HIP_TRY(hipStreamSynchronize(x->stream));
        HIP_TRY(hipMemcpy(g.free_flags, fr.data(), fr.size(), hipMemcpyHostToDevice));
        g.args.is_free = g.free_flags;
    }
    return SPX_OK;
}

int ranging_events(spx_ctx* x, int which, hipEvent_t* e0, hipEvent_t* e1) {
    RangingState& g = x->rng;
    *e0 = *e1 = nullptr;
    if (!x->timing) return SPX_OK;
    while (g.ev[which].size() < 2 * (g.n_ev[which] + 1)) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        g.ev[which].push_back(e);
    }
    *e0 = g.ev[which][2 * g.n_ev[which]];
    *e1 = g.ev[which][2 * g.n_ev[which] + 1];
    ++g.n_ev[which];
    return SPX_OK;
}

// bound ranging's buffers and geometry, on first use
int bound_setup(spx_ctx* x) {
    BoundRangingState& g = x->brng;
    if (g.args.parts) return SPX_OK;
    const size_t n = (size_t)x->n;
    g.cfg = bnd_geometry(x->m, x->n);
    HIP_TRY(bnd_prepare());
    SPX_TRY(pbox_binv_copy(x));
    SPX_TRY(x->alloc(&g.free_flags, n));
    SPX_TRY(x->alloc(&g.args.col, (size_t)g.cfg.cap));
    SPX_TRY(x->alloc(&g.args.kind, (size_t)g.cfg.cap));
    SPX_TRY(x->alloc(&g.args.ubj, (size_t)g.cfg.cap));
    SPX_TRY(x->alloc(&g.args.down, n));
    SPX_TRY(x->alloc(&g.args.up, n));
    SPX_TRY(x->alloc(&g.args.kdown, n));
    SPX_TRY(x->alloc(&g.args.kup, n));
    SPX_TRY(x->alloc(&g.args.parts, g.cfg.parts));
    g.args.cap = g.cfg.cap;
    g.args.row_blocks = g.cfg.row_blocks;
    return SPX_OK;
}

// what a call reads of the context as it is now (as ranging_bind)
int bound_bind(spx_ctx* x) {
    BoundRangingState& g = x->brng;
    g.args.S = x->pbox.wx_S;
    g.args.ub = x->dual.args.ub;
    g.args.at_upper = x->dual.args.at_upper;
    g.args.ub_B = x->dual.args.ub_B;
    g.args.tol = x->opts.piv_tol;
    g.args.is_free = nullptr;
    if (x->dual.nfree > 0) {
        std::vector<int8_t> fr((size_t)x->n);
        for (size_t j = 0; j < fr.size(); ++j) fr[j] = x->dual.lb[j] == -INFINITY ? 1 : 0;
        HIP_TRY(hipStreamSynchronize(x->stream));
        HIP_TRY(hipMemcpy(g.free_flags, fr.data(), fr.size(), hipMemcpyHostToDevice));
        g.args.is_free = g.free_flags;
    }
    return SPX_OK;
}

// z + sign * delta * mult; a multiplier that is exactly 0 gives z even where delta is +inf
double range_end(double z, double sign, double delta, double mult) {
    return mult == 0.0 ? z : z + sign * delta * mult;
}

}  // namespace

}  // namespace spx_host

using namespace spx_host;

extern "C" {

int spx_ranging_cost(spx_ctx* x, double* down, double* up, int64_t* block_down, int64_t* block_up) {
    if (!x || !down || !up) return fail(SPX_ERR_ARG, "NULL argument");
    SPX_TRY(ranging_refusal(x, "spx_ranging_cost"));
    SPX_TRY(ranging_setup(x));
    SPX_TRY(flush(x));
    SPX_TRY(ranging_bind(x));
    RangingState& g = x->rng;
    hipEvent_t e0, e1;
    SPX_TRY(ranging_events(x, 0, &e0, &e1));
    if (e0) HIP_TRY(hipEventRecord(e0, x->stream));
    HIP_TRY(launch_reduced_costs(x->P, g.d, x->stream));
    HIP_TRY(launch_materialize(x->P, x->pbox.wx_S, x->stream));
    HIP_TRY(launch_rng_cost(x->P, g.args, g.cfg, x->stream));
    if (e1) HIP_TRY(hipEventRecord(e1, x->stream));
    HIP_TRY(hipStreamSynchronize(x->stream));
    const size_t n = (size_t)x->n;
    HIP_TRY(hipMemcpy(down, g.args.c_down, n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(up, g.args.c_up, n * sizeof(double), hipMemcpyDeviceToHost));
    if (block_down) HIP_TRY(hipMemcpy(block_down, g.args.c_kdown, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (block_up) HIP_TRY(hipMemcpy(block_up, g.args.c_kup, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spx_ranging_rhs(spx_ctx* x, double* down, double* up, int64_t* leave_down, int64_t* leave_up) {
    if (!x || !down || !up) return fail(SPX_ERR_ARG, "NULL argument");
    SPX_TRY(ranging_refusal(x, "spx_ranging_rhs"));
    SPX_TRY(ranging_setup(x));
    SPX_TRY(flush(x));
    SPX_TRY(ranging_bind(x));
    RangingState& g = x->rng;
    hipEvent_t e0, e1;
    SPX_TRY(ranging_events(x, 1, &e0, &e1));
    if (e0) HIP_TRY(hipEventRecord(e0, x->stream));
    HIP_TRY(launch_materialize(x->P, x->pbox.wx_S, x->stream));
    HIP_TRY(launch_rng_rhs(x->P, g.args, g.cfg, x->stream));
    if (e1) HIP_TRY(hipEventRecord(e1, x->stream));
    HIP_TRY(hipStreamSynchronize(x->stream));
    const size_t m = (size_t)x->m;
    HIP_TRY(hipMemcpy(down, g.args.r_down, m * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(up, g.args.r_up, m * sizeof(double), hipMemcpyDeviceToHost));
    if (leave_down) HIP_TRY(hipMemcpy(leave_down, g.args.r_kdown, m * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (leave_up) HIP_TRY(hipMemcpy(leave_up, g.args.r_kup, m * sizeof(int64_t), hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spx_ranging_bound(spx_ctx* x, double* down, double* up, int64_t* leave_down, int64_t* leave_up) {
    if (!x || !down || !up) return fail(SPX_ERR_ARG, "NULL argument");
    SPX_TRY(ranging_refusal(x, "spx_ranging_bound"));
    SPX_TRY(bound_setup(x));
    SPX_TRY(flush(x));
    SPX_TRY(bound_bind(x));
    BoundRangingState& g = x->brng;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (x->timing) {
        while (g.ev.size() < 2 * (g.n_ev + 1)) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            g.ev.push_back(e);
        }
        e0 = g.ev[2 * g.n_ev];
        e1 = g.ev[2 * g.n_ev + 1];
        ++g.n_ev;
    }
    if (e0) HIP_TRY(hipEventRecord(e0, x->stream));
    HIP_TRY(launch_materialize(x->P, x->pbox.wx_S, x->stream));
    HIP_TRY(launch_rng_bound(x->P, g.args, g.cfg, x->stream));
    if (e1) HIP_TRY(hipEventRecord(e1, x->stream));
    HIP_TRY(hipStreamSynchronize(x->stream));
    const size_t n = (size_t)x->n;
    HIP_TRY(hipMemcpy(down, g.args.down, n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(up, g.args.up, n * sizeof(double), hipMemcpyDeviceToHost));
    if (leave_down) HIP_TRY(hipMemcpy(leave_down, g.args.kdown, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (leave_up) HIP_TRY(hipMemcpy(leave_up, g.args.kup, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spx_ranging_bound_times(spx_ctx* x, double* ms, int64_t* launches) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    if (!x->timing) return fail(SPX_ERR_STATE, "context created without SPX_FLAG_TIMING");
    HIP_TRY(hipStreamSynchronize(x->stream));
    BoundRangingState& g = x->brng;
    double t = 0.0;
    for (size_t i = 0; i < g.n_ev; ++i) {
        float e = 0.f;
        HIP_TRY(hipEventElapsedTime(&e, g.ev[2 * i], g.ev[2 * i + 1]));
        t += e;
    }
    if (ms) *ms = t;
    if (launches) *launches = (int64_t)g.n_ev;
    g.n_ev = 0;
    return SPX_OK;
}

int spx_ranging_objective(spx_ctx* x, int32_t what, const double* down, const double* up, double* obj_down,
                          double* obj_up) {
    if (!x || !down || !up || !obj_down || !obj_up) return fail(SPX_ERR_ARG, "NULL argument");
    if (what != SPX_RANGING_COST && what != SPX_RANGING_RHS && what != SPX_RANGING_BOUND)
        return fail(SPX_ERR_ARG, "unknown kind of ranging %d (SPX_RANGING_COST, _RHS or _BOUND)", (int)what);
    SPX_TRY(ranging_refusal(x, "spx_ranging_objective"));
    const size_t n = (size_t)x->n, m = (size_t)x->m;
    double z = 0.0;
    SPX_TRY(spx_objective(x, &z));
    if (what == SPX_RANGING_COST) {  // z +- delta x_j, x in the caller's variables
        std::vector<double> xv(n);
        SPX_TRY(spx_get_primal(x, xv.data(), nullptr));
        for (size_t j = 0; j < n; ++j) {
            obj_down[j] = range_end(z, -1.0, down[j], xv[j]);
            obj_up[j] = range_end(z, 1.0, up[j], xv[j]);
        }
    } else if (what == SPX_RANGING_RHS) {  // z +- delta y_r
        std::vector<double> y(m);
        SPX_TRY(spx_get_state(x, nullptr, nullptr, y.data(), nullptr, nullptr, nullptr, nullptr));
        for (size_t r = 0; r < m; ++r) {
            obj_down[r] = range_end(z, -1.0, down[r], y[r]);
            obj_up[r] = range_end(z, 1.0, up[r], y[r]);
        }
    } else {  // a non-basic column that is not free moves with its bound: z -+ delta d_j; basic or free: z
        std::vector<double> d(n);
        std::vector<int32_t> pos(n);
        SPX_TRY(spx_reduced_costs(x, d.data()));
        HIP_TRY(hipMemcpy(pos.data(), x->P.nb_pos, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t j = 0; j < n; ++j) {
            const bool moves = pos[j] >= 0 && !(x->dual.nfree > 0 && x->dual.lb[j] == -INFINITY);
            obj_down[j] = moves ? range_end(z, 1.0, down[j], d[j]) : z;
            obj_up[j] = moves ? range_end(z, -1.0, up[j], d[j]) : z;
        }
    }
    return SPX_OK;
}

int spx_ranging_times(spx_ctx* x, double ms[2], int64_t launches[2]) {
    if (!x) return fail(SPX_ERR_ARG, "ctx is NULL");
    if (!x->timing) return fail(SPX_ERR_STATE, "context created without SPX_FLAG_TIMING");
    HIP_TRY(hipStreamSynchronize(x->stream));
    RangingState& g = x->rng;
    for (int w = 0; w < 2; ++w) {
        double t = 0.0;
        for (size_t i = 0; i < g.n_ev[w]; ++i) {
            float e = 0.f;
            HIP_TRY(hipEventElapsedTime(&e, g.ev[w][2 * i], g.ev[w][2 * i + 1]));
            t += e;
        }
        if (ms) ms[w] = t;
        if (launches) launches[w] = (int64_t)g.n_ev[w];
        g.n_ev[w] = 0;
    }
    return SPX_OK;
}

}  // extern "C"
