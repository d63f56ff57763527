// spx_dual.hip — gfx950 kernels of the dual simplex loop (spx_dual.h).
#include "spx_dual.h"

#include <hip/hip_ext.h>

#include "spx_common.h"

namespace spx {

namespace {

// (key, column) argmin over the wave carrying the winner's a and d; every lane
// ends with the result (xor butterfly, argmin_better's order)
__device__ __forceinline__ void wave_argmin4(DualPartial& w) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double k2 = __shfl_xor(w.key, off, 64);
        const int64_t j2 = __shfl_xor(w.idx, off, 64);
        const double a2 = __shfl_xor(w.a, off, 64);
        const double d2 = __shfl_xor(w.d, off, 64);
        const bool t = argmin_better(k2, j2, w.key, w.idx);
        w.key = t ? k2 : w.key;
        w.idx = t ? j2 : w.idx;
        w.a = t ? a2 : w.a;
        w.d = t ? d2 : w.d;
    }
}

// the workgroup's merge of its waves' candidates, with selects on scalars (a
// struct copy per step became a private-memory temporary)
template <int WAVES>
__device__ __forceinline__ DualPartial merge_waves(const DualPartial* red) {
    double key = red[0].key, a = red[0].a, d = red[0].d;
    int64_t idx = red[0].idx;
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
        const double k2 = red[w].key, a2 = red[w].a, d2 = red[w].d;
        const int64_t j2 = red[w].idx;
        const bool t = argmin_better(k2, j2, key, idx);
        key = t ? k2 : key;
        idx = t ? j2 : idx;
        a = t ? a2 : a;
        d = t ? d2 : d;
    }
    return DualPartial{key, idx, a, d};
}

struct StepState {  // k_dual_step: the loop state, read once by thread 0
    int64_t it, limit, qprev;
    double aqprev;
    int32_t status, y_buf, fresh, cnt;
    int64_t q, p;
    double d_p;
};

}  // namespace

// ---------------------------------------------------------------------------
// Finish of the previous pass's pivot, leaving row, pivot row (one workgroup)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_dual_step(Params P, DualArgs D, int finish_only) {
    constexpr int BLOCK = 1024, WAVES = BLOCK / 64;
    DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = P.m, L = P.L;
    __shared__ StepState S;
    __shared__ ArgMinEntry s_red[WAVES];
    // The kernel is a chain of dependent memory round trips on one CU, so each
    // phase requests everything it needs before its first store: the state and
    // the pass record in one snapshot, the vectors in chunks of CH per thread
    // (loads of a chunk ahead of its stores), the bookkeeping's four loads
    // together on a wave of their own beside the vector updates.
    constexpr int CH = 4;
    if (tid == 0) {
        S.it = st->iter;
        S.limit = st->limit;
        S.qprev = st->q;
        S.aqprev = st->aq;
        S.status = st->status;
        S.y_buf = st->y_buf;
        S.cnt = st->nb_count;
        S.fresh = D.rec->fresh;
        S.q = D.rec->q;
        S.p = D.rec->p;
        S.d_p = D.rec->d_p;
    }
    __syncthreads();
    double* y = S.y_buf ? P.y1 : P.y0;
    int64_t it = S.it, qprev = S.qprev;
    double aqprev = S.aqprev;
    if (S.fresh) {
        // pivot it: alpha = B^-1 A_p is in alpha[(it + 1) & 1] (k_dual_update)
        const int64_t q = S.q, p = S.p;
        const double* al = ((it + 1) & 1) ? P.alpha1 : P.alpha0;
        const double aq = al[q], xq = P.x_b[q];  // (every thread: the same two words)
        const bool book = tid == BLOCK - 64;      // the last wave's lane 0
        int64_t leave = -1;
        double c_p = 0.0;
        int kp = -1, last = -1;
        if (book) {
            leave = P.b_ixs[q];
            c_p = P.c[p];
            kp = P.nb_pos[p];
            last = P.nb_list[S.cnt - 1];
        }
        const double theta = xq / aq, sy = -(S.d_p / aq);
        __syncthreads();  // x_b[q] is read by every thread before its owner overwrites it
        for (int64_t i0 = tid; i0 < L; i0 += (int64_t)CH * BLOCK) {
            double xv[CH], av[CH], yv[CH], rv[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int64_t i = i0 + (int64_t)u * BLOCK;
                xv[u] = i < m ? P.x_b[i] : 0.0;
                av[u] = i < m ? al[i] : 0.0;
                yv[u] = i < L ? y[i] : 0.0;
                rv[u] = i < L ? D.rho[i] : 0.0;  // (rho's padding is 0: so is y's)
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int64_t i = i0 + (int64_t)u * BLOCK;
                if (i < m) P.x_b[i] = (i == q) ? theta : fma(-theta, av[u], xv[u]);
                if (i < L) y[i] = fma(sy, rv[u], yv[u]);
            }
        }
        if (book) {
            P.c_B[q] = c_p;
            P.b_ixs[q] = p;
            // nb_list / nb_pos as pivot_bookkeeping keeps them: swap-remove p, append the leaving column
            int cnt = S.cnt;
            P.nb_list[kp] = last;
            P.nb_pos[last] = kp;
            P.nb_pos[p] = -1;
            --cnt;
            P.nb_list[cnt] = (int32_t)leave;
            P.nb_pos[leave] = cnt;
            ++cnt;
            st->nb_count = cnt;
            st->aq = aq;
            st->s_y = sy;
            st->y_applied = it + 1;  // y and x_b are current: only B^-1 stays pending
            st->xb_applied = it + 1;
            st->p = p;
            st->q = q;
            st->min_e = S.d_p;
            st->iter = it + 1;
            record_pivot(P, it, p, q);
            D.rec->fresh = 0;
        }
        it += 1;
        qprev = q;
        aqprev = aq;
        __syncthreads();  // x_b as this workgroup's threads left it
    }
    if (finish_only || S.status != ST_RUNNING || it >= S.limit) return;

    // leaving row: the most negative x_b below -feas_tol, first index on ties
    double bv = INFINITY;
    int64_t bi = INT64_MAX;
    for (int64_t i = tid; i < m; i += BLOCK) {
        const double v = P.x_b[i];
        if (v < -D.feas_tol && argmin_better(v, i, bv, bi)) {
            bv = v;
            bi = i;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double v2 = __shfl_xor(bv, off, 64);
        const int64_t j2 = __shfl_xor(bi, off, 64);
        if (argmin_better(v2, j2, bv, bi)) {
            bv = v2;
            bi = j2;
        }
    }
    if (lane == 0) s_red[wave] = ArgMinEntry{bv, bi};
    __syncthreads();
    if (tid == 0) {
        ArgMinEntry t = s_red[0];
        for (int w = 1; w < WAVES; ++w)
            if (argmin_better(s_red[w].val, s_red[w].idx, t.val, t.idx)) t = s_red[w];
        S.q = t.idx;
        if (t.idx == INT64_MAX) st->status = ST_OPTIMAL;  // primal feasible: optimum
        else D.rec->q = t.idx;
    }
    __syncthreads();
    const int64_t q = S.q;
    if (q == INT64_MAX) return;

    // rho = row q of the true B^-1 = S[q] + E_q r', r' = S[q'] the pending pivot's
    // row (staged into rbuf: k_dual_update overwrites row q' while other waves
    // still read it)
    const bool pend = it > 0 && qprev >= 0;
    const double* Sq = P.B0 + q * L;
    const double* Sp = P.B0 + (pend ? qprev : q) * L;
    const double* a_prev = (it & 1) ? P.alpha1 : P.alpha0;
    const double aq_prev = pend ? a_prev[q] : 0.0;
    for (int64_t k0 = tid; k0 < L; k0 += (int64_t)CH * BLOCK) {
        double sp[CH], sq[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t k = k0 + (int64_t)u * BLOCK;
            sq[u] = k < L ? Sq[k] : 0.0;
            sp[u] = (pend && k < L) ? Sp[k] : 0.0;
        }
        const double eq = pend ? eta_entry(aq_prev, q, qprev, aqprev) : 0.0;
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t k = k0 + (int64_t)u * BLOCK;
            if (k < L) {
                if (pend) P.rbuf[k] = sp[u];
                D.rho[k] = pend ? fma(eq, sp[u], sq[u]) : sq[u];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Dual ratio test (the hot kernel): two dots per streamed non-basic column
// ---------------------------------------------------------------------------
// One wave per column, grid-stride over nb_list.  A column is L/2 dbl2 in
// chunks of 64 lanes; U chunks are in flight per wave while the previous U are
// multiplied with rho and y (double-buffered registers), non-temporal as
// k_price's A stream.  Per lane the chunks are accumulated in ascending order
// into four partial sums, then one butterfly: a column's a_j and d_j do not
// depend on the grid or on which wave prices it.
template <bool LDS>
__global__ __launch_bounds__(DUAL_BLOCK) void k_dual_price(Params P, DualArgs D) {
    constexpr int WAVES = DUAL_WAVES, U = 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    __shared__ DualPartial s_red[WAVES];
    const DevState* st = P.st;
    const int32_t status = st->status;
    const int32_t cnt = st->nb_count;
    const int32_t y_buf = st->y_buf;
    const int64_t iter = st->iter, limit = st->limit;
    if (status != ST_RUNNING || iter >= limit) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t L = P.L, L2 = L >> 1;
    const int nch = (int)(L2 >> 6);  // chunks of 64 dbl2 (L is a multiple of 128)
    const dbl2* rho_g = reinterpret_cast<const dbl2*>(D.rho);
    const dbl2* y_g = reinterpret_cast<const dbl2*>(y_buf ? P.y1 : P.y0);
    if constexpr (LDS) {
        dbl2* d = reinterpret_cast<dbl2*>(dsm);
        for (int64_t k = tid; k < L2; k += DUAL_BLOCK) {
            d[k] = rho_g[k];
            d[L2 + k] = y_g[k];
        }
        __syncthreads();
    }
    const dbl2* rv = LDS ? reinterpret_cast<const dbl2*>(dsm) : rho_g;
    const dbl2* yv = LDS ? reinterpret_cast<const dbl2*>(dsm) + L2 : y_g;
    const double* rs = reinterpret_cast<const double*>(rv);
    const double* ys = reinterpret_cast<const double*>(yv);

    double bkey = INFINITY, ba = 0.0, bd = 0.0;
    int64_t bidx = INT64_MAX;
    const int nwv = (int)gridDim.x * WAVES;
    for (int s = (int)blockIdx.x * WAVES + wave; s < cnt; s += nwv) {
        const int64_t j = P.nb_list[s];
        double a, d;
        if (P.slack_unit && j >= P.ns) {  // A_j = e_k: no stream
            const int64_t k = j - P.ns;
            a = rs[k];
            d = ys[k] - P.c[j];
        } else {
            const dbl2* col = reinterpret_cast<const dbl2*>(P.A + j * L) + lane;
            dbl2 cur[U], nxt[U];
#pragma unroll
            for (int t = 0; t < U; ++t) cur[t] = t < nch ? ld2<SPX_NT_A>(col + 64 * t) : dbl2{0.0, 0.0};
            double a0 = 0.0, a1 = 0.0, d0 = 0.0, d1 = 0.0;
            for (int c0 = 0; c0 < nch; c0 += U) {
#pragma unroll
                for (int t = 0; t < U; ++t)
                    nxt[t] = c0 + U + t < nch ? ld2<SPX_NT_A>(col + 64 * (c0 + U + t)) : dbl2{0.0, 0.0};
#pragma unroll
                for (int t = 0; t < U; ++t) {
                    if (c0 + t < nch) {
                        const int k = 64 * (c0 + t) + lane;
                        const dbl2 r = rv[k], w = yv[k];
                        a0 = fma(cur[t].x, r.x, a0);
                        a1 = fma(cur[t].y, r.y, a1);
                        d0 = fma(cur[t].x, w.x, d0);
                        d1 = fma(cur[t].y, w.y, d1);
                    }
                }
#pragma unroll
                for (int t = 0; t < U; ++t) cur[t] = nxt[t];
            }
            a = a0 + a1;
            d = d0 + d1;
            wave_sum2(a, d);
            d -= P.c[j];
        }
        if (a < -D.piv_tol) {
            const double key = (d > 0.0 ? d : 0.0) / (-a);
            if (argmin_better(key, j, bkey, bidx)) {
                bkey = key;
                bidx = j;
                ba = a;
                bd = d;
            }
        }
    }
    if (lane == 0) s_red[wave] = DualPartial{bkey, bidx, ba, bd};
    __syncthreads();
    if (tid == 0) D.parts[blockIdx.x] = merge_waves<WAVES>(s_red);  // read after the kernel boundary (k_dual_update)
}

// ---------------------------------------------------------------------------
// Entering column, FTRAN fused with the pending rank-1 update of B^-1
// ---------------------------------------------------------------------------
// One row per wave.  Row i of S is read once, becomes S[i] + E_i r' (the
// pending pivot it-1; r' from rbuf), is written back in place and dotted with
// A_p: alpha_i into alpha[(it + 1) & 1].  After the launch S is B^-1 before
// pivot it, and (q, alpha_q, alpha) is the new pending pivot once k_dual_step
// commits it.
template <bool XL>
__global__ __launch_bounds__(DUAL_BLOCK) void k_dual_update(Params P, DualArgs D) {
    constexpr int WAVES = DUAL_WAVES, U = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    __shared__ DualPartial s_red[WAVES];
    __shared__ StepState Sv;
    DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // one reader per workgroup: workgroup 0 may store ST_INFEASIBLE below while
    // other workgroups start, and every wave of a workgroup must take the same exit
    if (tid == 0) {
        Sv.status = st->status;
        Sv.it = st->iter;
        Sv.limit = st->limit;
        Sv.qprev = st->q;
        Sv.aqprev = st->aq;
    }
    __syncthreads();
    const int64_t it = Sv.it, qp = Sv.qprev;
    const double aqp = Sv.aqprev;
    if (Sv.status != ST_RUNNING || it >= Sv.limit) return;

    // the ratio test's grid step: every workgroup merges the same partials
    DualPartial w{INFINITY, INT64_MAX, 0.0, 0.0};
    for (int g = tid; g < D.price_grid; g += DUAL_BLOCK) {
        const DualPartial v = D.parts[g];
        if (argmin_better(v.key, v.idx, w.key, w.idx)) w = v;
    }
    wave_argmin4(w);
    if (lane == 0) s_red[wave] = w;
    __syncthreads();
    const DualPartial t = merge_waves<WAVES>(s_red);
    if (t.idx == INT64_MAX) {  // no a_j < -piv_tol in a row with x_b < 0: primal infeasible
        if (blockIdx.x == 0 && tid == 0) st->status = ST_INFEASIBLE;
        return;
    }
    const int64_t p = t.idx;
    if (blockIdx.x == 0 && tid == 0) {
        D.rec->p = p;
        D.rec->d_p = t.d;
        D.rec->fresh = 1;
    }

    const int64_t m = P.m, L = P.L, L2 = L >> 1;
    const int nch = (int)(L2 >> 6);
    const bool pend = it > 0 && qp >= 0;
    const dbl2* rp = reinterpret_cast<const dbl2*>(pend ? P.rbuf : P.zeros);
    const dbl2* ap = reinterpret_cast<const dbl2*>(P.A + p * L);
    if constexpr (XL) {
        dbl2* d = reinterpret_cast<dbl2*>(dsm);
        for (int64_t k = tid; k < L2; k += DUAL_BLOCK) {
            d[k] = rp[k];
            d[L2 + k] = ap[k];
        }
        __syncthreads();
    }
    const dbl2* xr = XL ? reinterpret_cast<const dbl2*>(dsm) : rp;
    const dbl2* xa = XL ? reinterpret_cast<const dbl2*>(dsm) + L2 : ap;

    const int64_t i = (int64_t)blockIdx.x * WAVES + wave;
    if (i >= m) return;  // (no barrier below)
    const double* a_prev = (it & 1) ? P.alpha1 : P.alpha0;
    double* a_new = (it & 1) ? P.alpha0 : P.alpha1;
    const double ei = pend ? eta_entry(a_prev[i], i, qp, aqp) : 0.0;
    dbl2* row = reinterpret_cast<dbl2*>(P.B0 + i * L) + lane;
    dbl2 cur[U], nxt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = u < nch ? ld2<SPX_NT_BLOAD>(row + 64 * u) : dbl2{0.0, 0.0};
    double acc0 = 0.0, acc1 = 0.0;
    for (int c0 = 0; c0 < nch; c0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u)
            nxt[u] = c0 + U + u < nch ? ld2<SPX_NT_BLOAD>(row + 64 * (c0 + U + u)) : dbl2{0.0, 0.0};
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c0 + u < nch) {
                const int k = 64 * (c0 + u) + lane;
                const dbl2 r = xr[k], a = xa[k];
                dbl2 nv;
                nv.x = fma(ei, r.x, cur[u].x);
                nv.y = fma(ei, r.y, cur[u].y);
                st2<SPX_NT_BSTORE>(nv, row + 64 * (c0 + u));
                acc0 = fma(nv.x, a.x, acc0);
                acc1 = fma(nv.y, a.y, acc1);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
    const double alpha = wave_sum(acc0 + acc1);
    if (lane == 0) a_new[i] = alpha;
}

// ---------------------------------------------------------------------------
// Host-side launchers
// ---------------------------------------------------------------------------
namespace {

constexpr size_t DUAL_LDS_CAP = 150 * 1024;

template <typename K>
hipError_t set_lds(K kernel, size_t lds) {
    if (lds <= 65536) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds);
}

template <typename K>
hipError_t launch_timed(K kernel, int grid, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1, const Params& P,
                        const DualArgs& D) {
    if (e0 || e1) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(DUAL_BLOCK), (uint32_t)lds, s, e0, e1, 0, P, D);
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(DUAL_BLOCK), lds, s, P, D);
    return hipGetLastError();
}

}  // namespace

hipError_t dual_prepare(const Params& P, int cus, int price_grid_opt, bool global_y, DualCfg* cfg) {
    const size_t vec2 = (size_t)P.L * 16;  // two staged vectors
    cfg->price_lds = !global_y && vec2 <= DUAL_LDS_CAP;
    cfg->update_lds = vec2 <= DUAL_LDS_CAP;
    hipError_t e = hipSuccess;
    int per_cu = 0;
    if (cfg->price_lds) {
        e = set_lds(k_dual_price<true>, vec2);
        if (e == hipSuccess)
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_dual_price<true>, DUAL_BLOCK, vec2);
    } else {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_dual_price<false>, DUAL_BLOCK, 0);
    }
    if (e != hipSuccess) return e;
    if (cfg->update_lds) {
        e = set_lds(k_dual_update<true>, vec2);
        if (e != hipSuccess) return e;
    }
    if (per_cu < 1) per_cu = 1;
    const int64_t cols = P.n - P.m;  // the non-basic count never changes
    const int64_t want = (cols + DUAL_WAVES - 1) / DUAL_WAVES;
    const int64_t cap = (int64_t)cus * per_cu;
    int64_t g = want < cap ? want : cap;
    if (g < 1) g = 1;
    cfg->price_grid = price_grid_opt > 0 ? price_grid_opt : (int)g;
    cfg->update_grid = (int)((P.m + DUAL_WAVES - 1) / DUAL_WAVES);
    return hipSuccess;
}

hipError_t launch_dual_step(const Params& P, const DualArgs& D, bool finish_only, hipStream_t s) {
    hipLaunchKernelGGL(k_dual_step, dim3(1), dim3(1024), 0, s, P, D, finish_only ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_dual_price(const Params& P, const DualArgs& D, const DualCfg& c, hipStream_t s, hipEvent_t e0,
                             hipEvent_t e1) {
    if (c.price_lds) return launch_timed(k_dual_price<true>, c.price_grid, (size_t)P.L * 16, s, e0, e1, P, D);
    return launch_timed(k_dual_price<false>, c.price_grid, 0, s, e0, e1, P, D);
}

hipError_t launch_dual_update(const Params& P, const DualArgs& D, const DualCfg& c, hipStream_t s, hipEvent_t e0,
                              hipEvent_t e1) {
    if (c.update_lds) return launch_timed(k_dual_update<true>, c.update_grid, (size_t)P.L * 16, s, e0, e1, P, D);
    return launch_timed(k_dual_update<false>, c.update_grid, 0, s, e0, e1, P, D);
}

}  // namespace spx
