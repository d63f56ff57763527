// spx_pbox.hip — gfx950 kernels of the bounded primal simplex loop (spx_pbox.h).
#include "spx_pbox.h"

#include <hip/hip_ext.h>

#include "spx_common.h"

namespace spx {

namespace {

// the workgroup's merge of its waves' pricing candidates, with selects on scalars
template <int WAVES>
__device__ __forceinline__ PboxPartial merge_price(const PboxPartial* red) {
    double key = red[0].key, d = red[0].d;
    int64_t idx = red[0].idx;
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
        const double k2 = red[w].key, d2 = red[w].d;
        const int64_t j2 = red[w].idx;
        const bool t = argmin_better(k2, j2, key, idx);
        key = t ? k2 : key;
        idx = t ? j2 : idx;
        d = t ? d2 : d;
    }
    return PboxPartial{key, idx, d, 0.0};
}

// (value, index) argmin over the wave; every lane ends with the result (xor
// butterfly, argmin_better's order)
__device__ __forceinline__ void wave_argmin(double& v, int64_t& j) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double v2 = __shfl_xor(v, off, 64);
        const int64_t j2 = __shfl_xor(j, off, 64);
        const bool t = argmin_better(v2, j2, v, j);
        v = t ? v2 : v;
        j = t ? j2 : j;
    }
}

struct PboxSnap {  // the loop state, read once per workgroup by thread 0
    int64_t it, limit, qprev, p;
    double aqprev, d_p;
    int32_t status, y_buf, fresh, cnt;
};

}  // namespace

// ---------------------------------------------------------------------------
// Pricing (the hot kernel): one dot per streamed non-basic column
// ---------------------------------------------------------------------------
// k_dual_price's stream with one operand: one wave per column, grid-stride over
// nb_list.  A column is L/2 dbl2 in chunks of 64 lanes; U chunks are in flight
// per wave while the previous U are multiplied with y (double-buffered
// registers), non-temporal as k_price's A stream.  Per lane the chunks are
// accumulated in ascending order into two partial sums, then one butterfly: a
// column's d_j does not depend on the grid or on which wave prices it.  sigma_j
// is one wave-uniform flag read per column, ahead of its stream.
template <bool LDS>
__global__ __launch_bounds__(PBOX_BLOCK) void k_pbox_price(Params P, PboxArgs D) {
    constexpr int WAVES = PBOX_WAVES, U = 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    __shared__ PboxPartial s_red[WAVES];
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
    const dbl2* y_g = reinterpret_cast<const dbl2*>(y_buf ? P.y1 : P.y0);
    if constexpr (LDS) {
        dbl2* d = reinterpret_cast<dbl2*>(dsm);
        for (int64_t k = tid; k < L2; k += PBOX_BLOCK) d[k] = y_g[k];
        __syncthreads();
    }
    const dbl2* yv = LDS ? reinterpret_cast<const dbl2*>(dsm) : y_g;
    const double* ys = reinterpret_cast<const double*>(yv);

    double bkey = INFINITY, bd = 0.0;
    int64_t bidx = INT64_MAX;
    const int nwv = (int)gridDim.x * WAVES;
    for (int s = (int)blockIdx.x * WAVES + wave; s < cnt; s += nwv) {
        const int64_t j = P.nb_list[s];
        const int up = D.at_upper[j];
        double d;
        if (P.slack_unit && j >= P.ns) {  // A_j = e_k: no stream
            d = ys[j - P.ns] - P.c[j];
        } else {
            const dbl2* col = reinterpret_cast<const dbl2*>(P.A + j * L) + lane;
            dbl2 cur[U], nxt[U];
#pragma unroll
            for (int t = 0; t < U; ++t) cur[t] = t < nch ? ld2<SPX_NT_A>(col + 64 * t) : dbl2{0.0, 0.0};
            double d0 = 0.0, d1 = 0.0;
            for (int c0 = 0; c0 < nch; c0 += U) {
#pragma unroll
                for (int t = 0; t < U; ++t)
                    nxt[t] = c0 + U + t < nch ? ld2<SPX_NT_A>(col + 64 * (c0 + U + t)) : dbl2{0.0, 0.0};
#pragma unroll
                for (int t = 0; t < U; ++t) {
                    if (c0 + t < nch) {
                        const dbl2 w = yv[64 * (c0 + t) + lane];
                        d0 = fma(cur[t].x, w.x, d0);
                        d1 = fma(cur[t].y, w.y, d1);
                    }
                }
#pragma unroll
                for (int t = 0; t < U; ++t) cur[t] = nxt[t];
            }
            d = wave_sum(d0 + d1) - P.c[j];
        }
        const double key = up ? -d : d;  // sigma_j d_j (a sign flip: exact)
        if (key < -P.eps && argmin_better(key, j, bkey, bidx)) {
            bkey = key;
            bidx = j;
            bd = d;
        }
    }
    if (lane == 0) s_red[wave] = PboxPartial{bkey, bidx, bd, 0.0};
    __syncthreads();
    if (tid == 0) D.parts[blockIdx.x] = merge_price<WAVES>(s_red);  // read after the kernel boundary (k_pbox_update)
}

// ---------------------------------------------------------------------------
// Entering column, FTRAN fused with the pending rank-1 update, ratio entries
// ---------------------------------------------------------------------------
// One row per wave, k_dual_update's stream.  Row i of S is read once, becomes
// S[i] + E_i r' (the pending pivot; r' from rbuf), is written back in place and
// dotted with A_p: alpha_i into alpha[(it + 1) & 1].  After the launch S is the
// true B^-1.  x_b[i] and ub_B[i] are requested ahead of the stream; with ahat_i
// = sigma_p alpha_i the row's ratio-test entry is max(x_b, 0) / ahat_i (ahat_i >
// piv_tol: to its lower bound) or max(ub_B - x_b, 0) / -ahat_i (ahat_i <
// -piv_tol, finite ub_B: to its upper bound), keyed (t, 2 i + side) so that the
// first row wins ties through every reduction.
template <bool XL>
__global__ __launch_bounds__(PBOX_BLOCK) void k_pbox_update(Params P, PboxArgs D) {
    constexpr int WAVES = PBOX_WAVES, U = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    __shared__ PboxPartial s_red[WAVES];
    __shared__ ArgMinEntry s_rat[WAVES];
    __shared__ PboxSnap Sv;
    DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // one reader per workgroup: workgroup 0 may store ST_OPTIMAL below while
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

    // pricing's grid step: every workgroup merges the same partials
    double wk = INFINITY, wd = 0.0;
    int64_t wj = INT64_MAX;
    for (int g = tid; g < D.price_grid; g += PBOX_BLOCK) {
        const PboxPartial v = D.parts[g];
        if (argmin_better(v.key, v.idx, wk, wj)) {
            wk = v.key;
            wj = v.idx;
            wd = v.d;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double k2 = __shfl_xor(wk, off, 64);
        const int64_t j2 = __shfl_xor(wj, off, 64);
        const double d2 = __shfl_xor(wd, off, 64);
        const bool t = argmin_better(k2, j2, wk, wj);
        wk = t ? k2 : wk;
        wj = t ? j2 : wj;
        wd = t ? d2 : wd;
    }
    if (lane == 0) s_red[wave] = PboxPartial{wk, wj, wd, 0.0};
    __syncthreads();
    const PboxPartial t = merge_price<WAVES>(s_red);
    if (t.idx == INT64_MAX) {  // no sigma_j d_j < -eps: optimum
        if (blockIdx.x == 0 && tid == 0) st->status = ST_OPTIMAL;
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
        for (int64_t k = tid; k < L2; k += PBOX_BLOCK) {
            d[k] = rp[k];
            d[L2 + k] = ap[k];
        }
        __syncthreads();
    }
    const dbl2* xr = XL ? reinterpret_cast<const dbl2*>(dsm) : rp;
    const dbl2* xa = XL ? reinterpret_cast<const dbl2*>(dsm) + L2 : ap;

    const int64_t i = (int64_t)blockIdx.x * WAVES + wave;
    double rt = INFINITY;
    int64_t ri = INT64_MAX;
    if (i < m) {  // (wave-uniform; the barrier below is outside)
        const double sg = D.at_upper[p] ? -1.0 : 1.0;
        const double xi = P.x_b[i], ubi = D.ub_B[i];
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
        const double ah = sg * alpha;  // (a sign flip: exact)
        if (ah > D.piv_tol) {
            rt = (xi > 0.0 ? xi : 0.0) / ah;
            ri = 2 * i;
        } else if (ah < -D.piv_tol && ubi < INFINITY) {
            const double gap = ubi - xi;
            rt = (gap > 0.0 ? gap : 0.0) / (-ah);
            ri = 2 * i + 1;
        }
    }
    if (lane == 0) s_rat[wave] = ArgMinEntry{rt, ri};
    __syncthreads();
    if (tid == 0) {
        ArgMinEntry b = s_rat[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            const ArgMinEntry v = s_rat[w];
            const bool tk = argmin_better(v.val, v.idx, b.val, b.idx);
            b.val = tk ? v.val : b.val;
            b.idx = tk ? v.idx : b.idx;
        }
        D.rparts[blockIdx.x] = b;  // read after the kernel boundary (k_pbox_step)
    }
}

// ---------------------------------------------------------------------------
// Ratio-test merge, decision and commit (one workgroup)
// ---------------------------------------------------------------------------
// alpha = B^-1 A_p is in alpha[(it + 1) & 1] and S is the true B^-1
// (k_pbox_update).  A pivot makes (q, alpha_q, alpha[(it + 1) & 1]) the pending
// one with iter = it + 1 and stages rho = S[q] into rbuf while y takes it.  A
// flip or an unbounded column leaves iter alone and nothing pending: st->q = 0,
// st->aq = 1, alpha[it & 1] = e_0 (a reinversion's state: every eta entry 0).
__global__ __launch_bounds__(1024) void k_pbox_step(Params P, PboxArgs D) {
    constexpr int BLOCK = 1024, WAVES = BLOCK / 64, CH = 4;
    DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = P.m, L = P.L;
    __shared__ PboxSnap S;
    __shared__ ArgMinEntry s_red[WAVES];
    __shared__ ArgMinEntry s_win;
    __shared__ double s_up;   // u_p
    __shared__ int32_t s_at;  // at_upper[p], read once: the commit's thread 0 / bookkeeping lane rewrites it
    if (tid == 0) {
        S.it = st->iter;
        S.limit = st->limit;
        S.status = st->status;
        S.y_buf = st->y_buf;
        S.cnt = st->nb_count;
        S.fresh = D.rec->fresh;
        S.p = D.rec->p;
        S.d_p = D.rec->d_p;
    }
    __syncthreads();
    const int64_t it = S.it;
    if (S.status != ST_RUNNING || it >= S.limit || !S.fresh) return;

    // the ratio test's grid step
    double bv = INFINITY;
    int64_t bi = INT64_MAX;
    for (int g = tid; g < D.update_grid; g += BLOCK) {
        const ArgMinEntry v = D.rparts[g];
        if (argmin_better(v.val, v.idx, bv, bi)) {
            bv = v.val;
            bi = v.idx;
        }
    }
    wave_argmin(bv, bi);
    if (lane == 0) s_red[wave] = ArgMinEntry{bv, bi};
    __syncthreads();
    if (tid == 0) {
        ArgMinEntry t = s_red[0];
        for (int w = 1; w < WAVES; ++w)
            if (argmin_better(s_red[w].val, s_red[w].idx, t.val, t.idx)) t = s_red[w];
        s_win = t;
        s_up = D.ub[S.p];
        s_at = D.at_upper[S.p];
    }
    __syncthreads();
    const double tq = s_win.val;
    const bool none = s_win.idx == INT64_MAX;
    const int64_t q = none ? 0 : (s_win.idx >> 1);
    const int side = none ? 0 : (int)(s_win.idx & 1);  // 1: the row leaves to its upper bound
    const int64_t p = S.p;
    const double u_p = s_up;
    const int up_p = s_at;
    const double sg = up_p ? -1.0 : 1.0;
    const double* al = ((it + 1) & 1) ? P.alpha1 : P.alpha0;
    double* a_cur = (it & 1) ? P.alpha1 : P.alpha0;
    const bool flip = u_p < INFINITY && (none || u_p <= tq);

    if (flip || none) {
        // no pivot: S has the pending pivot applied and iter stays, so nothing is pending
        if (flip) {
            const double dx = up_p ? -u_p : u_p;  // the column's move
            const double* Ap = P.A + p * L;
            for (int64_t i = tid; i < m; i += BLOCK) {
                P.x_b[i] = fma(-u_p, sg * al[i], P.x_b[i]);
                D.b_eff[i] = fma(-dx, Ap[i], D.b_eff[i]);
            }
        }
        for (int64_t i = tid; i < L; i += BLOCK) a_cur[i] = (i == 0) ? 1.0 : 0.0;
        if (tid == 0) {
            if (flip) {
                D.at_upper[p] = up_p ? 0 : 1;
                D.rec->flips += 1;
            } else {
                st->status = ST_UNBOUNDED;
            }
            st->q = 0;
            st->aq = 1.0;
            st->p = p;
            st->min_e = S.d_p;
            D.rec->fresh = 0;
        }
        return;
    }

    // pivot it
    double* y = S.y_buf ? P.y1 : P.y0;
    const double aq = al[q];
    const double theta = tq, sy = -(S.d_p / aq);
    const double x_off = up_p ? u_p : 0.0;  // where the entering column starts from
    const bool book = tid == BLOCK - 64;    // the last wave's lane 0
    int64_t leave = -1;
    double c_p = 0.0;
    int kp = -1, last = -1;
    if (book) {
        leave = P.b_ixs[q];
        c_p = P.c[p];
        kp = P.nb_pos[p];
        last = P.nb_list[S.cnt - 1];
    }
    const double* Sq = P.B0 + q * L;  // rho: row q of B^-1 before this pivot
    for (int64_t i0 = tid; i0 < L; i0 += (int64_t)CH * BLOCK) {
        double xv[CH], av[CH], yv[CH], rv[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t i = i0 + (int64_t)u * BLOCK;
            xv[u] = i < m ? P.x_b[i] : 0.0;
            av[u] = i < m ? al[i] : 0.0;
            yv[u] = i < L ? y[i] : 0.0;
            rv[u] = i < L ? Sq[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t i = i0 + (int64_t)u * BLOCK;
            if (i < m) P.x_b[i] = (i == q) ? x_off + sg * theta : fma(-theta, sg * av[u], xv[u]);
            if (i < L) {
                y[i] = fma(sy, rv[u], yv[u]);
                P.rbuf[i] = rv[u];  // the pending pivot's row, before the next update overwrites it
            }
        }
    }
    if (book) {
        P.c_B[q] = c_p;
        P.b_ixs[q] = p;
        D.ub_B[q] = u_p;
        D.at_upper[p] = 0;
        D.at_upper[leave] = (int8_t)side;
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
        if (side) D.rec->to_upper += 1;
    }
}

// rbuf = row st->q of S where a pivot is pending (one workgroup)
__global__ __launch_bounds__(1024) void k_pbox_stage(Params P) {
    const DevState* st = P.st;
    const int64_t it = st->iter, q = st->q;
    if (it <= 0 || q < 0 || q >= P.m) return;
    const double* Sq = P.B0 + q * P.L;
    for (int64_t k = threadIdx.x; k < P.L; k += 1024) P.rbuf[k] = Sq[k];
}

// ---------------------------------------------------------------------------
// Phase 1 (spx_pbox.h)
// ---------------------------------------------------------------------------
namespace {

// a row's class from its value and its basic column's bound: +1 below, -1 above, 0 feasible
__device__ __forceinline__ double row_class(double x, double ub, double tol) {
    return x < -tol ? 1.0 : (x > ub + tol ? -1.0 : 0.0);
}

struct VtbSnap {
    int64_t it, limit, q;
    double aq;
    int32_t status, ninf, stale, y_buf;
};

// what a vtb launch has to do: 0 nothing, 1 yp = w B^-1, 2 y = c_B B^-1
__device__ __forceinline__ int vtb_mode(const VtbSnap& s, int force) {
    if (force) return s.stale ? 2 : 0;
    if (s.status != ST_RUNNING || s.it >= s.limit) return 0;
    return s.ninf > 0 ? 1 : (s.stale ? 2 : 0);
}

}  // namespace

// out = v B^-1 for v = w (phase 1) or c_B (the switch, a readback), as per-row-
// block partial vectors.  Workgroup (x, y): row block y (PBOX_VTB_ROWS rows of
// S), wave k the 1 KiB column chunk PBOX_VTB_WAVES x + k; a lane owns one dbl2
// of the chunk.  The rows with v'_i != 0 are listed in LDS by one ballot
// (ascending), then streamed U at a time, double-buffered, non-temporal as the
// update stream; one accumulator pair per lane in list order, so the bits
// depend on m alone.
__global__ __launch_bounds__(PBOX_VTB_BLOCK) void k_pbox_vtb(Params P, Pbox1Args X) {
    constexpr int WAVES = PBOX_VTB_WAVES, U = 8;
    __shared__ double s_v[PBOX_VTB_ROWS];
    __shared__ int32_t s_row[PBOX_VTB_ROWS];
    __shared__ int32_t s_n;
    __shared__ double s_dot[WAVES];
    __shared__ VtbSnap Sv;
    const DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid == 0) {
        Sv.status = st->status;
        Sv.it = st->iter;
        Sv.limit = st->limit;
        Sv.q = st->q;
        Sv.aq = st->aq;
        Sv.ninf = X.ph->ninf;
        Sv.stale = X.ph->y_stale;
    }
    __syncthreads();
    const int mode = vtb_mode(Sv, X.force);
    if (mode == 0) return;
    const double* v = mode == 1 ? X.w : P.c_B;
    const int64_t m = P.m, L = P.L, L2 = L >> 1;
    const int nch = (int)(L2 >> 6);
    const int64_t it = Sv.it, q = Sv.q;
    const bool pend = it > 0 && q >= 0;
    const int64_t r0 = (int64_t)blockIdx.y * PBOX_VTB_ROWS;
    double vq_add = 0.0;
    if (pend && q >= r0 && q < r0 + PBOX_VTB_ROWS) {  // (workgroup-uniform) v'_q - v_q = sum_i v_i E_i
        // E_i = -alpha_i / alpha_q (i != q), E_q = 1 / alpha_q - 1: one division, after the sum
        const double* a_prev = (it & 1) ? P.alpha1 : P.alpha0;
        const double aq = Sv.aq;
        double s = 0.0;
#pragma unroll 4
        for (int64_t i = tid; i < m; i += PBOX_VTB_BLOCK) s = fma(v[i], i != q ? a_prev[i] : 0.0, s);
        s = wave_sum(s);
        if (lane == 0) s_dot[wave] = s;
        __syncthreads();
        double t = s_dot[0];
#pragma unroll
        for (int k = 1; k < WAVES; ++k) t += s_dot[k];
        vq_add = fma(v[q], 1.0 / aq - 1.0, -(t / aq));
    }
    if (wave == 0) {
        const int64_t i = r0 + lane;
        double vi = i < m ? v[i] : 0.0;
        if (pend && i == q) vi += vq_add;
        const unsigned long long mask = __ballot(vi != 0.0);
        const int pos = __popcll(mask & ((1ull << lane) - 1ull));
        if (vi != 0.0) {
            s_v[pos] = vi;
            s_row[pos] = lane;
        }
        if (lane == 0) s_n = __popcll(mask);
    }
    __syncthreads();
    const int c = (int)blockIdx.x * WAVES + wave;
    if (c >= nch) return;
    const int n = s_n;
    const dbl2* base = reinterpret_cast<const dbl2*>(P.B0 + r0 * L) + 64 * c + lane;
    dbl2 acc{0.0, 0.0};
    dbl2 cur[U], nxt[U];
#pragma unroll
    for (int t = 0; t < U; ++t) cur[t] = t < n ? ld2<SPX_NT_BLOAD>(base + (int64_t)s_row[t] * L2) : dbl2{0.0, 0.0};
    for (int k0 = 0; k0 < n; k0 += U) {
#pragma unroll
        for (int t = 0; t < U; ++t)
            nxt[t] = k0 + U + t < n ? ld2<SPX_NT_BLOAD>(base + (int64_t)s_row[k0 + U + t] * L2) : dbl2{0.0, 0.0};
#pragma unroll
        for (int t = 0; t < U; ++t) {
            if (k0 + t < n) {
                const double vv = s_v[k0 + t];
                acc.x = fma(vv, cur[t].x, acc.x);
                acc.y = fma(vv, cur[t].y, acc.y);
            }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) cur[t] = nxt[t];
    }
    reinterpret_cast<dbl2*>(X.vparts + (int64_t)blockIdx.y * L)[64 * c + lane] = acc;  // read after the kernel boundary
}

// the row blocks' partial vectors added in a fixed order, into yp (phase 1) or
// y: a workgroup owns one 1 KiB chunk, wave g the g-th quarter of the row blocks
// (ascending), and lane-wise ((s0 + s1) + s2) + s3 closes it -- a function of m
__global__ __launch_bounds__(PBOX_VTB_BLOCK) void k_pbox_vtb_sum(Params P, Pbox1Args X) {
    constexpr int WAVES = PBOX_VTB_WAVES;
    __shared__ dbl2 s_acc[WAVES][64];
    __shared__ VtbSnap Sv;
    const DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid == 0) {
        Sv.status = st->status;
        Sv.it = st->iter;
        Sv.limit = st->limit;
        Sv.ninf = X.ph->ninf;
        Sv.stale = X.ph->y_stale;
        Sv.y_buf = st->y_buf;
    }
    __syncthreads();
    const int mode = vtb_mode(Sv, X.force);
    if (mode == 0) return;
    const int64_t L2 = P.L >> 1;
    const int64_t k = (int64_t)blockIdx.x * 64 + lane;  // (L2 is a multiple of 64: the grid is L2 / 64)
    const int nb = X.vtb_blocks, per = (nb + WAVES - 1) / WAVES;
    const int b0 = wave * per, b1 = b0 + per < nb ? b0 + per : nb;
    const dbl2* parts = reinterpret_cast<const dbl2*>(X.vparts) + k;
    dbl2 acc{0.0, 0.0};
#pragma unroll 4
    for (int b = b0; b < b1; ++b) {
        const dbl2 t = parts[(int64_t)b * L2];
        acc.x += t.x;
        acc.y += t.y;
    }
    s_acc[wave][lane] = acc;
    __syncthreads();
    if (wave == 0) {
        dbl2 r = s_acc[0][lane];
#pragma unroll
        for (int g = 1; g < WAVES; ++g) {
            r.x += s_acc[g][lane].x;
            r.y += s_acc[g][lane].y;
        }
        double* out = mode == 1 ? X.yp : (Sv.y_buf ? P.y1 : P.y0);
        reinterpret_cast<dbl2*>(out)[k] = r;
    }
}

// k_pbox_price with the phase read from the device: phase 1 prices with yp and no c_j
template <bool LDS>
__global__ __launch_bounds__(PBOX_BLOCK) void k_pbox_price1(Params P, PboxArgs D, Pbox1Args X) {
    constexpr int WAVES = PBOX_WAVES, U = 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    __shared__ PboxPartial s_red[WAVES];
    const DevState* st = P.st;
    const int32_t status = st->status;
    const int32_t cnt = st->nb_count;
    const int32_t y_buf = st->y_buf;
    const int64_t iter = st->iter, limit = st->limit;
    const bool ph1 = X.ph->ninf > 0;
    if (status != ST_RUNNING || iter >= limit) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t L = P.L, L2 = L >> 1;
    const int nch = (int)(L2 >> 6);
    const dbl2* y_g = reinterpret_cast<const dbl2*>(ph1 ? X.yp : (y_buf ? P.y1 : P.y0));
    if constexpr (LDS) {
        dbl2* d = reinterpret_cast<dbl2*>(dsm);
        for (int64_t k = tid; k < L2; k += PBOX_BLOCK) d[k] = y_g[k];
        __syncthreads();
    }
    const dbl2* yv = LDS ? reinterpret_cast<const dbl2*>(dsm) : y_g;
    const double* ys = reinterpret_cast<const double*>(yv);

    double bkey = INFINITY, bd = 0.0;
    int64_t bidx = INT64_MAX;
    const int nwv = (int)gridDim.x * WAVES;
    for (int s = (int)blockIdx.x * WAVES + wave; s < cnt; s += nwv) {
        const int64_t j = P.nb_list[s];
        const int up = D.at_upper[j];
        const double cj = ph1 ? 0.0 : P.c[j];  // (x - 0.0 = x: exact)
        double d;
        if (P.slack_unit && j >= P.ns) {
            d = ys[j - P.ns] - cj;
        } else {
            const dbl2* col = reinterpret_cast<const dbl2*>(P.A + j * L) + lane;
            dbl2 cur[U], nxt[U];
#pragma unroll
            for (int t = 0; t < U; ++t) cur[t] = t < nch ? ld2<SPX_NT_A>(col + 64 * t) : dbl2{0.0, 0.0};
            double d0 = 0.0, d1 = 0.0;
            for (int c0 = 0; c0 < nch; c0 += U) {
#pragma unroll
                for (int t = 0; t < U; ++t)
                    nxt[t] = c0 + U + t < nch ? ld2<SPX_NT_A>(col + 64 * (c0 + U + t)) : dbl2{0.0, 0.0};
#pragma unroll
                for (int t = 0; t < U; ++t) {
                    if (c0 + t < nch) {
                        const dbl2 w = yv[64 * (c0 + t) + lane];
                        d0 = fma(cur[t].x, w.x, d0);
                        d1 = fma(cur[t].y, w.y, d1);
                    }
                }
#pragma unroll
                for (int t = 0; t < U; ++t) cur[t] = nxt[t];
            }
            d = wave_sum(d0 + d1) - cj;
        }
        const double key = up ? -d : d;
        if (key < -P.eps && argmin_better(key, j, bkey, bidx)) {
            bkey = key;
            bidx = j;
            bd = d;
        }
    }
    if (lane == 0) s_red[wave] = PboxPartial{bkey, bidx, bd, 0.0};
    __syncthreads();
    if (tid == 0) D.parts[blockIdx.x] = merge_price<WAVES>(s_red);
}

// k_pbox_update with the phase read from the device: in phase 1 no candidate is
// ST_INFEASIBLE and row i's ratio entry depends on its class w[i], requested
// ahead of the stream beside x_b[i] and ub_B[i]
template <bool XL>
__global__ __launch_bounds__(PBOX_BLOCK) void k_pbox_update1(Params P, PboxArgs D, Pbox1Args X) {
    constexpr int WAVES = PBOX_WAVES, U = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    __shared__ PboxPartial s_red[WAVES];
    __shared__ ArgMinEntry s_rat[WAVES];
    __shared__ PboxSnap Sv;
    __shared__ int32_t s_ninf;
    DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid == 0) {  // one reader per workgroup (k_pbox_update)
        Sv.status = st->status;
        Sv.it = st->iter;
        Sv.limit = st->limit;
        Sv.qprev = st->q;
        Sv.aqprev = st->aq;
        s_ninf = X.ph->ninf;
    }
    __syncthreads();
    const int64_t it = Sv.it, qp = Sv.qprev;
    const double aqp = Sv.aqprev;
    const bool ph1 = s_ninf > 0;
    if (Sv.status != ST_RUNNING || it >= Sv.limit) return;

    double wk = INFINITY, wd = 0.0;
    int64_t wj = INT64_MAX;
    for (int g = tid; g < D.price_grid; g += PBOX_BLOCK) {
        const PboxPartial v = D.parts[g];
        if (argmin_better(v.key, v.idx, wk, wj)) {
            wk = v.key;
            wj = v.idx;
            wd = v.d;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double k2 = __shfl_xor(wk, off, 64);
        const int64_t j2 = __shfl_xor(wj, off, 64);
        const double d2 = __shfl_xor(wd, off, 64);
        const bool t = argmin_better(k2, j2, wk, wj);
        wk = t ? k2 : wk;
        wj = t ? j2 : wj;
        wd = t ? d2 : wd;
    }
    if (lane == 0) s_red[wave] = PboxPartial{wk, wj, wd, 0.0};
    __syncthreads();
    const PboxPartial t = merge_price<WAVES>(s_red);
    if (t.idx == INT64_MAX) {  // phase 1: the violation cannot decrease; phase 2: optimum
        if (blockIdx.x == 0 && tid == 0) st->status = ph1 ? ST_INFEASIBLE : ST_OPTIMAL;
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
        for (int64_t k = tid; k < L2; k += PBOX_BLOCK) {
            d[k] = rp[k];
            d[L2 + k] = ap[k];
        }
        __syncthreads();
    }
    const dbl2* xr = XL ? reinterpret_cast<const dbl2*>(dsm) : rp;
    const dbl2* xa = XL ? reinterpret_cast<const dbl2*>(dsm) + L2 : ap;

    const int64_t i = (int64_t)blockIdx.x * WAVES + wave;
    double rt = INFINITY;
    int64_t ri = INT64_MAX;
    if (i < m) {
        const double sg = D.at_upper[p] ? -1.0 : 1.0;
        const double xi = P.x_b[i], ubi = D.ub_B[i];
        const double wi = ph1 ? X.w[i] : 0.0;
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
        const double ah = sg * alpha;
        if (wi == 0.0) {  // a feasible row: phase 2's entry
            if (ah > D.piv_tol) {
                rt = (xi > 0.0 ? xi : 0.0) / ah;
                ri = 2 * i;
            } else if (ah < -D.piv_tol && ubi < INFINITY) {
                const double gap = ubi - xi;
                rt = (gap > 0.0 ? gap : 0.0) / (-ah);
                ri = 2 * i + 1;
            }
        } else if (wi > 0.0) {  // below: blocks where it rises to 0
            if (ah < -D.piv_tol) {
                rt = xi / ah;
                ri = 2 * i;
            }
        } else {  // above: blocks where it falls to its bound
            if (ah > D.piv_tol) {
                rt = (xi - ubi) / ah;
                ri = 2 * i + 1;
            }
        }
    }
    if (lane == 0) s_rat[wave] = ArgMinEntry{rt, ri};
    __syncthreads();
    if (tid == 0) {
        ArgMinEntry b = s_rat[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            const ArgMinEntry v = s_rat[w];
            const bool tk = argmin_better(v.val, v.idx, b.val, b.idx);
            b.val = tk ? v.val : b.val;
            b.idx = tk ? v.idx : b.idx;
        }
        D.rparts[blockIdx.x] = b;
    }
}

// k_pbox_step with the phase read from the device.  A phase-1 commit leaves y
// alone (y_stale = 1 after a pivot), classifies every row from the x_b it has
// just written (w, ninf) and bumps the phase-1 counters; no row and no bound is
// ST_BREAKDOWN.  The first phase-2 pass after the switch clears y_stale:
// k_pbox_vtb rebuilt y ahead of this pass's pricing.
__global__ __launch_bounds__(1024) void k_pbox_step1(Params P, PboxArgs D, Pbox1Args X) {
    constexpr int BLOCK = 1024, WAVES = BLOCK / 64, CH = 4;
    DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = P.m, L = P.L;
    __shared__ PboxSnap S;
    __shared__ ArgMinEntry s_red[WAVES];
    __shared__ ArgMinEntry s_win;
    __shared__ double s_up;
    __shared__ int32_t s_at;
    __shared__ int32_t s_ninf, s_stale, s_cnt;
    if (tid == 0) {
        S.it = st->iter;
        S.limit = st->limit;
        S.status = st->status;
        S.y_buf = st->y_buf;
        S.cnt = st->nb_count;
        S.fresh = D.rec->fresh;
        S.p = D.rec->p;
        S.d_p = D.rec->d_p;
        s_ninf = X.ph->ninf;
        s_stale = X.ph->y_stale;
        s_cnt = 0;
    }
    __syncthreads();
    const int64_t it = S.it;
    if (S.status != ST_RUNNING || it >= S.limit || !S.fresh) return;
    const bool ph1 = s_ninf > 0;
    const double ftol = X.feas_tol;

    double bv = INFINITY;
    int64_t bi = INT64_MAX;
    for (int g = tid; g < D.update_grid; g += BLOCK) {
        const ArgMinEntry v = D.rparts[g];
        if (argmin_better(v.val, v.idx, bv, bi)) {
            bv = v.val;
            bi = v.idx;
        }
    }
    wave_argmin(bv, bi);
    if (lane == 0) s_red[wave] = ArgMinEntry{bv, bi};
    __syncthreads();
    if (tid == 0) {
        ArgMinEntry t = s_red[0];
        for (int w = 1; w < WAVES; ++w)
            if (argmin_better(s_red[w].val, s_red[w].idx, t.val, t.idx)) t = s_red[w];
        s_win = t;
        s_up = D.ub[S.p];
        s_at = D.at_upper[S.p];
    }
    __syncthreads();
    const double tq = s_win.val;
    const bool none = s_win.idx == INT64_MAX;
    const int64_t q = none ? 0 : (s_win.idx >> 1);
    const int side = none ? 0 : (int)(s_win.idx & 1);
    const int64_t p = S.p;
    const double u_p = s_up;
    const int up_p = s_at;
    const double sg = up_p ? -1.0 : 1.0;
    const double* al = ((it + 1) & 1) ? P.alpha1 : P.alpha0;
    double* a_cur = (it & 1) ? P.alpha1 : P.alpha0;
    const bool flip = u_p < INFINITY && (none || u_p <= tq);

    if (flip || none) {
        if (flip) {
            const double dx = up_p ? -u_p : u_p;
            const double* Ap = P.A + p * L;
            int bad = 0;
            for (int64_t i = tid; i < m; i += BLOCK) {
                const double xn = fma(-u_p, sg * al[i], P.x_b[i]);
                P.x_b[i] = xn;
                D.b_eff[i] = fma(-dx, Ap[i], D.b_eff[i]);
                if (ph1) {
                    const double wv = row_class(xn, D.ub_B[i], ftol);
                    X.w[i] = wv;
                    bad += wv != 0.0;
                }
            }
            if (ph1 && bad) atomicAdd(&s_cnt, bad);  // (an integer count: order-free)
        }
        for (int64_t i = tid; i < L; i += BLOCK) a_cur[i] = (i == 0) ? 1.0 : 0.0;
        __syncthreads();
        if (tid == 0) {
            if (flip) {
                D.at_upper[p] = up_p ? 0 : 1;
                D.rec->flips += 1;
                if (ph1) {
                    X.ph->ninf = s_cnt;
                    X.ph->passes += 1;
                }
            } else {
                st->status = ph1 ? ST_BREAKDOWN : ST_UNBOUNDED;
            }
            if (!ph1 && s_stale) X.ph->y_stale = 0;
            st->q = 0;
            st->aq = 1.0;
            st->p = p;
            st->min_e = S.d_p;
            D.rec->fresh = 0;
        }
        return;
    }

    double* y = S.y_buf ? P.y1 : P.y0;
    const double aq = al[q];
    const double theta = tq, sy = -(S.d_p / aq);
    const double x_off = up_p ? u_p : 0.0;
    const bool book = tid == BLOCK - 64;
    int64_t leave = -1;
    double c_p = 0.0;
    int kp = -1, last = -1;
    if (book) {
        leave = P.b_ixs[q];
        c_p = P.c[p];
        kp = P.nb_pos[p];
        last = P.nb_list[S.cnt - 1];
    }
    const double* Sq = P.B0 + q * L;
    int bad = 0;
    for (int64_t i0 = tid; i0 < L; i0 += (int64_t)CH * BLOCK) {
        double xv[CH], av[CH], yv[CH], rv[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t i = i0 + (int64_t)u * BLOCK;
            xv[u] = i < m ? P.x_b[i] : 0.0;
            av[u] = i < m ? al[i] : 0.0;
            yv[u] = i < L ? y[i] : 0.0;
            rv[u] = i < L ? Sq[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t i = i0 + (int64_t)u * BLOCK;
            if (i < m) {
                const double xn = (i == q) ? x_off + sg * theta : fma(-theta, sg * av[u], xv[u]);
                P.x_b[i] = xn;
                if (ph1) {  // (row q's bound is the entering column's: the bookkeeping lane stores it below)
                    const double wv = row_class(xn, i == q ? u_p : D.ub_B[i], ftol);
                    X.w[i] = wv;
                    bad += wv != 0.0;
                }
            }
            if (i < L) {
                if (!ph1) y[i] = fma(sy, rv[u], yv[u]);
                P.rbuf[i] = rv[u];
            }
        }
    }
    if (ph1 && bad) atomicAdd(&s_cnt, bad);
    __syncthreads();
    if (book) {
        P.c_B[q] = c_p;
        P.b_ixs[q] = p;
        D.ub_B[q] = u_p;
        D.at_upper[p] = 0;
        D.at_upper[leave] = (int8_t)side;
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
        st->y_applied = it + 1;
        st->xb_applied = it + 1;
        st->p = p;
        st->q = q;
        st->min_e = S.d_p;
        st->iter = it + 1;
        record_pivot(P, it, p, q);
        D.rec->fresh = 0;
        if (side) D.rec->to_upper += 1;
        if (ph1) {
            X.ph->ninf = s_cnt;
            X.ph->passes += 1;
            X.ph->pivots += 1;
            X.ph->y_stale = 1;
        } else if (s_stale) {
            X.ph->y_stale = 0;
        }
    }
}

// w and ninf from x_b and ub_B (one workgroup): the entry check (ninf0 too) and after a reinversion
__global__ __launch_bounds__(1024) void k_pbox_classify(Params P, PboxArgs D, Pbox1Args X, int entry) {
    __shared__ int32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    int bad = 0;
    for (int64_t i = threadIdx.x; i < P.L; i += 1024) {
        const double wv = i < P.m ? row_class(P.x_b[i], D.ub_B[i], X.feas_tol) : 0.0;
        X.w[i] = wv;
        bad += wv != 0.0;
    }
    if (bad) atomicAdd(&s_cnt, bad);
    __syncthreads();
    if (threadIdx.x == 0) {
        X.ph->ninf = s_cnt;
        if (entry) X.ph->ninf0 = s_cnt;
    }
}

// ---------------------------------------------------------------------------
// Free columns (spx_pbox.h)
// ---------------------------------------------------------------------------
namespace {

// row_class with the basic column's lower bound (0, or -inf for a free column:
// such a row is never out of its bounds)
__device__ __forceinline__ double row_class_f(double x, double lb, double ub, double tol) {
    return x < lb - tol ? 1.0 : (x > ub + tol ? -1.0 : 0.0);
}

}  // namespace

// k_pbox_price1 with free columns: one more wave-uniform flag per column, read
// ahead of its stream beside at_upper; a free column's key is -|d_j|.  The dot
// is k_pbox_price's, chunk for chunk.
template <bool LDS>
__global__ __launch_bounds__(PBOX_BLOCK) void k_pbox_price_f(Params P, PboxArgs D, Pbox1Args X, PboxFreeArgs F) {
    constexpr int WAVES = PBOX_WAVES, U = 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    __shared__ PboxPartial s_red[WAVES];
    const DevState* st = P.st;
    const int32_t status = st->status;
    const int32_t cnt = st->nb_count;
    const int32_t y_buf = st->y_buf;
    const int64_t iter = st->iter, limit = st->limit;
    const bool ph1 = X.ph->ninf > 0;
    if (status != ST_RUNNING || iter >= limit) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t L = P.L, L2 = L >> 1;
    const int nch = (int)(L2 >> 6);
    const dbl2* y_g = reinterpret_cast<const dbl2*>(ph1 ? X.yp : (y_buf ? P.y1 : P.y0));
    if constexpr (LDS) {
        dbl2* d = reinterpret_cast<dbl2*>(dsm);
        for (int64_t k = tid; k < L2; k += PBOX_BLOCK) d[k] = y_g[k];
        __syncthreads();
    }
    const dbl2* yv = LDS ? reinterpret_cast<const dbl2*>(dsm) : y_g;
    const double* ys = reinterpret_cast<const double*>(yv);

    double bkey = INFINITY, bd = 0.0;
    int64_t bidx = INT64_MAX;
    const int nwv = (int)gridDim.x * WAVES;
    for (int s = (int)blockIdx.x * WAVES + wave; s < cnt; s += nwv) {
        const int64_t j = P.nb_list[s];
        const int up = D.at_upper[j];
        const int fr = F.is_free[j];
        const double cj = ph1 ? 0.0 : P.c[j];  // (x - 0.0 = x: exact)
        double d;
        if (P.slack_unit && j >= P.ns) {
            d = ys[j - P.ns] - cj;
        } else {
            const dbl2* col = reinterpret_cast<const dbl2*>(P.A + j * L) + lane;
            dbl2 cur[U], nxt[U];
#pragma unroll
            for (int t = 0; t < U; ++t) cur[t] = t < nch ? ld2<SPX_NT_A>(col + 64 * t) : dbl2{0.0, 0.0};
            double d0 = 0.0, d1 = 0.0;
            for (int c0 = 0; c0 < nch; c0 += U) {
#pragma unroll
                for (int t = 0; t < U; ++t)
                    nxt[t] = c0 + U + t < nch ? ld2<SPX_NT_A>(col + 64 * (c0 + U + t)) : dbl2{0.0, 0.0};
#pragma unroll
                for (int t = 0; t < U; ++t) {
                    if (c0 + t < nch) {
                        const dbl2 w = yv[64 * (c0 + t) + lane];
                        d0 = fma(cur[t].x, w.x, d0);
                        d1 = fma(cur[t].y, w.y, d1);
                    }
                }
#pragma unroll
                for (int t = 0; t < U; ++t) cur[t] = nxt[t];
            }
            d = wave_sum(d0 + d1) - cj;
        }
        const double key = fr ? -fabs(d) : (up ? -d : d);  // free: either direction improves
        if (key < -P.eps && argmin_better(key, j, bkey, bidx)) {
            bkey = key;
            bidx = j;
            bd = d;
        }
    }
    if (lane == 0) s_red[wave] = PboxPartial{bkey, bidx, bd, 0.0};
    __syncthreads();
    if (tid == 0) D.parts[blockIdx.x] = merge_price<WAVES>(s_red);
}

// k_pbox_update1 with free columns: sigma_p of a free entering column is the
// sign that improves (+1 for d_p < 0), and row i's basic column's lower bound
// lb_B[i] (0 or -inf) is requested ahead of the stream beside x_b[i], ub_B[i]
// and w[i]: a row whose basic column is free never blocks
template <bool XL>
__global__ __launch_bounds__(PBOX_BLOCK) void k_pbox_update_f(Params P, PboxArgs D, Pbox1Args X, PboxFreeArgs F) {
    constexpr int WAVES = PBOX_WAVES, U = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    __shared__ PboxPartial s_red[WAVES];
    __shared__ ArgMinEntry s_rat[WAVES];
    __shared__ PboxSnap Sv;
    __shared__ int32_t s_ninf;
    DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid == 0) {  // one reader per workgroup (k_pbox_update)
        Sv.status = st->status;
        Sv.it = st->iter;
        Sv.limit = st->limit;
        Sv.qprev = st->q;
        Sv.aqprev = st->aq;
        s_ninf = X.ph->ninf;
    }
    __syncthreads();
    const int64_t it = Sv.it, qp = Sv.qprev;
    const double aqp = Sv.aqprev;
    const bool ph1 = s_ninf > 0;
    if (Sv.status != ST_RUNNING || it >= Sv.limit) return;

    double wk = INFINITY, wd = 0.0;
    int64_t wj = INT64_MAX;
    for (int g = tid; g < D.price_grid; g += PBOX_BLOCK) {
        const PboxPartial v = D.parts[g];
        if (argmin_better(v.key, v.idx, wk, wj)) {
            wk = v.key;
            wj = v.idx;
            wd = v.d;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double k2 = __shfl_xor(wk, off, 64);
        const int64_t j2 = __shfl_xor(wj, off, 64);
        const double d2 = __shfl_xor(wd, off, 64);
        const bool t = argmin_better(k2, j2, wk, wj);
        wk = t ? k2 : wk;
        wj = t ? j2 : wj;
        wd = t ? d2 : wd;
    }
    if (lane == 0) s_red[wave] = PboxPartial{wk, wj, wd, 0.0};
    __syncthreads();
    const PboxPartial t = merge_price<WAVES>(s_red);
    if (t.idx == INT64_MAX) {  // phase 1: the violation cannot decrease; phase 2: optimum
        if (blockIdx.x == 0 && tid == 0) st->status = ph1 ? ST_INFEASIBLE : ST_OPTIMAL;
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
        for (int64_t k = tid; k < L2; k += PBOX_BLOCK) {
            d[k] = rp[k];
            d[L2 + k] = ap[k];
        }
        __syncthreads();
    }
    const dbl2* xr = XL ? reinterpret_cast<const dbl2*>(dsm) : rp;
    const dbl2* xa = XL ? reinterpret_cast<const dbl2*>(dsm) + L2 : ap;

    const int64_t i = (int64_t)blockIdx.x * WAVES + wave;
    double rt = INFINITY;
    int64_t ri = INT64_MAX;
    if (i < m) {
        const double sg = F.is_free[p] ? (t.d < 0.0 ? 1.0 : -1.0) : (D.at_upper[p] ? -1.0 : 1.0);
        const double xi = P.x_b[i], ubi = D.ub_B[i], lbi = F.lb_B[i];
        const double wi = ph1 ? X.w[i] : 0.0;
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
        const double ah = sg * alpha;
        if (wi == 0.0) {  // a feasible row: phase 2's entry; no lower bound (a free basic column): no entry
            if (ah > D.piv_tol && lbi > -INFINITY) {
                rt = (xi > 0.0 ? xi : 0.0) / ah;
                ri = 2 * i;
            } else if (ah < -D.piv_tol && ubi < INFINITY) {
                const double gap = ubi - xi;
                rt = (gap > 0.0 ? gap : 0.0) / (-ah);
                ri = 2 * i + 1;
            }
        } else if (wi > 0.0) {  // below: blocks where it rises to 0
            if (ah < -D.piv_tol) {
                rt = xi / ah;
                ri = 2 * i;
            }
        } else {  // above: blocks where it falls to its bound
            if (ah > D.piv_tol) {
                rt = (xi - ubi) / ah;
                ri = 2 * i + 1;
            }
        }
    }
    if (lane == 0) s_rat[wave] = ArgMinEntry{rt, ri};
    __syncthreads();
    if (tid == 0) {
        ArgMinEntry b = s_rat[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            const ArgMinEntry v = s_rat[w];
            const bool tk = argmin_better(v.val, v.idx, b.val, b.idx);
            b.val = tk ? v.val : b.val;
            b.idx = tk ? v.idx : b.idx;
        }
        D.rparts[blockIdx.x] = b;
    }
}

// k_pbox_step1 with free columns.  A free entering column starts from 0 with
// the sign k_pbox_update_f used and has no bound to flip to (u_p = +inf: no row
// is ST_UNBOUNDED, in phase 1 ST_BREAKDOWN); a pivot stores lb_B[q] (-inf for a
// free entering column, else 0) beside ub_B[q]; rows are classified with
// lb_B.  The leaving column is never free (its row had no ratio entry), so the
// placements after a pivot are k_pbox_step1's.
__global__ __launch_bounds__(1024) void k_pbox_step_f(Params P, PboxArgs D, Pbox1Args X, PboxFreeArgs F) {
    constexpr int BLOCK = 1024, WAVES = BLOCK / 64, CH = 4;
    DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = P.m, L = P.L;
    __shared__ PboxSnap S;
    __shared__ ArgMinEntry s_red[WAVES];
    __shared__ ArgMinEntry s_win;
    __shared__ double s_up;
    __shared__ int32_t s_at, s_fr;
    __shared__ int32_t s_ninf, s_stale, s_cnt;
    if (tid == 0) {
        S.it = st->iter;
        S.limit = st->limit;
        S.status = st->status;
        S.y_buf = st->y_buf;
        S.cnt = st->nb_count;
        S.fresh = D.rec->fresh;
        S.p = D.rec->p;
        S.d_p = D.rec->d_p;
        s_ninf = X.ph->ninf;
        s_stale = X.ph->y_stale;
        s_cnt = 0;
    }
    __syncthreads();
    const int64_t it = S.it;
    if (S.status != ST_RUNNING || it >= S.limit || !S.fresh) return;
    const bool ph1 = s_ninf > 0;
    const double ftol = X.feas_tol;

    double bv = INFINITY;
    int64_t bi = INT64_MAX;
    for (int g = tid; g < D.update_grid; g += BLOCK) {
        const ArgMinEntry v = D.rparts[g];
        if (argmin_better(v.val, v.idx, bv, bi)) {
            bv = v.val;
            bi = v.idx;
        }
    }
    wave_argmin(bv, bi);
    if (lane == 0) s_red[wave] = ArgMinEntry{bv, bi};
    __syncthreads();
    if (tid == 0) {
        ArgMinEntry t = s_red[0];
        for (int w = 1; w < WAVES; ++w)
            if (argmin_better(s_red[w].val, s_red[w].idx, t.val, t.idx)) t = s_red[w];
        s_win = t;
        s_up = D.ub[S.p];
        s_at = D.at_upper[S.p];
        s_fr = F.is_free[S.p];
    }
    __syncthreads();
    const double tq = s_win.val;
    const bool none = s_win.idx == INT64_MAX;
    const int64_t q = none ? 0 : (s_win.idx >> 1);
    const int side = none ? 0 : (int)(s_win.idx & 1);
    const int64_t p = S.p;
    const double u_p = s_up;
    const int up_p = s_at;
    const bool fr_p = s_fr != 0;
    const double sg = fr_p ? (S.d_p < 0.0 ? 1.0 : -1.0) : (up_p ? -1.0 : 1.0);
    const double* al = ((it + 1) & 1) ? P.alpha1 : P.alpha0;
    double* a_cur = (it & 1) ? P.alpha1 : P.alpha0;
    const bool flip = u_p < INFINITY && (none || u_p <= tq);  // (a free column: u_p = +inf)

    if (flip || none) {
        if (flip) {
            const double dx = up_p ? -u_p : u_p;
            const double* Ap = P.A + p * L;
            int bad = 0;
            for (int64_t i = tid; i < m; i += BLOCK) {
                const double xn = fma(-u_p, sg * al[i], P.x_b[i]);
                P.x_b[i] = xn;
                D.b_eff[i] = fma(-dx, Ap[i], D.b_eff[i]);
                if (ph1) {
                    const double wv = row_class_f(xn, F.lb_B[i], D.ub_B[i], ftol);
                    X.w[i] = wv;
                    bad += wv != 0.0;
                }
            }
            if (ph1 && bad) atomicAdd(&s_cnt, bad);  // (an integer count: order-free)
        }
        for (int64_t i = tid; i < L; i += BLOCK) a_cur[i] = (i == 0) ? 1.0 : 0.0;
        __syncthreads();
        if (tid == 0) {
            if (flip) {
                D.at_upper[p] = up_p ? 0 : 1;
                D.rec->flips += 1;
                if (ph1) {
                    X.ph->ninf = s_cnt;
                    X.ph->passes += 1;
                }
            } else {
                st->status = ph1 ? ST_BREAKDOWN : ST_UNBOUNDED;
            }
            if (!ph1 && s_stale) X.ph->y_stale = 0;
            st->q = 0;
            st->aq = 1.0;
            st->p = p;
            st->min_e = S.d_p;
            D.rec->fresh = 0;
        }
        return;
    }

    double* y = S.y_buf ? P.y1 : P.y0;
    const double aq = al[q];
    const double theta = tq, sy = -(S.d_p / aq);
    const double x_off = up_p ? u_p : 0.0;  // (a free column sits at 0 and is never at upper)
    const double l_p = fr_p ? -INFINITY : 0.0;
    const bool book = tid == BLOCK - 64;
    int64_t leave = -1;
    double c_p = 0.0;
    int kp = -1, last = -1;
    if (book) {
        leave = P.b_ixs[q];
        c_p = P.c[p];
        kp = P.nb_pos[p];
        last = P.nb_list[S.cnt - 1];
    }
    const double* Sq = P.B0 + q * L;
    int bad = 0;
    for (int64_t i0 = tid; i0 < L; i0 += (int64_t)CH * BLOCK) {
        double xv[CH], av[CH], yv[CH], rv[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t i = i0 + (int64_t)u * BLOCK;
            xv[u] = i < m ? P.x_b[i] : 0.0;
            av[u] = i < m ? al[i] : 0.0;
            yv[u] = i < L ? y[i] : 0.0;
            rv[u] = i < L ? Sq[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t i = i0 + (int64_t)u * BLOCK;
            if (i < m) {
                const double xn = (i == q) ? x_off + sg * theta : fma(-theta, sg * av[u], xv[u]);
                P.x_b[i] = xn;
                if (ph1) {  // (row q's bounds are the entering column's: the bookkeeping lane stores them below)
                    const double wv = row_class_f(xn, i == q ? l_p : F.lb_B[i], i == q ? u_p : D.ub_B[i], ftol);
                    X.w[i] = wv;
                    bad += wv != 0.0;
                }
            }
            if (i < L) {
                if (!ph1) y[i] = fma(sy, rv[u], yv[u]);
                P.rbuf[i] = rv[u];
            }
        }
    }
    if (ph1 && bad) atomicAdd(&s_cnt, bad);
    __syncthreads();
    if (book) {
        P.c_B[q] = c_p;
        P.b_ixs[q] = p;
        D.ub_B[q] = u_p;
        F.lb_B[q] = l_p;
        D.at_upper[p] = 0;
        D.at_upper[leave] = (int8_t)side;
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
        st->y_applied = it + 1;
        st->xb_applied = it + 1;
        st->p = p;
        st->q = q;
        st->min_e = S.d_p;
        st->iter = it + 1;
        record_pivot(P, it, p, q);
        D.rec->fresh = 0;
        if (side) D.rec->to_upper += 1;
        if (ph1) {
            X.ph->ninf = s_cnt;
            X.ph->passes += 1;
            X.ph->pivots += 1;
            X.ph->y_stale = 1;
        } else if (s_stale) {
            X.ph->y_stale = 0;
        }
    }
}

// k_pbox_classify with lb_B: a row whose basic column is free is feasible
__global__ __launch_bounds__(1024) void k_pbox_classify_f(Params P, PboxArgs D, Pbox1Args X, PboxFreeArgs F, int entry) {
    __shared__ int32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    int bad = 0;
    for (int64_t i = threadIdx.x; i < P.L; i += 1024) {
        const double wv = i < P.m ? row_class_f(P.x_b[i], F.lb_B[i], D.ub_B[i], X.feas_tol) : 0.0;
        X.w[i] = wv;
        bad += wv != 0.0;
    }
    if (bad) atomicAdd(&s_cnt, bad);
    __syncthreads();
    if (threadIdx.x == 0) {
        X.ph->ninf = s_cnt;
        if (entry) X.ph->ninf0 = s_cnt;
    }
}

// ---------------------------------------------------------------------------
// Steepest edge (spx_pbox.h)
// ---------------------------------------------------------------------------
namespace {

// a column's dots with y (and, PEND, with rho and tau) in k_pbox_price's order:
// chunks ascending into two partial sums per lane and operand, one butterfly each
template <bool PEND>
__device__ __forceinline__ void se_dots(const dbl2* col, int nch, int lane, const dbl2* yv, const dbl2* rv,
                                        const dbl2* tv, double& dy, double& dr, double& dt) {
    constexpr int U = 8;
    dbl2 cur[U], nxt[U];
#pragma unroll
    for (int t = 0; t < U; ++t) cur[t] = t < nch ? ld2<SPX_NT_A>(col + 64 * t) : dbl2{0.0, 0.0};
    double d0 = 0.0, d1 = 0.0, r0 = 0.0, r1 = 0.0, t0 = 0.0, t1 = 0.0;
    for (int c0 = 0; c0 < nch; c0 += U) {
#pragma unroll
        for (int t = 0; t < U; ++t)
            nxt[t] = c0 + U + t < nch ? ld2<SPX_NT_A>(col + 64 * (c0 + U + t)) : dbl2{0.0, 0.0};
#pragma unroll
        for (int t = 0; t < U; ++t) {
            if (c0 + t < nch) {
                const int k = 64 * (c0 + t) + lane;
                const dbl2 w = yv[k];
                d0 = fma(cur[t].x, w.x, d0);
                d1 = fma(cur[t].y, w.y, d1);
                if constexpr (PEND) {
                    const dbl2 r = rv[k], u = tv[k];
                    r0 = fma(cur[t].x, r.x, r0);
                    r1 = fma(cur[t].y, r.y, r1);
                    t0 = fma(cur[t].x, u.x, t0);
                    t1 = fma(cur[t].y, u.y, t1);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) cur[t] = nxt[t];
    }
    dy = wave_sum(d0 + d1);
    if constexpr (PEND) {
        dr = wave_sum(r0 + r1);
        dt = wave_sum(t0 + t1);
    }
}

}  // namespace

// NL: vectors staged in LDS -- 0 none, 1 y, 3 y, rho and tau (rho and tau only
// while an update is pending).  The arithmetic does not depend on NL.
template <int NL>
__global__ __launch_bounds__(PBOX_BLOCK) void k_pbox_price_se(Params P, PboxArgs D, PboxSeArgs E) {
    constexpr int WAVES = PBOX_WAVES;
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    __shared__ PboxPartial s_red[WAVES];
    const DevState* st = P.st;
    const int32_t status = st->status;
    const int32_t cnt = st->nb_count;
    const int32_t y_buf = st->y_buf;
    const int64_t iter = st->iter, limit = st->limit;
    const bool pend = E.se->pend != 0;
    const int64_t leave = E.se->leave;
    const double aq = E.se->aq, gp = E.se->gp;
    if (E.apply) {
        if (!pend) return;
    } else if (status != ST_RUNNING || iter >= limit) {
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t L = P.L, L2 = L >> 1;
    const int nch = (int)(L2 >> 6);
    const dbl2* y_g = reinterpret_cast<const dbl2*>(y_buf ? P.y1 : P.y0);
    const dbl2* r_g = reinterpret_cast<const dbl2*>(E.rho);
    const dbl2* t_g = reinterpret_cast<const dbl2*>(E.tau);
    if constexpr (NL >= 1) {
        dbl2* d = reinterpret_cast<dbl2*>(dsm);
        for (int64_t k = tid; k < L2; k += PBOX_BLOCK) d[k] = y_g[k];
        if (NL == 3 && pend) {
            for (int64_t k = tid; k < L2; k += PBOX_BLOCK) {
                d[L2 + k] = r_g[k];
                d[2 * L2 + k] = t_g[k];
            }
        }
        __syncthreads();
    }
    const dbl2* yv = NL >= 1 ? reinterpret_cast<const dbl2*>(dsm) : y_g;
    const dbl2* rv = NL == 3 ? reinterpret_cast<const dbl2*>(dsm) + L2 : r_g;
    const dbl2* tv = NL == 3 ? reinterpret_cast<const dbl2*>(dsm) + 2 * L2 : t_g;
    const double* ys = reinterpret_cast<const double*>(yv);
    const double* rs = reinterpret_cast<const double*>(rv);
    const double* ts = reinterpret_cast<const double*>(tv);

    double bkey = INFINITY, bd = 0.0;
    int64_t bidx = INT64_MAX;
    const int nwv = (int)gridDim.x * WAVES;
    for (int s = (int)blockIdx.x * WAVES + wave; s < cnt; s += nwv) {
        const int64_t j = P.nb_list[s];
        const int up = D.at_upper[j];
        double gam = E.gamma[j];
        const double cj = P.c[j];
        double dy, dr = 0.0, dt = 0.0;
        if (P.slack_unit && j >= P.ns) {  // A_j = e_k: no stream
            dy = ys[j - P.ns];
            if (pend) {
                dr = rs[j - P.ns];
                dt = ts[j - P.ns];
            }
        } else {
            const dbl2* col = reinterpret_cast<const dbl2*>(P.A + j * L) + lane;
            if (pend) se_dots<true>(col, nch, lane, yv, rv, tv, dy, dr, dt);
            else se_dots<false>(col, nch, lane, yv, rv, tv, dy, dr, dt);
        }
        if (pend && j != leave) {  // Goldfarb and Reid; the commit wrote the leaving column's weight
            const double g = dr / aq;
            const double gn = fma(g * g, gp, fma(-2.0 * g, dt, gam));
            const double fl = fma(g, g, 1.0);
            gam = gn > fl ? gn : fl;
            if (lane == 0) E.gamma[j] = gam;  // one owner per column
        }
        if (E.apply) continue;
        const double d = dy - cj;
        const double sd = up ? -d : d;  // sigma_j d_j (a sign flip: exact)
        const double key = -(d * d) / gam;
        if (sd < -P.eps && argmin_better(key, j, bkey, bidx)) {
            bkey = key;
            bidx = j;
            bd = d;
        }
    }
    if (E.apply) return;
    if (lane == 0) s_red[wave] = PboxPartial{bkey, bidx, bd, 0.0};
    __syncthreads();
    if (tid == 0) D.parts[blockIdx.x] = merge_price<WAVES>(s_red);  // read after the kernel boundary (k_pbox_update)
}

// gamma_j = 1 + ||A_j||^2 for every column, in se_dots' order
__global__ __launch_bounds__(PBOX_BLOCK) void k_pbox_se_init(Params P, PboxSeArgs E) {
    constexpr int WAVES = PBOX_WAVES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t L = P.L, L2 = L >> 1;
    const int nch = (int)(L2 >> 6);
    const int64_t nwv = (int64_t)gridDim.x * WAVES;
    for (int64_t j = (int64_t)blockIdx.x * WAVES + wave; j < P.n; j += nwv) {
        double g;
        if (P.slack_unit && j >= P.ns) {
            g = 2.0;
        } else {
            const dbl2* col = reinterpret_cast<const dbl2*>(P.A + j * L) + lane;
            double d0 = 0.0, d1 = 0.0;
            for (int c = 0; c < nch; ++c) {
                const dbl2 a = col[64 * c];
                d0 = fma(a.x, a.x, d0);
                d1 = fma(a.y, a.y, d1);
            }
            g = 1.0 + wave_sum(d0 + d1);
        }
        if (lane == 0) E.gamma[j] = g;
    }
}

// k_pbox_step with the steepest-edge bookkeeping (spx_pbox.h)
__global__ __launch_bounds__(1024) void k_pbox_step_se(Params P, PboxArgs D, PboxSeArgs E) {
    constexpr int BLOCK = 1024, WAVES = BLOCK / 64, CH = 4;
    DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = P.m, L = P.L;
    __shared__ PboxSnap S;
    __shared__ ArgMinEntry s_red[WAVES];
    __shared__ ArgMinEntry s_win;
    __shared__ double s_up;
    __shared__ int32_t s_at;
    __shared__ double s_gp[WAVES];
    if (tid == 0) {
        S.it = st->iter;
        S.limit = st->limit;
        S.status = st->status;
        S.y_buf = st->y_buf;
        S.cnt = st->nb_count;
        S.fresh = D.rec->fresh;
        S.p = D.rec->p;
        S.d_p = D.rec->d_p;
    }
    __syncthreads();
    const int64_t it = S.it;
    if (S.status != ST_RUNNING || it >= S.limit || !S.fresh) {
        if (tid == 0) {
            E.se->need_tau = 0;
            // the optimum was found by a pass whose pricing applied the pending recurrence
            if (S.status == ST_OPTIMAL) E.se->pend = 0;
        }
        return;
    }

    double bv = INFINITY;
    int64_t bi = INT64_MAX;
    for (int g = tid; g < D.update_grid; g += BLOCK) {
        const ArgMinEntry v = D.rparts[g];
        if (argmin_better(v.val, v.idx, bv, bi)) {
            bv = v.val;
            bi = v.idx;
        }
    }
    wave_argmin(bv, bi);
    if (lane == 0) s_red[wave] = ArgMinEntry{bv, bi};
    __syncthreads();
    if (tid == 0) {
        ArgMinEntry t = s_red[0];
        for (int w = 1; w < WAVES; ++w)
            if (argmin_better(s_red[w].val, s_red[w].idx, t.val, t.idx)) t = s_red[w];
        s_win = t;
        s_up = D.ub[S.p];
        s_at = D.at_upper[S.p];
    }
    __syncthreads();
    const double tq = s_win.val;
    const bool none = s_win.idx == INT64_MAX;
    const int64_t q = none ? 0 : (s_win.idx >> 1);
    const int side = none ? 0 : (int)(s_win.idx & 1);
    const int64_t p = S.p;
    const double u_p = s_up;
    const int up_p = s_at;
    const double sg = up_p ? -1.0 : 1.0;
    const double* al = ((it + 1) & 1) ? P.alpha1 : P.alpha0;
    double* a_cur = (it & 1) ? P.alpha1 : P.alpha0;
    const bool flip = u_p < INFINITY && (none || u_p <= tq);

    if (flip || none) {
        if (flip) {
            const double dx = up_p ? -u_p : u_p;
            const double* Ap = P.A + p * L;
            for (int64_t i = tid; i < m; i += BLOCK) {
                P.x_b[i] = fma(-u_p, sg * al[i], P.x_b[i]);
                D.b_eff[i] = fma(-dx, Ap[i], D.b_eff[i]);
            }
        }
        for (int64_t i = tid; i < L; i += BLOCK) a_cur[i] = (i == 0) ? 1.0 : 0.0;
        if (tid == 0) {
            if (flip) {
                D.at_upper[p] = up_p ? 0 : 1;
                D.rec->flips += 1;
            } else {
                st->status = ST_UNBOUNDED;
            }
            st->q = 0;
            st->aq = 1.0;
            st->p = p;
            st->min_e = S.d_p;
            D.rec->fresh = 0;
            E.se->pend = 0;  // (this pass's pricing applied it; a flip changes no weight)
            E.se->need_tau = 0;
        }
        return;
    }

    // pivot it
    double* y = S.y_buf ? P.y1 : P.y0;
    const double aq = al[q];
    const double theta = tq, sy = -(S.d_p / aq);
    const double x_off = up_p ? u_p : 0.0;
    const bool book = tid == BLOCK - 64;
    int64_t leave = -1;
    double c_p = 0.0;
    int kp = -1, last = -1;
    if (book) {
        leave = P.b_ixs[q];
        c_p = P.c[p];
        kp = P.nb_pos[p];
        last = P.nb_list[S.cnt - 1];
    }
    // ||alpha||^2: a thread's rows ascending, one butterfly, the waves in order
    double a2 = 0.0;
    for (int64_t i = tid; i < m; i += BLOCK) a2 = fma(al[i], al[i], a2);
    a2 = wave_sum(a2);
    if (lane == 0) s_gp[wave] = a2;
    const double* Sq = P.B0 + q * L;
    for (int64_t i0 = tid; i0 < L; i0 += (int64_t)CH * BLOCK) {
        double xv[CH], av[CH], yv[CH], rv[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t i = i0 + (int64_t)u * BLOCK;
            xv[u] = i < m ? P.x_b[i] : 0.0;
            av[u] = i < m ? al[i] : 0.0;
            yv[u] = i < L ? y[i] : 0.0;
            rv[u] = i < L ? Sq[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t i = i0 + (int64_t)u * BLOCK;
            if (i < m) P.x_b[i] = (i == q) ? x_off + sg * theta : fma(-theta, sg * av[u], xv[u]);
            if (i < L) {
                y[i] = fma(sy, rv[u], yv[u]);
                P.rbuf[i] = rv[u];
                E.rho[i] = rv[u];  // the weight update's own copy
            }
        }
    }
    __syncthreads();
    if (book) {
        double t = s_gp[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) t += s_gp[w];
        const double gp = 1.0 + t;
        const double gl = gp / (aq * aq);
        E.gamma[leave] = gl > 1.0 ? gl : 1.0;
        E.se->aq = aq;
        E.se->gp = gp;
        E.se->leave = leave;
        E.se->pend = 1;
        E.se->need_tau = 1;
        P.c_B[q] = c_p;
        P.b_ixs[q] = p;
        D.ub_B[q] = u_p;
        D.at_upper[p] = 0;
        D.at_upper[leave] = (int8_t)side;
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
        st->y_applied = it + 1;
        st->xb_applied = it + 1;
        st->p = p;
        st->q = q;
        st->min_e = S.d_p;
        st->iter = it + 1;
        record_pivot(P, it, p, q);
        D.rec->fresh = 0;
        if (side) D.rec->to_upper += 1;
    }
}

// tau's per-row-block partial vectors: k_pbox_vtb with v = alpha[iter & 1] (the
// alpha of the pivot k_pbox_step_se has just committed) and S read as it is
__global__ __launch_bounds__(PBOX_VTB_BLOCK) void k_pbox_tau(Params P, PboxSeArgs E) {
    constexpr int WAVES = PBOX_VTB_WAVES, U = 8;
    __shared__ double s_v[PBOX_VTB_ROWS];
    __shared__ int32_t s_row[PBOX_VTB_ROWS];
    __shared__ int32_t s_n;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (!E.se->need_tau) return;  // (written by k_pbox_step_se alone: one value for the whole launch)
    const double* v = (P.st->iter & 1) ? P.alpha1 : P.alpha0;
    const int64_t m = P.m, L = P.L, L2 = L >> 1;
    const int nch = (int)(L2 >> 6);
    const int64_t r0 = (int64_t)blockIdx.y * PBOX_VTB_ROWS;
    if (wave == 0) {
        const int64_t i = r0 + lane;
        const double vi = i < m ? v[i] : 0.0;
        const unsigned long long mask = __ballot(vi != 0.0);
        const int pos = __popcll(mask & ((1ull << lane) - 1ull));
        if (vi != 0.0) {
            s_v[pos] = vi;
            s_row[pos] = lane;
        }
        if (lane == 0) s_n = __popcll(mask);
    }
    __syncthreads();
    const int c = (int)blockIdx.x * WAVES + wave;
    if (c >= nch) return;
    const int n = s_n;
    const dbl2* base = reinterpret_cast<const dbl2*>(P.B0 + r0 * L) + 64 * c + lane;
    dbl2 acc{0.0, 0.0};
    dbl2 cur[U], nxt[U];
#pragma unroll
    for (int t = 0; t < U; ++t) cur[t] = t < n ? ld2<SPX_NT_BLOAD>(base + (int64_t)s_row[t] * L2) : dbl2{0.0, 0.0};
    for (int k0 = 0; k0 < n; k0 += U) {
#pragma unroll
        for (int t = 0; t < U; ++t)
            nxt[t] = k0 + U + t < n ? ld2<SPX_NT_BLOAD>(base + (int64_t)s_row[k0 + U + t] * L2) : dbl2{0.0, 0.0};
#pragma unroll
        for (int t = 0; t < U; ++t) {
            if (k0 + t < n) {
                const double vv = s_v[k0 + t];
                acc.x = fma(vv, cur[t].x, acc.x);
                acc.y = fma(vv, cur[t].y, acc.y);
            }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) cur[t] = nxt[t];
    }
    reinterpret_cast<dbl2*>(E.tparts + (int64_t)blockIdx.y * L)[64 * c + lane] = acc;  // read after the kernel boundary
}

// k_pbox_vtb_sum's order, into tau
__global__ __launch_bounds__(PBOX_VTB_BLOCK) void k_pbox_tau_sum(Params P, PboxSeArgs E) {
    constexpr int WAVES = PBOX_VTB_WAVES;
    __shared__ dbl2 s_acc[WAVES][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (!E.se->need_tau) return;
    const int64_t L2 = P.L >> 1;
    const int64_t k = (int64_t)blockIdx.x * 64 + lane;
    const int nb = E.vtb_blocks, per = (nb + WAVES - 1) / WAVES;
    const int b0 = wave * per, b1 = b0 + per < nb ? b0 + per : nb;
    const dbl2* parts = reinterpret_cast<const dbl2*>(E.tparts) + k;
    dbl2 acc{0.0, 0.0};
#pragma unroll 4
    for (int b = b0; b < b1; ++b) {
        const dbl2 t = parts[(int64_t)b * L2];
        acc.x += t.x;
        acc.y += t.y;
    }
    s_acc[wave][lane] = acc;
    __syncthreads();
    if (wave == 0) {
        dbl2 r = s_acc[0][lane];
#pragma unroll
        for (int g = 1; g < WAVES; ++g) {
            r.x += s_acc[g][lane].x;
            r.y += s_acc[g][lane].y;
        }
        reinterpret_cast<dbl2*>(E.tau)[k] = r;
    }
}

// ---------------------------------------------------------------------------
// Steepest edge through phase 1 (spx_pbox.h)
// ---------------------------------------------------------------------------
// k_pbox_price_se with the phase read from the device: phase 1 prices with yp
// and no c_j; the recurrence, the weights' owner and the key are the same in
// both phases.  (The apply-only mode stays k_pbox_price_se's.)
template <int NL>
__global__ __launch_bounds__(PBOX_BLOCK) void k_pbox_price_se1(Params P, PboxArgs D, Pbox1Args X, PboxSeArgs E) {
    constexpr int WAVES = PBOX_WAVES;
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    __shared__ PboxPartial s_red[WAVES];
    const DevState* st = P.st;
    const int32_t status = st->status;
    const int32_t cnt = st->nb_count;
    const int32_t y_buf = st->y_buf;
    const int64_t iter = st->iter, limit = st->limit;
    const bool ph1 = X.ph->ninf > 0;
    const bool pend = E.se->pend != 0;
    const int64_t leave = E.se->leave;
    const double aq = E.se->aq, gp = E.se->gp;
    if (status != ST_RUNNING || iter >= limit) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t L = P.L, L2 = L >> 1;
    const int nch = (int)(L2 >> 6);
    const dbl2* y_g = reinterpret_cast<const dbl2*>(ph1 ? X.yp : (y_buf ? P.y1 : P.y0));
    const dbl2* r_g = reinterpret_cast<const dbl2*>(E.rho);
    const dbl2* t_g = reinterpret_cast<const dbl2*>(E.tau);
    if constexpr (NL >= 1) {
        dbl2* d = reinterpret_cast<dbl2*>(dsm);
        for (int64_t k = tid; k < L2; k += PBOX_BLOCK) d[k] = y_g[k];
        if (NL == 3 && pend) {
            for (int64_t k = tid; k < L2; k += PBOX_BLOCK) {
                d[L2 + k] = r_g[k];
                d[2 * L2 + k] = t_g[k];
            }
        }
        __syncthreads();
    }
    const dbl2* yv = NL >= 1 ? reinterpret_cast<const dbl2*>(dsm) : y_g;
    const dbl2* rv = NL == 3 ? reinterpret_cast<const dbl2*>(dsm) + L2 : r_g;
    const dbl2* tv = NL == 3 ? reinterpret_cast<const dbl2*>(dsm) + 2 * L2 : t_g;
    const double* ys = reinterpret_cast<const double*>(yv);
    const double* rs = reinterpret_cast<const double*>(rv);
    const double* ts = reinterpret_cast<const double*>(tv);

    double bkey = INFINITY, bd = 0.0;
    int64_t bidx = INT64_MAX;
    const int nwv = (int)gridDim.x * WAVES;
    for (int s = (int)blockIdx.x * WAVES + wave; s < cnt; s += nwv) {
        const int64_t j = P.nb_list[s];
        const int up = D.at_upper[j];
        double gam = E.gamma[j];
        const double cj = ph1 ? 0.0 : P.c[j];  // (x - 0.0 = x: exact)
        double dy, dr = 0.0, dt = 0.0;
        if (P.slack_unit && j >= P.ns) {  // A_j = e_k: no stream
            dy = ys[j - P.ns];
            if (pend) {
                dr = rs[j - P.ns];
                dt = ts[j - P.ns];
            }
        } else {
            const dbl2* col = reinterpret_cast<const dbl2*>(P.A + j * L) + lane;
            if (pend) se_dots<true>(col, nch, lane, yv, rv, tv, dy, dr, dt);
            else se_dots<false>(col, nch, lane, yv, rv, tv, dy, dr, dt);
        }
        if (pend && j != leave) {  // Goldfarb and Reid; the commit wrote the leaving column's weight
            const double g = dr / aq;
            const double gn = fma(g * g, gp, fma(-2.0 * g, dt, gam));
            const double fl = fma(g, g, 1.0);
            gam = gn > fl ? gn : fl;
            if (lane == 0) E.gamma[j] = gam;  // one owner per column
        }
        const double d = dy - cj;
        const double sd = up ? -d : d;  // sigma_j d_j (a sign flip: exact)
        const double key = -(d * d) / gam;
        if (sd < -P.eps && argmin_better(key, j, bkey, bidx)) {
            bkey = key;
            bidx = j;
            bd = d;
        }
    }
    if (lane == 0) s_red[wave] = PboxPartial{bkey, bidx, bd, 0.0};
    __syncthreads();
    if (tid == 0) D.parts[blockIdx.x] = merge_price<WAVES>(s_red);  // read after the kernel boundary (k_pbox_update1)
}

// k_pbox_step1's decisions and commit with k_pbox_step_se's bookkeeping: a pivot
// of either phase records the weight update (gamma_p, gamma_leave, rho, pend,
// need_tau); a flip, ST_INFEASIBLE, ST_BREAKDOWN, ST_UNBOUNDED and an optimum
// clear pend (this pass's pricing applied it), the limit leaves it.
__global__ __launch_bounds__(1024) void k_pbox_step_se1(Params P, PboxArgs D, Pbox1Args X, PboxSeArgs E) {
    constexpr int BLOCK = 1024, WAVES = BLOCK / 64, CH = 4;
    DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = P.m, L = P.L;
    __shared__ PboxSnap S;
    __shared__ ArgMinEntry s_red[WAVES];
    __shared__ ArgMinEntry s_win;
    __shared__ double s_up;
    __shared__ int32_t s_at;
    __shared__ int32_t s_ninf, s_stale, s_cnt;
    __shared__ double s_gp[WAVES];
    if (tid == 0) {
        S.it = st->iter;
        S.limit = st->limit;
        S.status = st->status;
        S.y_buf = st->y_buf;
        S.cnt = st->nb_count;
        S.fresh = D.rec->fresh;
        S.p = D.rec->p;
        S.d_p = D.rec->d_p;
        s_ninf = X.ph->ninf;
        s_stale = X.ph->y_stale;
        s_cnt = 0;
    }
    __syncthreads();
    const int64_t it = S.it;
    if (S.status != ST_RUNNING || it >= S.limit || !S.fresh) {
        if (tid == 0) {
            E.se->need_tau = 0;
            // the pass that found the optimum, or no phase-1 candidate, applied the pending recurrence in its pricing
            if (S.status == ST_OPTIMAL || S.status == ST_INFEASIBLE) E.se->pend = 0;
        }
        return;
    }
    const bool ph1 = s_ninf > 0;
    const double ftol = X.feas_tol;

    double bv = INFINITY;
    int64_t bi = INT64_MAX;
    for (int g = tid; g < D.update_grid; g += BLOCK) {
        const ArgMinEntry v = D.rparts[g];
        if (argmin_better(v.val, v.idx, bv, bi)) {
            bv = v.val;
            bi = v.idx;
        }
    }
    wave_argmin(bv, bi);
    if (lane == 0) s_red[wave] = ArgMinEntry{bv, bi};
    __syncthreads();
    if (tid == 0) {
        ArgMinEntry t = s_red[0];
        for (int w = 1; w < WAVES; ++w)
            if (argmin_better(s_red[w].val, s_red[w].idx, t.val, t.idx)) t = s_red[w];
        s_win = t;
        s_up = D.ub[S.p];
        s_at = D.at_upper[S.p];
    }
    __syncthreads();
    const double tq = s_win.val;
    const bool none = s_win.idx == INT64_MAX;
    const int64_t q = none ? 0 : (s_win.idx >> 1);
    const int side = none ? 0 : (int)(s_win.idx & 1);
    const int64_t p = S.p;
    const double u_p = s_up;
    const int up_p = s_at;
    const double sg = up_p ? -1.0 : 1.0;
    const double* al = ((it + 1) & 1) ? P.alpha1 : P.alpha0;
    double* a_cur = (it & 1) ? P.alpha1 : P.alpha0;
    const bool flip = u_p < INFINITY && (none || u_p <= tq);

    if (flip || none) {
        if (flip) {
            const double dx = up_p ? -u_p : u_p;
            const double* Ap = P.A + p * L;
            int bad = 0;
            for (int64_t i = tid; i < m; i += BLOCK) {
                const double xn = fma(-u_p, sg * al[i], P.x_b[i]);
                P.x_b[i] = xn;
                D.b_eff[i] = fma(-dx, Ap[i], D.b_eff[i]);
                if (ph1) {
                    const double wv = row_class(xn, D.ub_B[i], ftol);
                    X.w[i] = wv;
                    bad += wv != 0.0;
                }
            }
            if (ph1 && bad) atomicAdd(&s_cnt, bad);  // (an integer count: order-free)
        }
        for (int64_t i = tid; i < L; i += BLOCK) a_cur[i] = (i == 0) ? 1.0 : 0.0;
        __syncthreads();
        if (tid == 0) {
            if (flip) {
                D.at_upper[p] = up_p ? 0 : 1;
                D.rec->flips += 1;
                if (ph1) {
                    X.ph->ninf = s_cnt;
                    X.ph->passes += 1;
                }
            } else {
                st->status = ph1 ? ST_BREAKDOWN : ST_UNBOUNDED;
            }
            if (!ph1 && s_stale) X.ph->y_stale = 0;
            st->q = 0;
            st->aq = 1.0;
            st->p = p;
            st->min_e = S.d_p;
            D.rec->fresh = 0;
            E.se->pend = 0;  // (this pass's pricing applied it; a flip changes no weight)
            E.se->need_tau = 0;
        }
        return;
    }

    // pivot it
    double* y = S.y_buf ? P.y1 : P.y0;
    const double aq = al[q];
    const double theta = tq, sy = -(S.d_p / aq);
    const double x_off = up_p ? u_p : 0.0;
    const bool book = tid == BLOCK - 64;
    int64_t leave = -1;
    double c_p = 0.0;
    int kp = -1, last = -1;
    if (book) {
        leave = P.b_ixs[q];
        c_p = P.c[p];
        kp = P.nb_pos[p];
        last = P.nb_list[S.cnt - 1];
    }
    // ||alpha||^2: a thread's rows ascending, one butterfly, the waves in order (k_pbox_step_se's)
    double a2 = 0.0;
    for (int64_t i = tid; i < m; i += BLOCK) a2 = fma(al[i], al[i], a2);
    a2 = wave_sum(a2);
    if (lane == 0) s_gp[wave] = a2;
    const double* Sq = P.B0 + q * L;
    int bad = 0;
    for (int64_t i0 = tid; i0 < L; i0 += (int64_t)CH * BLOCK) {
        double xv[CH], av[CH], yv[CH], rv[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t i = i0 + (int64_t)u * BLOCK;
            xv[u] = i < m ? P.x_b[i] : 0.0;
            av[u] = i < m ? al[i] : 0.0;
            yv[u] = i < L ? y[i] : 0.0;
            rv[u] = i < L ? Sq[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t i = i0 + (int64_t)u * BLOCK;
            if (i < m) {
                const double xn = (i == q) ? x_off + sg * theta : fma(-theta, sg * av[u], xv[u]);
                P.x_b[i] = xn;
                if (ph1) {  // (row q's bound is the entering column's: the bookkeeping lane stores it below)
                    const double wv = row_class(xn, i == q ? u_p : D.ub_B[i], ftol);
                    X.w[i] = wv;
                    bad += wv != 0.0;
                }
            }
            if (i < L) {
                if (!ph1) y[i] = fma(sy, rv[u], yv[u]);
                P.rbuf[i] = rv[u];
                E.rho[i] = rv[u];  // the weight update's own copy
            }
        }
    }
    if (ph1 && bad) atomicAdd(&s_cnt, bad);
    __syncthreads();
    if (book) {
        double t = s_gp[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) t += s_gp[w];
        const double gp = 1.0 + t;
        const double gl = gp / (aq * aq);
        E.gamma[leave] = gl > 1.0 ? gl : 1.0;
        E.se->aq = aq;
        E.se->gp = gp;
        E.se->leave = leave;
        E.se->pend = 1;
        E.se->need_tau = 1;
        P.c_B[q] = c_p;
        P.b_ixs[q] = p;
        D.ub_B[q] = u_p;
        D.at_upper[p] = 0;
        D.at_upper[leave] = (int8_t)side;
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
        st->y_applied = it + 1;
        st->xb_applied = it + 1;
        st->p = p;
        st->q = q;
        st->min_e = S.d_p;
        st->iter = it + 1;
        record_pivot(P, it, p, q);
        D.rec->fresh = 0;
        if (side) D.rec->to_upper += 1;
        if (ph1) {
            X.ph->ninf = s_cnt;
            X.ph->passes += 1;
            X.ph->pivots += 1;
            X.ph->y_stale = 1;
        } else if (s_stale) {
            X.ph->y_stale = 0;
        }
    }
}

// ---------------------------------------------------------------------------
// Steepest edge with free columns (spx_pbox.h)
// ---------------------------------------------------------------------------
// k_pbox_price_se1 with free columns: k_pbox_price_f's flag, read per column
// beside at_upper ahead of the stream, decides who is a candidate (|d_j| > eps
// for a free column); the dots, the recurrence, the weights' owner and the key
// are k_pbox_price_se1's, operation for operation.  The phase word is 0 on a
// context without phase 1, so one kernel serves both.
template <int NL>
__global__ __launch_bounds__(PBOX_BLOCK) void k_pbox_price_se_f(Params P, PboxArgs D, Pbox1Args X, PboxSeArgs E,
                                                                PboxFreeArgs F) {
    constexpr int WAVES = PBOX_WAVES;
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    __shared__ PboxPartial s_red[WAVES];
    const DevState* st = P.st;
    const int32_t status = st->status;
    const int32_t cnt = st->nb_count;
    const int32_t y_buf = st->y_buf;
    const int64_t iter = st->iter, limit = st->limit;
    const bool ph1 = X.ph->ninf > 0;
    const bool pend = E.se->pend != 0;
    const int64_t leave = E.se->leave;
    const double aq = E.se->aq, gp = E.se->gp;
    if (status != ST_RUNNING || iter >= limit) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t L = P.L, L2 = L >> 1;
    const int nch = (int)(L2 >> 6);
    const dbl2* y_g = reinterpret_cast<const dbl2*>(ph1 ? X.yp : (y_buf ? P.y1 : P.y0));
    const dbl2* r_g = reinterpret_cast<const dbl2*>(E.rho);
    const dbl2* t_g = reinterpret_cast<const dbl2*>(E.tau);
    if constexpr (NL >= 1) {
        dbl2* d = reinterpret_cast<dbl2*>(dsm);
        for (int64_t k = tid; k < L2; k += PBOX_BLOCK) d[k] = y_g[k];
        if (NL == 3 && pend) {
            for (int64_t k = tid; k < L2; k += PBOX_BLOCK) {
                d[L2 + k] = r_g[k];
                d[2 * L2 + k] = t_g[k];
            }
        }
        __syncthreads();
    }
    const dbl2* yv = NL >= 1 ? reinterpret_cast<const dbl2*>(dsm) : y_g;
    const dbl2* rv = NL == 3 ? reinterpret_cast<const dbl2*>(dsm) + L2 : r_g;
    const dbl2* tv = NL == 3 ? reinterpret_cast<const dbl2*>(dsm) + 2 * L2 : t_g;
    const double* ys = reinterpret_cast<const double*>(yv);
    const double* rs = reinterpret_cast<const double*>(rv);
    const double* ts = reinterpret_cast<const double*>(tv);

    double bkey = INFINITY, bd = 0.0;
    int64_t bidx = INT64_MAX;
    const int nwv = (int)gridDim.x * WAVES;
    for (int s = (int)blockIdx.x * WAVES + wave; s < cnt; s += nwv) {
        const int64_t j = P.nb_list[s];
        const int up = D.at_upper[j];
        const int fr = F.is_free[j];
        double gam = E.gamma[j];
        const double cj = ph1 ? 0.0 : P.c[j];  // (x - 0.0 = x: exact)
        double dy, dr = 0.0, dt = 0.0;
        if (P.slack_unit && j >= P.ns) {  // A_j = e_k: no stream
            dy = ys[j - P.ns];
            if (pend) {
                dr = rs[j - P.ns];
                dt = ts[j - P.ns];
            }
        } else {
            const dbl2* col = reinterpret_cast<const dbl2*>(P.A + j * L) + lane;
            if (pend) se_dots<true>(col, nch, lane, yv, rv, tv, dy, dr, dt);
            else se_dots<false>(col, nch, lane, yv, rv, tv, dy, dr, dt);
        }
        if (pend && j != leave) {  // Goldfarb and Reid; the commit wrote the leaving column's weight
            const double g = dr / aq;
            const double gn = fma(g * g, gp, fma(-2.0 * g, dt, gam));
            const double fl = fma(g, g, 1.0);
            gam = gn > fl ? gn : fl;
            if (lane == 0) E.gamma[j] = gam;  // one owner per column
        }
        const double d = dy - cj;
        const double sd = fr ? -fabs(d) : (up ? -d : d);  // free: either direction improves
        const double key = -(d * d) / gam;
        if (sd < -P.eps && argmin_better(key, j, bkey, bidx)) {
            bkey = key;
            bidx = j;
            bd = d;
        }
    }
    if (lane == 0) s_red[wave] = PboxPartial{bkey, bidx, bd, 0.0};
    __syncthreads();
    if (tid == 0) D.parts[blockIdx.x] = merge_price<WAVES>(s_red);  // read after the kernel boundary (k_pbox_update_f)
}

// k_pbox_step_f's decisions and commit with k_pbox_step_se1's bookkeeping: a
// pivot of either phase records the weight update (gamma_p, gamma_leave, rho,
// pend, need_tau); the leaving column is never free, so its weight needs no new
// case.  pend is cleared as k_pbox_step_se1 clears it.
__global__ __launch_bounds__(1024) void k_pbox_step_se_f(Params P, PboxArgs D, Pbox1Args X, PboxSeArgs E,
                                                         PboxFreeArgs F) {
    constexpr int BLOCK = 1024, WAVES = BLOCK / 64, CH = 4;
    DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = P.m, L = P.L;
    __shared__ PboxSnap S;
    __shared__ ArgMinEntry s_red[WAVES];
    __shared__ ArgMinEntry s_win;
    __shared__ double s_up;
    __shared__ int32_t s_at, s_fr;
    __shared__ int32_t s_ninf, s_stale, s_cnt;
    __shared__ double s_gp[WAVES];
    if (tid == 0) {
        S.it = st->iter;
        S.limit = st->limit;
        S.status = st->status;
        S.y_buf = st->y_buf;
        S.cnt = st->nb_count;
        S.fresh = D.rec->fresh;
        S.p = D.rec->p;
        S.d_p = D.rec->d_p;
        s_ninf = X.ph->ninf;
        s_stale = X.ph->y_stale;
        s_cnt = 0;
    }
    __syncthreads();
    const int64_t it = S.it;
    if (S.status != ST_RUNNING || it >= S.limit || !S.fresh) {
        if (tid == 0) {
            E.se->need_tau = 0;
            // the pass that found the optimum, or no phase-1 candidate, applied the pending recurrence in its pricing
            if (S.status == ST_OPTIMAL || S.status == ST_INFEASIBLE) E.se->pend = 0;
        }
        return;
    }
    const bool ph1 = s_ninf > 0;
    const double ftol = X.feas_tol;

    double bv = INFINITY;
    int64_t bi = INT64_MAX;
    for (int g = tid; g < D.update_grid; g += BLOCK) {
        const ArgMinEntry v = D.rparts[g];
        if (argmin_better(v.val, v.idx, bv, bi)) {
            bv = v.val;
            bi = v.idx;
        }
    }
    wave_argmin(bv, bi);
    if (lane == 0) s_red[wave] = ArgMinEntry{bv, bi};
    __syncthreads();
    if (tid == 0) {
        ArgMinEntry t = s_red[0];
        for (int w = 1; w < WAVES; ++w)
            if (argmin_better(s_red[w].val, s_red[w].idx, t.val, t.idx)) t = s_red[w];
        s_win = t;
        s_up = D.ub[S.p];
        s_at = D.at_upper[S.p];
        s_fr = F.is_free[S.p];
    }
    __syncthreads();
    const double tq = s_win.val;
    const bool none = s_win.idx == INT64_MAX;
    const int64_t q = none ? 0 : (s_win.idx >> 1);
    const int side = none ? 0 : (int)(s_win.idx & 1);
    const int64_t p = S.p;
    const double u_p = s_up;
    const int up_p = s_at;
    const bool fr_p = s_fr != 0;
    const double sg = fr_p ? (S.d_p < 0.0 ? 1.0 : -1.0) : (up_p ? -1.0 : 1.0);
    const double* al = ((it + 1) & 1) ? P.alpha1 : P.alpha0;
    double* a_cur = (it & 1) ? P.alpha1 : P.alpha0;
    const bool flip = u_p < INFINITY && (none || u_p <= tq);  // (a free column: u_p = +inf)

    if (flip || none) {
        if (flip) {
            const double dx = up_p ? -u_p : u_p;
            const double* Ap = P.A + p * L;
            int bad = 0;
            for (int64_t i = tid; i < m; i += BLOCK) {
                const double xn = fma(-u_p, sg * al[i], P.x_b[i]);
                P.x_b[i] = xn;
                D.b_eff[i] = fma(-dx, Ap[i], D.b_eff[i]);
                if (ph1) {
                    const double wv = row_class_f(xn, F.lb_B[i], D.ub_B[i], ftol);
                    X.w[i] = wv;
                    bad += wv != 0.0;
                }
            }
            if (ph1 && bad) atomicAdd(&s_cnt, bad);  // (an integer count: order-free)
        }
        for (int64_t i = tid; i < L; i += BLOCK) a_cur[i] = (i == 0) ? 1.0 : 0.0;
        __syncthreads();
        if (tid == 0) {
            if (flip) {
                D.at_upper[p] = up_p ? 0 : 1;
                D.rec->flips += 1;
                if (ph1) {
                    X.ph->ninf = s_cnt;
                    X.ph->passes += 1;
                }
            } else {
                st->status = ph1 ? ST_BREAKDOWN : ST_UNBOUNDED;
            }
            if (!ph1 && s_stale) X.ph->y_stale = 0;
            st->q = 0;
            st->aq = 1.0;
            st->p = p;
            st->min_e = S.d_p;
            D.rec->fresh = 0;
            E.se->pend = 0;  // (this pass's pricing applied it; a flip changes no weight)
            E.se->need_tau = 0;
        }
        return;
    }

    // pivot it
    double* y = S.y_buf ? P.y1 : P.y0;
    const double aq = al[q];
    const double theta = tq, sy = -(S.d_p / aq);
    const double x_off = up_p ? u_p : 0.0;  // (a free column sits at 0 and is never at upper)
    const double l_p = fr_p ? -INFINITY : 0.0;
    const bool book = tid == BLOCK - 64;
    int64_t leave = -1;
    double c_p = 0.0;
    int kp = -1, last = -1;
    if (book) {
        leave = P.b_ixs[q];
        c_p = P.c[p];
        kp = P.nb_pos[p];
        last = P.nb_list[S.cnt - 1];
    }
    // ||alpha||^2: a thread's rows ascending, one butterfly, the waves in order (k_pbox_step_se's)
    double a2 = 0.0;
    for (int64_t i = tid; i < m; i += BLOCK) a2 = fma(al[i], al[i], a2);
    a2 = wave_sum(a2);
    if (lane == 0) s_gp[wave] = a2;
    const double* Sq = P.B0 + q * L;
    int bad = 0;
    for (int64_t i0 = tid; i0 < L; i0 += (int64_t)CH * BLOCK) {
        double xv[CH], av[CH], yv[CH], rv[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t i = i0 + (int64_t)u * BLOCK;
            xv[u] = i < m ? P.x_b[i] : 0.0;
            av[u] = i < m ? al[i] : 0.0;
            yv[u] = i < L ? y[i] : 0.0;
            rv[u] = i < L ? Sq[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t i = i0 + (int64_t)u * BLOCK;
            if (i < m) {
                const double xn = (i == q) ? x_off + sg * theta : fma(-theta, sg * av[u], xv[u]);
                P.x_b[i] = xn;
                if (ph1) {  // (row q's bounds are the entering column's: the bookkeeping lane stores them below)
                    const double wv = row_class_f(xn, i == q ? l_p : F.lb_B[i], i == q ? u_p : D.ub_B[i], ftol);
                    X.w[i] = wv;
                    bad += wv != 0.0;
                }
            }
            if (i < L) {
                if (!ph1) y[i] = fma(sy, rv[u], yv[u]);
                P.rbuf[i] = rv[u];
                E.rho[i] = rv[u];  // the weight update's own copy
            }
        }
    }
    if (ph1 && bad) atomicAdd(&s_cnt, bad);
    __syncthreads();
    if (book) {
        double t = s_gp[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) t += s_gp[w];
        const double gp = 1.0 + t;
        const double gl = gp / (aq * aq);
        E.gamma[leave] = gl > 1.0 ? gl : 1.0;
        E.se->aq = aq;
        E.se->gp = gp;
        E.se->leave = leave;
        E.se->pend = 1;
        E.se->need_tau = 1;
        P.c_B[q] = c_p;
        P.b_ixs[q] = p;
        D.ub_B[q] = u_p;
        F.lb_B[q] = l_p;
        D.at_upper[p] = 0;
        D.at_upper[leave] = (int8_t)side;
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
        st->y_applied = it + 1;
        st->xb_applied = it + 1;
        st->p = p;
        st->q = q;
        st->min_e = S.d_p;
        st->iter = it + 1;
        record_pivot(P, it, p, q);
        D.rec->fresh = 0;
        if (side) D.rec->to_upper += 1;
        if (ph1) {
            X.ph->ninf = s_cnt;
            X.ph->passes += 1;
            X.ph->pivots += 1;
            X.ph->y_stale = 1;
        } else if (s_stale) {
            X.ph->y_stale = 0;
        }
    }
}

// ---------------------------------------------------------------------------
// Phase 1's long-step ratio test: the walk past breakpoints
// ---------------------------------------------------------------------------
namespace {

// row i's entries: the soft breakpoint (an infeasible row reaches the bound it
// violates: k_pbox_update1's / _update_f's own entry, same operands, same
// operations) and the hard one (a feasible row's entry of those kernels, or the
// far bound of a row that has a soft breakpoint); idx INT64_MAX = none
template <bool FREE>
__device__ __forceinline__ void long_entries(int64_t i, double ah, double xi, double ubi, double lbi, double wi,
                                             double ptol, double& st, int64_t& si, double& ht, int64_t& hi) {
    st = ht = INFINITY;
    si = hi = INT64_MAX;
    if (wi == 0.0) {
        if (ah > ptol && (!FREE || lbi > -INFINITY)) {
            ht = (xi > 0.0 ? xi : 0.0) / ah;
            hi = 2 * i;
        } else if (ah < -ptol && ubi < INFINITY) {
            const double gap = ubi - xi;
            ht = (gap > 0.0 ? gap : 0.0) / (-ah);
            hi = 2 * i + 1;
        }
    } else if (wi > 0.0) {  // below: rises to 0 (soft), then to its upper bound (hard)
        if (ah < -ptol) {
            st = xi / ah;
            si = 2 * i;
            if (ubi < INFINITY) {
                ht = (xi - ubi) / ah;
                hi = 2 * i + 1;
            }
        }
    } else {  // above: falls to its upper bound (soft), then to 0 (hard)
        if (ah > ptol) {
            st = (xi - ubi) / ah;
            si = 2 * i + 1;
            ht = xi / ah;
            hi = 2 * i;
        }
    }
}

}  // namespace

// One workgroup, between k_pbox_update1 / k_pbox_update_f and the step kernel,
// phase-1 passes only (it returns at once under the step kernels' own return
// conditions and when ninf == 0).  The sum of violations is piecewise linear
// along the entering direction with slope sigma_p d_p < 0 at t = 0; it gains
// |ahat_i| where row i reaches the bound it violates.  h = the hard minimum in
// (t, 2 row + side) order; the soft breakpoints before h are compacted into LDS,
// sorted by rank (the keys are distinct: one per row), and thread 0 adds their
// |ahat| in that order: the first with slope >= -eps leaves; none: h leaves, or
// with no hard entry the last soft one.  The leaving entry goes to rparts[0] and
// "none" to every other slot, so the step kernels, which take their winner from
// rparts only, run unchanged.  More than G.cap soft breakpoints: rounds of
// argmin over the rows strictly beyond the last one taken, read from global
// memory; thread 0 sees the same entries in the same order with the same
// |ahat|, so both paths select the same row.  Every loop bound is m or the list
// count; nothing here waits on another workgroup.
template <bool FREE>
__global__ __launch_bounds__(PBOX_LONG_BLOCK) void k_pbox_long1(Params P, PboxArgs D, Pbox1Args X, PboxFreeArgs F,
                                                                PboxLongArgs G) {
    constexpr int BLOCK = PBOX_LONG_BLOCK, WAVES = BLOCK / 64, PER = PBOX_LONG_CAP / BLOCK;
    __shared__ double s_t[PBOX_LONG_CAP];
    __shared__ double s_a[PBOX_LONG_CAP];
    __shared__ int64_t s_i[PBOX_LONG_CAP];
    __shared__ ArgMinEntry s_red[WAVES];
    __shared__ ArgMinEntry s_win;
    __shared__ PboxSnap S;
    __shared__ int32_t s_ninf, s_cnt, s_done;
    const DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = P.m;
    if (tid == 0) {
        S.it = st->iter;
        S.limit = st->limit;
        S.status = st->status;
        S.fresh = D.rec->fresh;
        S.p = D.rec->p;
        S.d_p = D.rec->d_p;
        s_ninf = X.ph->ninf;
        s_cnt = 0;
        s_done = 0;
    }
    __syncthreads();
    const int64_t it = S.it;
    if (S.status != ST_RUNNING || it >= S.limit || !S.fresh || s_ninf <= 0) return;
    const int64_t p = S.p;
    bool fr_p = false;
    if constexpr (FREE) fr_p = F.is_free[p] != 0;
    const double sg = fr_p ? (S.d_p < 0.0 ? 1.0 : -1.0) : (D.at_upper[p] ? -1.0 : 1.0);
    const double* al = ((it + 1) & 1) ? P.alpha1 : P.alpha0;  // this pass's alpha (the step kernels' `al`)
    const double ptol = D.piv_tol;
    const int cap = G.cap < PBOX_LONG_CAP ? G.cap : PBOX_LONG_CAP;

    auto entries = [&](int64_t i, double& t1, int64_t& i1, double& t2, int64_t& i2, double& aa) {
        const double ah = sg * al[i];
        double lbi = 0.0;
        if constexpr (FREE) lbi = F.lb_B[i];
        long_entries<FREE>(i, ah, P.x_b[i], D.ub_B[i], lbi, X.w[i], ptol, t1, i1, t2, i2);
        aa = fabs(ah);
    };
    // the workgroup's (value, index) argmin; every thread returns with it in s_win
    auto block_argmin = [&](double v, int64_t j) {
        wave_argmin(v, j);
        if (lane == 0) s_red[wave] = ArgMinEntry{v, j};
        __syncthreads();
        if (tid == 0) {
            ArgMinEntry t = s_red[0];
            for (int w = 1; w < WAVES; ++w)
                if (argmin_better(s_red[w].val, s_red[w].idx, t.val, t.idx)) t = s_red[w];
            s_win = t;
        }
        __syncthreads();
    };

    // h: the hard minimum
    double hv = INFINITY;
    int64_t hj = INT64_MAX;
    for (int64_t i = tid; i < m; i += BLOCK) {
        double t1, t2, aa;
        int64_t i1, i2;
        entries(i, t1, i1, t2, i2, aa);
        if (argmin_better(t2, i2, hv, hj)) {
            hv = t2;
            hj = i2;
        }
    }
    block_argmin(hv, hj);
    hv = s_win.val;
    hj = s_win.idx;
    // the soft breakpoints before h, in any order (slots 0 .. cap - 1 are stored, all are counted)
    for (int64_t i = tid; i < m; i += BLOCK) {
        double t1, t2, aa;
        int64_t i1, i2;
        entries(i, t1, i1, t2, i2, aa);
        if (i1 != INT64_MAX && argmin_better(t1, i1, hv, hj)) {
            const int k = atomicAdd(&s_cnt, 1);  // (an integer count: order-free; the sort below fixes the order)
            if (k < cap) {
                s_t[k] = t1;
                s_i[k] = i1;
                s_a[k] = aa;
            }
        }
    }
    __syncthreads();
    const int cnt = s_cnt;  // <= m

    double slope = sg * S.d_p;  // thread 0's
    int64_t npass = 0;
    ArgMinEntry win{hv, hj};  // thread 0's: h, or none, unless the walk finds a row
    if (cnt <= cap) {
        double kt[PER], ka[PER];
        int64_t ki[PER];
        int rk[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + u * BLOCK;
            rk[u] = -1;
            if (e < cnt) {
                kt[u] = s_t[e];
                ki[u] = s_i[e];
                ka[u] = s_a[e];
                int r = 0;
                for (int f = 0; f < cnt; ++f) r += argmin_better(s_t[f], s_i[f], kt[u], ki[u]) ? 1 : 0;
                rk[u] = r;  // 0 <= r < cnt: the entries strictly before this one
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            if (rk[u] >= 0) {
                s_t[rk[u]] = kt[u];
                s_i[rk[u]] = ki[u];
                s_a[rk[u]] = ka[u];
            }
        }
        __syncthreads();
        if (tid == 0) {
            bool found = false;
            for (int k = 0; k < cnt; ++k) {
                slope += s_a[k];
                if (slope >= -P.eps) {
                    win = ArgMinEntry{s_t[k], s_i[k]};
                    found = true;
                    break;
                }
                ++npass;
            }
            if (!found && hj == INT64_MAX && cnt > 0) {  // no hard entry: the last soft breakpoint leaves
                win = ArgMinEntry{s_t[cnt - 1], s_i[cnt - 1]};
                --npass;
            }
        }
    } else {
        double lastv = -INFINITY;  // (every t is >= 0)
        int64_t lastj = -1;
        for (int round = 0; round < cnt; ++round) {
            double bv = INFINITY;
            int64_t bj = INT64_MAX;
            for (int64_t i = tid; i < m; i += BLOCK) {
                double t1, t2, aa;
                int64_t i1, i2;
                entries(i, t1, i1, t2, i2, aa);
                if (i1 != INT64_MAX && argmin_better(t1, i1, hv, hj) && argmin_better(lastv, lastj, t1, i1) &&
                    argmin_better(t1, i1, bv, bj)) {
                    bv = t1;
                    bj = i1;
                }
            }
            block_argmin(bv, bj);  // (round < cnt: an entry is left, 0 <= idx < 2 m)
            if (tid == 0) {
                if (s_win.idx == INT64_MAX) {  // (not reached: cnt entries were counted)
                    s_done = 1;
                } else if ((slope += fabs(al[s_win.idx >> 1])) >= -P.eps) {
                    win = s_win;
                    s_done = 1;
                } else if (round == cnt - 1 && hj == INT64_MAX) {
                    win = s_win;
                } else {
                    ++npass;
                }
            }
            lastv = s_win.val;
            lastj = s_win.idx;
            __syncthreads();  // (s_done; also fences the next round's stores to s_red and s_win)
            if (s_done) break;
        }
    }
    __syncthreads();
    if (tid == 0) {
        s_win = win;
        PboxLongRec* r = G.lrec;
        if (npass > 0) {
            r->passed += npass;
            r->passes += 1;
            if (npass > r->max_pass) r->max_pass = npass;
        }
    }
    __syncthreads();
    const ArgMinEntry out = s_win;
    for (int g = tid; g < D.update_grid; g += BLOCK) D.rparts[g] = g == 0 ? out : ArgMinEntry{INFINITY, INT64_MAX};
}

// ---------------------------------------------------------------------------
// Host-side launchers
// ---------------------------------------------------------------------------
namespace {

constexpr size_t PBOX_LDS_CAP = 150 * 1024;

template <typename K>
hipError_t set_lds(K kernel, size_t lds) {
    if (lds <= 65536) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds);
}

template <typename K>
hipError_t launch_timed(K kernel, int grid, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1, const Params& P,
                        const PboxArgs& D) {
    if (e0 || e1) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(PBOX_BLOCK), (uint32_t)lds, s, e0, e1, 0, P, D);
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(PBOX_BLOCK), lds, s, P, D);
    return hipGetLastError();
}

}  // namespace

hipError_t pbox_prepare(const Params& P, int cus, int price_grid_opt, bool global_y, size_t lds_cap_opt, PboxCfg* cfg) {
    const size_t vec1 = (size_t)P.L * 8;   // y
    const size_t vec2 = (size_t)P.L * 16;  // the pending row and A_p
    const size_t lds_cap = lds_cap_opt > 0 && lds_cap_opt < PBOX_LDS_CAP ? lds_cap_opt : PBOX_LDS_CAP;
    cfg->price_lds = !global_y && vec1 <= lds_cap;
    cfg->update_lds = vec2 <= lds_cap;
    hipError_t e = hipSuccess;
    int per_cu = 0;
    if (cfg->price_lds) {
        e = set_lds(k_pbox_price<true>, vec1);
        if (e == hipSuccess)
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pbox_price<true>, PBOX_BLOCK, vec1);
    } else {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pbox_price<false>, PBOX_BLOCK, 0);
    }
    if (e != hipSuccess) return e;
    if (cfg->update_lds) {
        e = set_lds(k_pbox_update<true>, vec2);
        if (e != hipSuccess) return e;
        e = set_lds(k_pbox_update1<true>, vec2);
        if (e != hipSuccess) return e;
    }
    if (cfg->price_lds) {  // (the phase-1 capable pricing runs on k_pbox_price's grid)
        e = set_lds(k_pbox_price1<true>, vec1);
        if (e != hipSuccess) return e;
    }
    // k_pbox_vtb: a wave per 1 KiB column chunk and row block -- from m alone
    const int nch = (int)(P.L >> 7);
    cfg->vtb_grid_x = (nch + PBOX_VTB_WAVES - 1) / PBOX_VTB_WAVES;
    cfg->vtb_blocks = (int)((P.m + PBOX_VTB_ROWS - 1) / PBOX_VTB_ROWS);
    cfg->vsum_grid = nch;  // k_pbox_vtb_sum: a workgroup per chunk
    if (per_cu < 1) per_cu = 1;
    const int64_t cols = P.n - P.m;  // the non-basic count never changes
    const int64_t want = (cols + PBOX_WAVES - 1) / PBOX_WAVES;
    const int64_t cap = (int64_t)cus * per_cu;
    int64_t g = want < cap ? want : cap;
    if (g < 1) g = 1;
    cfg->price_grid = price_grid_opt > 0 ? price_grid_opt : (int)g;
    cfg->update_grid = (int)((P.m + PBOX_WAVES - 1) / PBOX_WAVES);
    return hipSuccess;
}

hipError_t launch_pbox_price(const Params& P, const PboxArgs& D, const PboxCfg& c, hipStream_t s, hipEvent_t e0,
                             hipEvent_t e1) {
    if (c.price_lds) return launch_timed(k_pbox_price<true>, c.price_grid, (size_t)P.L * 8, s, e0, e1, P, D);
    return launch_timed(k_pbox_price<false>, c.price_grid, 0, s, e0, e1, P, D);
}

hipError_t launch_pbox_update(const Params& P, const PboxArgs& D, const PboxCfg& c, hipStream_t s, hipEvent_t e0,
                              hipEvent_t e1) {
    if (c.update_lds) return launch_timed(k_pbox_update<true>, c.update_grid, (size_t)P.L * 16, s, e0, e1, P, D);
    return launch_timed(k_pbox_update<false>, c.update_grid, 0, s, e0, e1, P, D);
}

hipError_t launch_pbox_step(const Params& P, const PboxArgs& D, hipStream_t s) {
    hipLaunchKernelGGL(k_pbox_step, dim3(1), dim3(1024), 0, s, P, D);
    return hipGetLastError();
}

hipError_t launch_pbox_vtb(const Params& P, const Pbox1Args& X, const PboxCfg& c, hipStream_t s, hipEvent_t e0,
                           hipEvent_t e1) {
    if (e0) {
        const hipError_t e = hipEventRecord(e0, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_pbox_vtb, dim3(c.vtb_grid_x, c.vtb_blocks), dim3(PBOX_VTB_BLOCK), 0, s, P, X);
    hipLaunchKernelGGL(k_pbox_vtb_sum, dim3(c.vsum_grid), dim3(PBOX_VTB_BLOCK), 0, s, P, X);
    if (e1) {
        const hipError_t e = hipEventRecord(e1, s);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

namespace {

template <typename K>
hipError_t launch_timed1(K kernel, int grid, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1, const Params& P,
                         const PboxArgs& D, const Pbox1Args& X) {
    if (e0 || e1) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(PBOX_BLOCK), (uint32_t)lds, s, e0, e1, 0, P, D, X);
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(PBOX_BLOCK), lds, s, P, D, X);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pbox_price1(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxCfg& c, hipStream_t s,
                              hipEvent_t e0, hipEvent_t e1) {
    if (c.price_lds) return launch_timed1(k_pbox_price1<true>, c.price_grid, (size_t)P.L * 8, s, e0, e1, P, D, X);
    return launch_timed1(k_pbox_price1<false>, c.price_grid, 0, s, e0, e1, P, D, X);
}

hipError_t launch_pbox_update1(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxCfg& c, hipStream_t s,
                               hipEvent_t e0, hipEvent_t e1) {
    if (c.update_lds) return launch_timed1(k_pbox_update1<true>, c.update_grid, (size_t)P.L * 16, s, e0, e1, P, D, X);
    return launch_timed1(k_pbox_update1<false>, c.update_grid, 0, s, e0, e1, P, D, X);
}

hipError_t launch_pbox_step1(const Params& P, const PboxArgs& D, const Pbox1Args& X, hipStream_t s) {
    hipLaunchKernelGGL(k_pbox_step1, dim3(1), dim3(1024), 0, s, P, D, X);
    return hipGetLastError();
}

hipError_t launch_pbox_classify(const Params& P, const PboxArgs& D, const Pbox1Args& X, bool entry, hipStream_t s) {
    hipLaunchKernelGGL(k_pbox_classify, dim3(1), dim3(1024), 0, s, P, D, X, entry ? 1 : 0);
    return hipGetLastError();
}

namespace {

template <typename K>
hipError_t launch_timed_f(K kernel, int grid, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1, const Params& P,
                          const PboxArgs& D, const Pbox1Args& X, const PboxFreeArgs& F) {
    if (e0 || e1) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(PBOX_BLOCK), (uint32_t)lds, s, e0, e1, 0, P, D, X, F);
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(PBOX_BLOCK), lds, s, P, D, X, F);
    return hipGetLastError();
}

}  // namespace

hipError_t pbox_free_prepare(const Params& P, const PboxCfg& c) {
    hipError_t e = hipSuccess;
    if (c.price_lds) e = set_lds(k_pbox_price_f<true>, (size_t)P.L * 8);
    if (e == hipSuccess && c.update_lds) e = set_lds(k_pbox_update_f<true>, (size_t)P.L * 16);
    return e;
}

hipError_t launch_pbox_price_f(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxFreeArgs& F,
                               const PboxCfg& c, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (c.price_lds) return launch_timed_f(k_pbox_price_f<true>, c.price_grid, (size_t)P.L * 8, s, e0, e1, P, D, X, F);
    return launch_timed_f(k_pbox_price_f<false>, c.price_grid, 0, s, e0, e1, P, D, X, F);
}

hipError_t launch_pbox_update_f(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxFreeArgs& F,
                                const PboxCfg& c, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (c.update_lds) return launch_timed_f(k_pbox_update_f<true>, c.update_grid, (size_t)P.L * 16, s, e0, e1, P, D, X, F);
    return launch_timed_f(k_pbox_update_f<false>, c.update_grid, 0, s, e0, e1, P, D, X, F);
}

hipError_t launch_pbox_step_f(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxFreeArgs& F,
                              hipStream_t s) {
    hipLaunchKernelGGL(k_pbox_step_f, dim3(1), dim3(1024), 0, s, P, D, X, F);
    return hipGetLastError();
}

hipError_t launch_pbox_classify_f(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxFreeArgs& F,
                                  bool entry, hipStream_t s) {
    hipLaunchKernelGGL(k_pbox_classify_f, dim3(1), dim3(1024), 0, s, P, D, X, F, entry ? 1 : 0);
    return hipGetLastError();
}

namespace {

template <typename K>
hipError_t launch_timed_se(K kernel, int grid, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1,
                           const Params& P, const PboxArgs& D, const PboxSeArgs& E) {
    if (e0 || e1) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(PBOX_BLOCK), (uint32_t)lds, s, e0, e1, 0, P, D, E);
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(PBOX_BLOCK), lds, s, P, D, E);
    return hipGetLastError();
}

}  // namespace

hipError_t pbox_se_prepare(const Params& P, int cus, int price_grid, bool global_y, int lds_vecs_opt, size_t lds_cap_opt,
                           PboxSeCfg* cfg) {
    const size_t vec = (size_t)P.L * 8;
    const size_t lds_cap = lds_cap_opt > 0 && lds_cap_opt < PBOX_LDS_CAP ? lds_cap_opt : PBOX_LDS_CAP;
    int nl = lds_vecs_opt < 0 ? 3 : lds_vecs_opt;  // the default: all three in LDS where they fit
    if (global_y) nl = 0;
    if (nl == 3 && 3 * vec > lds_cap) nl = 1;
    if (nl >= 1 && vec > lds_cap) nl = 0;
    nl = nl >= 3 ? 3 : (nl >= 1 ? 1 : 0);
    cfg->lds_vecs = nl;
    hipError_t e = hipSuccess;
    if (nl == 3) e = set_lds(k_pbox_price_se<3>, 3 * vec);
    else if (nl == 1) e = set_lds(k_pbox_price_se<1>, vec);
    if (e != hipSuccess) return e;
    int per_cu = 0;
    if (nl == 3) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pbox_price_se<3>, PBOX_BLOCK, 3 * vec);
    else if (nl == 1) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pbox_price_se<1>, PBOX_BLOCK, vec);
    else e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pbox_price_se<0>, PBOX_BLOCK, 0);
    if (e != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    const int64_t cols = P.n - P.m;
    const int64_t want = (cols + PBOX_WAVES - 1) / PBOX_WAVES;
    const int64_t cap = (int64_t)cus * per_cu;
    int64_t g = want < cap ? want : cap;
    if (g < 1) g = 1;
    // (the partials live in PboxArgs::parts, sized for price_grid: never more workgroups than that)
    cfg->price_grid = g < price_grid ? (int)g : price_grid;
    const int64_t wi = (P.n + PBOX_WAVES - 1) / PBOX_WAVES;
    const int64_t ci = (int64_t)cus * 4;
    cfg->init_grid = (int)(wi < ci ? wi : ci);
    if (cfg->init_grid < 1) cfg->init_grid = 1;
    return hipSuccess;
}

hipError_t launch_pbox_se_init(const Params& P, const PboxSeArgs& E, const PboxSeCfg& c, hipStream_t s) {
    hipLaunchKernelGGL(k_pbox_se_init, dim3(c.init_grid), dim3(PBOX_BLOCK), 0, s, P, E);
    return hipGetLastError();
}

hipError_t launch_pbox_price_se(const Params& P, const PboxArgs& D, const PboxSeArgs& E, const PboxSeCfg& c, bool apply,
                                hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    PboxSeArgs a = E;
    a.apply = apply ? 1 : 0;
    const size_t vec = (size_t)P.L * 8;
    if (c.lds_vecs == 3) return launch_timed_se(k_pbox_price_se<3>, c.price_grid, 3 * vec, s, e0, e1, P, D, a);
    if (c.lds_vecs == 1) return launch_timed_se(k_pbox_price_se<1>, c.price_grid, vec, s, e0, e1, P, D, a);
    return launch_timed_se(k_pbox_price_se<0>, c.price_grid, 0, s, e0, e1, P, D, a);
}

hipError_t launch_pbox_step_se(const Params& P, const PboxArgs& D, const PboxSeArgs& E, hipStream_t s) {
    hipLaunchKernelGGL(k_pbox_step_se, dim3(1), dim3(1024), 0, s, P, D, E);
    return hipGetLastError();
}

hipError_t launch_pbox_tau(const Params& P, const PboxSeArgs& E, const PboxCfg& c, hipStream_t s, hipEvent_t e0,
                           hipEvent_t e1) {
    if (e0) {
        const hipError_t e = hipEventRecord(e0, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_pbox_tau, dim3(c.vtb_grid_x, c.vtb_blocks), dim3(PBOX_VTB_BLOCK), 0, s, P, E);
    hipLaunchKernelGGL(k_pbox_tau_sum, dim3(c.vsum_grid), dim3(PBOX_VTB_BLOCK), 0, s, P, E);
    if (e1) {
        const hipError_t e = hipEventRecord(e1, s);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

hipError_t pbox_se1_prepare(const Params& P, const PboxSeCfg& c) {
    const size_t vec = (size_t)P.L * 8;
    if (c.lds_vecs == 3) return set_lds(k_pbox_price_se1<3>, 3 * vec);
    if (c.lds_vecs == 1) return set_lds(k_pbox_price_se1<1>, vec);
    return hipSuccess;
}

hipError_t launch_pbox_price_se1(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxSeArgs& E,
                                 const PboxSeCfg& c, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    const size_t vec = (size_t)P.L * 8;
    const size_t lds = c.lds_vecs == 3 ? 3 * vec : (c.lds_vecs == 1 ? vec : 0);
    auto kernel = c.lds_vecs == 3 ? k_pbox_price_se1<3> : (c.lds_vecs == 1 ? k_pbox_price_se1<1> : k_pbox_price_se1<0>);
    if (e0 || e1)
        hipExtLaunchKernelGGL(kernel, dim3(c.price_grid), dim3(PBOX_BLOCK), (uint32_t)lds, s, e0, e1, 0, P, D, X, E);
    else hipLaunchKernelGGL(kernel, dim3(c.price_grid), dim3(PBOX_BLOCK), lds, s, P, D, X, E);
    return hipGetLastError();
}

hipError_t launch_pbox_step_se1(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxSeArgs& E,
                                hipStream_t s) {
    hipLaunchKernelGGL(k_pbox_step_se1, dim3(1), dim3(1024), 0, s, P, D, X, E);
    return hipGetLastError();
}

hipError_t pbox_se_f_prepare(const Params& P, const PboxSeCfg& c) {
    const size_t vec = (size_t)P.L * 8;
    if (c.lds_vecs == 3) return set_lds(k_pbox_price_se_f<3>, 3 * vec);
    if (c.lds_vecs == 1) return set_lds(k_pbox_price_se_f<1>, vec);
    return hipSuccess;
}

hipError_t launch_pbox_price_se_f(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxSeArgs& E,
                                  const PboxFreeArgs& F, const PboxSeCfg& c, hipStream_t s, hipEvent_t e0,
                                  hipEvent_t e1) {
    const size_t vec = (size_t)P.L * 8;
    const size_t lds = c.lds_vecs == 3 ? 3 * vec : (c.lds_vecs == 1 ? vec : 0);
    auto kernel =
        c.lds_vecs == 3 ? k_pbox_price_se_f<3> : (c.lds_vecs == 1 ? k_pbox_price_se_f<1> : k_pbox_price_se_f<0>);
    if (e0 || e1)
        hipExtLaunchKernelGGL(kernel, dim3(c.price_grid), dim3(PBOX_BLOCK), (uint32_t)lds, s, e0, e1, 0, P, D, X, E, F);
    else hipLaunchKernelGGL(kernel, dim3(c.price_grid), dim3(PBOX_BLOCK), lds, s, P, D, X, E, F);
    return hipGetLastError();
}

hipError_t launch_pbox_step_se_f(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxSeArgs& E,
                                 const PboxFreeArgs& F, hipStream_t s) {
    hipLaunchKernelGGL(k_pbox_step_se_f, dim3(1), dim3(1024), 0, s, P, D, X, E, F);
    return hipGetLastError();
}

hipError_t launch_pbox_stage(const Params& P, hipStream_t s) {
    hipLaunchKernelGGL(k_pbox_stage, dim3(1), dim3(1024), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_pbox_long1(const Params& P, const PboxArgs& D, const Pbox1Args& X, const PboxFreeArgs* F,
                             const PboxLongArgs& G, hipStream_t s) {
    if (F) hipLaunchKernelGGL(k_pbox_long1<true>, dim3(1), dim3(PBOX_LONG_BLOCK), 0, s, P, D, X, *F, G);
    else hipLaunchKernelGGL(k_pbox_long1<false>, dim3(1), dim3(PBOX_LONG_BLOCK), 0, s, P, D, X, PboxFreeArgs{}, G);
    return hipGetLastError();
}

}  // namespace spx
