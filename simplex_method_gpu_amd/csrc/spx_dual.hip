// spx_dual.hip — gfx950 kernels of the dual simplex loop (spx_dual.h).
#include "spx_dual.h"

#include <hip/hip_ext.h>

#include <type_traits>

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

template <bool SE>
using DualArgsOf = std::conditional_t<SE, DualSeArgs, DualArgs>;

// what only k_dual_update's steepest-edge instantiations carry (nothing in the Dantzig ones)
template <int SE>
struct SeDots {  // k_dual_update: rho's operand and the two extra dots' accumulators
    const dbl2* xh;
    double t0 = 0.0, t1 = 0.0, w0 = 0.0, w1 = 0.0;
};
template <>
struct SeDots<0> {};

// ... and only its long-step instantiations
template <bool LONG>
struct FlipDots {  // k_dual_update: whether the pass flipped columns, v, and the dot's accumulators
    bool on = false;
    const dbl2* xv;
    double f0 = 0.0, f1 = 0.0;
};
template <>
struct FlipDots<false> {};

}  // namespace

// ---------------------------------------------------------------------------
// Finish of the previous pass's pivot, leaving row, pivot row (one workgroup)
// ---------------------------------------------------------------------------
#define SPX_STEP_KERNEL k_dual_step
#define SPX_STEP_ARGS DualArgs
#define SPX_STEP_SE 0
#define SPX_STEP_BOX 0
#include "spx_dual_step.inc"
#undef SPX_STEP_KERNEL
#undef SPX_STEP_ARGS
#undef SPX_STEP_SE
#define SPX_STEP_KERNEL k_dual_step_se
#define SPX_STEP_ARGS DualSeArgs
#define SPX_STEP_SE 1
#include "spx_dual_step.inc"
#undef SPX_STEP_KERNEL
#undef SPX_STEP_ARGS
#undef SPX_STEP_SE
#undef SPX_STEP_BOX
// boxed variables (0 <= x <= u): Dantzig and steepest edge
#define SPX_STEP_KERNEL k_dual_step_box
#define SPX_STEP_ARGS DualBoxArgs
#define SPX_STEP_SE 0
#define SPX_STEP_BOX 1
#include "spx_dual_step.inc"
#undef SPX_STEP_KERNEL
#undef SPX_STEP_SE
#define SPX_STEP_KERNEL k_dual_step_se_box
#define SPX_STEP_SE 1
#include "spx_dual_step.inc"
#undef SPX_STEP_KERNEL
#undef SPX_STEP_ARGS
#undef SPX_STEP_SE
// ... with the bound-flipping ratio test's flips in the commit
#define SPX_STEP_LONG 1
#define SPX_STEP_KERNEL k_dual_step_long
#define SPX_STEP_ARGS DualLongArgs
#define SPX_STEP_SE 0
#include "spx_dual_step.inc"
#undef SPX_STEP_KERNEL
#undef SPX_STEP_SE
#define SPX_STEP_KERNEL k_dual_step_se_long
#define SPX_STEP_SE 1
#include "spx_dual_step.inc"
#undef SPX_STEP_KERNEL
#undef SPX_STEP_ARGS
#undef SPX_STEP_SE
#undef SPX_STEP_LONG
#undef SPX_STEP_BOX

// ---------------------------------------------------------------------------
// Dual ratio test (the hot kernel): two dots per streamed non-basic column
// ---------------------------------------------------------------------------
// One wave per column, grid-stride over nb_list.  A column is L/2 dbl2 in
// chunks of 64 lanes; U chunks are in flight per wave while the previous U are
// multiplied with rho and y (double-buffered registers), non-temporal as
// k_price's A stream.  Per lane the chunks are accumulated in ascending order
// into four partial sums, then one butterfly: a column's a_j and d_j do not
// depend on the grid or on which wave prices it.
// BOX (0 <= x <= u): with s the pass's direction (DualRec::s) and sigma_j = -1
// for a column at its upper bound (one wave-uniform flag read per column, ahead
// of its stream), candidates are s sigma_j a_j < -piv_tol and the key is
// max(sigma_j d_j, 0) / -(s sigma_j a_j); the partial carries the raw a_j, d_j.
// LONG (BOX with the bound-flipping ratio test): lane 0 also stores the list
// slot's record after the butterfly, key (+inf: no candidate), u_j (-ahat_j)
// and d_j: 24 bytes beside the 8 (m + 1) streamed; u_j is read with the flag.
template <bool LDS, bool BOX, bool LONG = false>
__global__ __launch_bounds__(DUAL_BLOCK) void k_dual_price(
    Params P, std::conditional_t<LONG, DualLongArgs, std::conditional_t<BOX, DualBoxArgs, DualArgs>> D) {
    static_assert(BOX || !LONG, "the long-step ratio test is the boxed one's");
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
    [[maybe_unused]] double dir = 1.0;
    if constexpr (BOX) dir = D.rec->s < 0 ? -1.0 : 1.0;
    for (int s = (int)blockIdx.x * WAVES + wave; s < cnt; s += nwv) {
        const int64_t j = P.nb_list[s];
        [[maybe_unused]] int up = 0;
        if constexpr (BOX) up = D.at_upper[j];
        [[maybe_unused]] double uj = 0.0;
        if constexpr (LONG) uj = D.ub[j];
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
        if constexpr (BOX) {
            const double sg = up ? -1.0 : 1.0;
            const double ah = dir * sg * a, dh = sg * d;  // (sign flips: exact)
            [[maybe_unused]] double rk = INFINITY;
            if (ah < -D.piv_tol) {
                const double key = (dh > 0.0 ? dh : 0.0) / (-ah);
                if constexpr (LONG) rk = key;
                if (argmin_better(key, j, bkey, bidx)) {
                    bkey = key;
                    bidx = j;
                    ba = a;
                    bd = d;
                }
            }
            if constexpr (LONG) {
                if (lane == 0) {  // (s < cnt <= n: the buffers hold n slots)
                    D.rkey[s] = rk;
                    reinterpret_cast<dbl2*>(D.rcd)[s] = dbl2{uj * (-ah), d};
                }
            }
        } else if (a < -D.piv_tol) {
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
// SE (dual steepest edge): the updated row is also dotted with the pivot row
// rho (tau_i) and with itself (the exact weight wex_i), in acc0 / acc1's fixed
// order, so neither depends on the grid.  SE 1 stages rho in LDS beside the
// pending row and A_p (24 L bytes), SE 2 reads it from global memory (L2 hits).
// LONG (the bound-flipping ratio test): p comes from the pass record (k_dual_long
// merged the partials), and when the pass flipped columns the updated row is
// also dotted with v (global memory, L2 hits: a fourth LDS operand would halve
// the occupancy of the passes without flips) into fl, in acc0 / acc1's order;
// the test is wave-uniform and a pass without flips reads nothing more.
template <bool XL, int SE, bool LONG = false>
__global__ __launch_bounds__(DUAL_BLOCK) void k_dual_update(
    Params P, std::conditional_t<LONG, DualLongArgs, DualArgsOf<SE != 0>> D) {
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
        if constexpr (LONG) {
            Sv.p = D.rec->p;
            Sv.cnt = D.lrec->nflip;
        }
    }
    __syncthreads();
    const int64_t it = Sv.it, qp = Sv.qprev;
    const double aqp = Sv.aqprev;
    if (Sv.status != ST_RUNNING || it >= Sv.limit) return;

    // the ratio test's grid step: every workgroup merges the same partials
    // (LONG: k_dual_long did, and left the entering column in the pass record)
    DualPartial w{INFINITY, INT64_MAX, 0.0, 0.0};
    if constexpr (!LONG) {
        for (int g = tid; g < D.price_grid; g += DUAL_BLOCK) {
            const DualPartial v = D.parts[g];
            if (argmin_better(v.key, v.idx, w.key, w.idx)) w = v;
        }
        wave_argmin4(w);
        if (lane == 0) s_red[wave] = w;
        __syncthreads();
    }
    const DualPartial t = LONG ? DualPartial{0.0, Sv.p, 0.0, 0.0} : merge_waves<WAVES>(s_red);
    if (t.idx == INT64_MAX) {  // no a_j < -piv_tol in a row with x_b < 0: primal infeasible
        if (blockIdx.x == 0 && tid == 0) st->status = ST_INFEASIBLE;
        return;
    }
    const int64_t p = t.idx;
    if (blockIdx.x == 0 && tid == 0) {
        if constexpr (!LONG) {
            D.rec->p = p;
            D.rec->d_p = t.d;
        }
        D.rec->fresh = 1;
    }
    [[maybe_unused]] FlipDots<LONG> fd;
    if constexpr (LONG) {
        fd.on = Sv.cnt > 0;
        fd.xv = reinterpret_cast<const dbl2*>(D.v);
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
            if constexpr (SE == 1) d[2 * L2 + k] = reinterpret_cast<const dbl2*>(D.rho)[k];
        }
        __syncthreads();
    }
    const dbl2* xr = XL ? reinterpret_cast<const dbl2*>(dsm) : rp;
    const dbl2* xa = XL ? reinterpret_cast<const dbl2*>(dsm) + L2 : ap;
    [[maybe_unused]] SeDots<SE> se;
    if constexpr (SE != 0)
        se.xh = (XL && SE == 1) ? reinterpret_cast<const dbl2*>(dsm) + 2 * L2 : reinterpret_cast<const dbl2*>(D.rho);

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
                if constexpr (SE != 0) {
                    const dbl2 h = se.xh[k];
                    se.t0 = fma(nv.x, h.x, se.t0);
                    se.t1 = fma(nv.y, h.y, se.t1);
                    se.w0 = fma(nv.x, nv.x, se.w0);
                    se.w1 = fma(nv.y, nv.y, se.w1);
                }
                if constexpr (LONG) {
                    if (fd.on) {
                        const dbl2 vv = fd.xv[k];
                        fd.f0 = fma(nv.x, vv.x, fd.f0);
                        fd.f1 = fma(nv.y, vv.y, fd.f1);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
    const double alpha = wave_sum(acc0 + acc1);
    if (lane == 0) a_new[i] = alpha;
    if constexpr (LONG) {
        if (fd.on) {
            const double f = wave_sum(fd.f0 + fd.f1);
            if (lane == 0) D.fl[i] = f;
        }
    }
    if constexpr (SE != 0) {
        double t = se.t0 + se.t1, w = se.w0 + se.w1;
        wave_sum2(t, w);
        if (lane == 0) {
            D.tau[i] = t;
            D.wex[i] = w;
        }
    }
}

// ---------------------------------------------------------------------------
// Dual steepest-edge weights of the current basis, from scratch
// ---------------------------------------------------------------------------
// One row per wave: w_i = ||S[i] + E_i r'||^2, the pending pivot (r' = S[q'],
// read in place: nothing is written to B^-1) applied in registers, summed in
// k_dual_update's order.  Runs between passes only (DualRec::fresh == 0).
__global__ __launch_bounds__(DUAL_BLOCK) void k_dual_norms(Params P, DualSeArgs D) {
    constexpr int WAVES = DUAL_WAVES;
    const DevState* st = P.st;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t it = st->iter, qp = st->q;
    const double aqp = st->aq;
    const int64_t m = P.m, L = P.L;
    const int nch = (int)(L >> 7);
    const int64_t i = (int64_t)blockIdx.x * WAVES + wave;
    if (i >= m) return;
    const bool pend = it > 0 && qp >= 0 && qp < m;
    const double* a_prev = (it & 1) ? P.alpha1 : P.alpha0;
    const double ei = pend ? eta_entry(a_prev[i], i, qp, aqp) : 0.0;
    const dbl2* row = reinterpret_cast<const dbl2*>(P.B0 + i * L) + lane;
    const dbl2* rp = reinterpret_cast<const dbl2*>(pend ? P.B0 + qp * L : P.zeros) + lane;
    double w0 = 0.0, w1 = 0.0;
    for (int c = 0; c < nch; ++c) {
        const dbl2 s = row[64 * c], r = rp[64 * c];
        const double vx = fma(ei, r.x, s.x), vy = fma(ei, r.y, s.y);
        w0 = fma(vx, vx, w0);
        w1 = fma(vy, vy, w1);
    }
    const double w = wave_sum(w0 + w1);
    if (lane == 0) D.w[i] = fmax(w, DUAL_W_FLOOR);
}

// ---------------------------------------------------------------------------
// Boxed variables: the effective right-hand side and x_b from it
// ---------------------------------------------------------------------------
// One thread per row: b_eff_i = b_i - sum_j u_j A_ij over the non-basic columns
// at their upper bound, in ascending j (a fixed order, no atomics); rows m..L-1
// stay 0.  Also ub_B_i = ub[b_ixs[i]].  Runs between passes, before anything
// that recomputes x_b from P.b.
constexpr int BOX_BLOCK = 256;
__global__ __launch_bounds__(BOX_BLOCK) void k_box_rhs(Params P, DualBoxArgs D, const double* b_user, double* b_eff) {
    const int64_t i = (int64_t)blockIdx.x * BOX_BLOCK + threadIdx.x;
    const int64_t m = P.m, n = P.n, L = P.L;
    if (i >= L) return;
    double acc = i < m ? b_user[i] : 0.0;
    if (i < m) {
        for (int64_t j = 0; j < n; ++j)
            if (D.at_upper[j] && P.nb_pos[j] >= 0) acc = fma(-D.ub[j], P.A[j * L + i], acc);
        D.ub_B[i] = D.ub[P.b_ixs[i]];
    }
    b_eff[i] = acc;
}

// k_box_rhs for shifted variables x'_j = x_j - l_j: b_eff_i = b_i
// - sum_j l_j A_ij - sum_{j non-basic at upper} (u_j - l_j) A_ij, one pass over
// ascending j in which a column is read only where l_j != 0 or it sits at its
// upper bound (its lower term first); D.ub holds u - l.  The same fixed order,
// no atomics; ub_B as k_box_rhs writes it.
__global__ __launch_bounds__(BOX_BLOCK) void k_box_rhs_lu(Params P, DualBoxArgs D, const double* lsh,
                                                          const double* b_user, double* b_eff) {
    const int64_t i = (int64_t)blockIdx.x * BOX_BLOCK + threadIdx.x;
    const int64_t m = P.m, n = P.n, L = P.L;
    if (i >= L) return;
    double acc = i < m ? b_user[i] : 0.0;
    if (i < m) {
        for (int64_t j = 0; j < n; ++j) {
            const double lj = lsh[j];
            const bool up = D.at_upper[j] && P.nb_pos[j] >= 0;
            if (lj == 0.0 && !up) continue;
            const double a = P.A[j * L + i];
            if (lj != 0.0) acc = fma(-lj, a, acc);
            if (up) acc = fma(-D.ub[j], a, acc);
        }
        D.ub_B[i] = D.ub[P.b_ixs[i]];
    }
    b_eff[i] = acc;
}

// One row per wave: x_b_i = (S[i] + E_i r') . b, the pending pivot applied in
// registers as k_dual_norms does (nothing is written to B^-1).
__global__ __launch_bounds__(DUAL_BLOCK) void k_box_xb(Params P) {
    constexpr int WAVES = DUAL_WAVES;
    const DevState* st = P.st;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t it = st->iter, qp = st->q;
    const double aqp = st->aq;
    const int64_t m = P.m, L = P.L;
    const int nch = (int)(L >> 7);
    const int64_t i = (int64_t)blockIdx.x * WAVES + wave;
    if (i >= m) return;
    const bool pend = it > 0 && qp >= 0 && qp < m;
    const double* a_prev = (it & 1) ? P.alpha1 : P.alpha0;
    const double ei = pend ? eta_entry(a_prev[i], i, qp, aqp) : 0.0;
    const dbl2* row = reinterpret_cast<const dbl2*>(P.B0 + i * L) + lane;
    const dbl2* rp = reinterpret_cast<const dbl2*>(pend ? P.B0 + qp * L : P.zeros) + lane;
    const dbl2* bv = reinterpret_cast<const dbl2*>(P.b) + lane;
    double x0 = 0.0, x1 = 0.0;
    for (int c = 0; c < nch; ++c) {
        const dbl2 s = row[64 * c], r = rp[64 * c], b = bv[64 * c];
        x0 = fma(fma(ei, r.x, s.x), b.x, x0);
        x1 = fma(fma(ei, r.y, s.y), b.y, x1);
    }
    const double x = wave_sum(x0 + x1);
    if (lane == 0) P.x_b[i] = x;
}

// ---------------------------------------------------------------------------
// Bound-flipping ratio test: the walk over k_dual_price<., ., true>'s records
// ---------------------------------------------------------------------------
// One workgroup.  Round 0 merges the pricing workgroups' partials (the textbook
// winner); every later round is the argmin over the records strictly beyond the
// last (key, column) taken, so the candidates come in (key, column) order.
// Thread 0 keeps the slope: a candidate with no bound, or whose u_j (-ahat_j)
// takes the slope to 0 or below, enters (at exactly 0 the flips and that column
// at its bound make row q feasible); any other is flipped and the walk goes on.
// A pass without flips is round 0 alone.  The first round that scans loads each
// thread's LONG_SLOTS keys and columns into registers (nb_count <= LONG_SLOTS x
// LONG_BLOCK; beyond that, or with DualLongArgs::walk_global, every round reads
// them from global memory), so a later round costs two reductions and thread
// 0's one round trip for the winner's record.  At most nb_count + 1 rounds
// (every round takes a distinct slot or ends the walk); nothing here waits on
// another workgroup.  No candidate left: ST_INFEASIBLE, no flip applied, no
// counter moved.
constexpr int LONG_BLOCK = 512;
constexpr int LONG_SLOTS = 32;
__global__ __launch_bounds__(LONG_BLOCK) void k_dual_long(Params P, DualLongArgs D) {
    constexpr int WAVES = LONG_BLOCK / 64;
    __shared__ double s_key[WAVES];
    __shared__ int64_t s_j[WAVES];
    __shared__ int32_t s_s[WAVES];
    __shared__ double w_key;
    __shared__ int64_t w_j;
    __shared__ int32_t w_state;  // 0 flipped: go on, 1 entering column found, 2 no candidate left
    DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t status = st->status, cnt = st->nb_count;
    const int64_t iter = st->iter, limit = st->limit;
    if (status != ST_RUNNING || iter >= limit) return;  // (thread 0 stores the status after a barrier only)
    double slope = 0.0;
    int nfl = 0;
    if (tid == 0) {
        const int64_t q = D.rec->q;
        const double xq = P.x_b[q];
        slope = fabs(D.rec->s > 0 ? xq : xq - D.ub_B[q]);  // |delta_q|
    }
    // one round's end: the workgroup's (key, column, slot) argmin, then thread 0's decision
    auto decide = [&](double bk, int64_t bj, int32_t bs) -> int {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double k2 = __shfl_xor(bk, off, 64);
            const int64_t j2 = __shfl_xor(bj, off, 64);
            const int32_t s2 = __shfl_xor(bs, off, 64);
            const bool t = argmin_better(k2, j2, bk, bj);
            bk = t ? k2 : bk;
            bj = t ? j2 : bj;
            bs = t ? s2 : bs;
        }
        if (lane == 0) {
            s_key[wave] = bk;
            s_j[wave] = bj;
            s_s[wave] = bs;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < WAVES; ++w) {
                const bool t = argmin_better(s_key[w], s_j[w], bk, bj);
                bk = t ? s_key[w] : bk;
                bj = t ? s_j[w] : bj;
                bs = t ? s_s[w] : bs;
            }
            if (bj == INT64_MAX) {
                w_state = 2;
            } else {
                const int64_t sl = bs >= 0 ? bs : P.nb_pos[bj];  // its list slot: 0 <= sl < cnt
                const double cap = D.rcd[2 * sl], d = D.rcd[2 * sl + 1];
                const double u = D.ub[bj];
                const int up = D.at_upper[bj];
                const double slope2 = slope - cap;
                if (!(cap < INFINITY) || slope2 <= 0.0) {
                    D.rec->p = bj;
                    D.rec->d_p = d;
                    w_state = 1;
                } else {
                    D.flist[nfl] = DualFlip{bj, up ? -u : u};  // (nfl < cnt <= n)
                    ++nfl;
                    slope = slope2;
                    w_key = bk;
                    w_j = bj;
                    w_state = 0;
                }
            }
        }
        __syncthreads();  // (also fences the next round's stores to s_key .. s_s)
        return w_state;
    };
    // round 0: the partials (slot -1: thread 0 looks it up)
    double bk = INFINITY;
    int64_t bj = INT64_MAX;
    for (int g = tid; g < D.price_grid; g += LONG_BLOCK) {
        const DualPartial v = D.parts[g];
        if (argmin_better(v.key, v.idx, bk, bj)) {
            bk = v.key;
            bj = v.idx;
        }
    }
    int state = decide(bk, bj, -1);
    if (state == 0) {
        double lastk = w_key;
        int64_t lastj = w_j;
        if (!D.walk_global && cnt <= LONG_SLOTS * LONG_BLOCK) {
            double ck[LONG_SLOTS];
            int32_t cj[LONG_SLOTS];
#pragma unroll
            for (int t = 0; t < LONG_SLOTS; ++t) {
                const int s = tid + t * LONG_BLOCK;
                ck[t] = s < cnt ? D.rkey[s] : INFINITY;
                cj[t] = s < cnt ? P.nb_list[s] : INT32_MAX;
            }
            for (int round = 1; round <= cnt && state == 0; ++round) {
                bk = INFINITY;
                bj = INT64_MAX;
                int32_t bs = -1;
#pragma unroll
                for (int t = 0; t < LONG_SLOTS; ++t) {
                    const double k = ck[t];
                    const int64_t j = cj[t];
                    if (k < INFINITY && argmin_better(lastk, lastj, k, j) && argmin_better(k, j, bk, bj)) {
                        bk = k;
                        bj = j;
                        bs = tid + t * LONG_BLOCK;
                    }
                }
                state = decide(bk, bj, bs);
                lastk = w_key;
                lastj = w_j;
            }
        } else {
            for (int round = 1; round <= cnt && state == 0; ++round) {
                bk = INFINITY;
                bj = INT64_MAX;
                int32_t bs = -1;
                for (int s = tid; s < cnt; s += LONG_BLOCK) {
                    const double k = D.rkey[s];
                    const int64_t j = P.nb_list[s];
                    if (k < INFINITY && argmin_better(lastk, lastj, k, j) && argmin_better(k, j, bk, bj)) {
                        bk = k;
                        bj = j;
                        bs = s;
                    }
                }
                state = decide(bk, bj, bs);
                lastk = w_key;
                lastj = w_j;
            }
        }
    }
    if (tid == 0) {
        if (state == 1) {
            DualLongRec* r = D.lrec;
            r->nflip = nfl;
            if (nfl > 0) {
                r->flips += nfl;
                r->passes += 1;
                if (nfl > r->max_pass) r->max_pass = nfl;
            }
        } else {  // every candidate flipped and none enters, or none at all: primal infeasible
            D.lrec->nflip = 0;
            st->status = ST_INFEASIBLE;
        }
    }
}

// The flipped columns' move: v = sum over the flip list, in its order, of dx_j
// A_j, one thread per row (k_box_rhs's form: coalesced in the column-major A, no
// atomics), P.b -= v; workgroup 0 toggles at_upper.  Returns at once when the
// pass flipped nothing (or did not run: k_dual_long's exits).
__global__ __launch_bounds__(BOX_BLOCK) void k_dual_flips(Params P, DualLongArgs D, double* b_eff) {
    const DevState* st = P.st;
    if (st->status != ST_RUNNING || st->iter >= st->limit) return;
    const int nfl = D.lrec->nflip;
    if (nfl <= 0) return;
    const int64_t i = (int64_t)blockIdx.x * BOX_BLOCK + threadIdx.x;
    const int64_t m = P.m, L = P.L;
    if (i < L) {
        double acc = 0.0;
        if (i < m) {
            for (int f = 0; f < nfl; ++f) {
                const DualFlip t = D.flist[f];
                acc = fma(t.dx, P.A[t.j * L + i], acc);
            }
            b_eff[i] -= acc;  // (= P.b, as k_box_rhs writes it)
        }
        D.v[i] = acc;
    }
    if (blockIdx.x == 0)
        for (int f = threadIdx.x; f < nfl; f += BOX_BLOCK) {
            const int64_t j = D.flist[f].j;  // (distinct columns)
            D.at_upper[j] = D.at_upper[j] ? 0 : 1;
        }
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

template <typename K, typename DA>
hipError_t launch_timed(K kernel, int grid, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1, const Params& P,
                        const DA& D) {
    if (e0 || e1) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(DUAL_BLOCK), (uint32_t)lds, s, e0, e1, 0, P, D);
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(DUAL_BLOCK), lds, s, P, D);
    return hipGetLastError();
}

}  // namespace

hipError_t dual_prepare(const Params& P, int cus, int price_grid_opt, bool global_y, bool se_rho_lds,
                        size_t lds_cap_opt, DualCfg* cfg) {
    const size_t vec2 = (size_t)P.L * 16;  // two staged vectors
    const size_t vec3 = (size_t)P.L * 24;  // with rho
    const size_t lds_cap = lds_cap_opt > 0 && lds_cap_opt < DUAL_LDS_CAP ? lds_cap_opt : DUAL_LDS_CAP;
    cfg->price_lds = !global_y && vec2 <= lds_cap;
    cfg->update_lds = vec2 <= lds_cap;
    cfg->se_update_lds = !global_y && vec3 <= lds_cap;
    cfg->se_rho_lds = se_rho_lds;
    hipError_t e = hipSuccess;
    int per_cu = 0;
    if (cfg->price_lds) {
        e = set_lds(k_dual_price<true, false>, vec2);
        if (e == hipSuccess) e = set_lds(k_dual_price<true, true>, vec2);  // (the same grid: DESIGN.md 7d)
        if (e == hipSuccess)
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_dual_price<true, false>, DUAL_BLOCK, vec2);
    } else {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_dual_price<false, false>, DUAL_BLOCK, 0);
    }
    if (e != hipSuccess) return e;
    if (cfg->update_lds) {
        e = set_lds(k_dual_update<true, 0>, vec2);
        if (e != hipSuccess) return e;
    }
    if (cfg->se_update_lds) {
        e = se_rho_lds ? set_lds(k_dual_update<true, 1>, vec3) : set_lds(k_dual_update<true, 2>, vec2);
        if (e != hipSuccess) return e;
    }
    // the long-step instantiations (launched only under SPX_DUAL_RATIO_LONG_STEP with finite bounds)
    if (cfg->price_lds) {
        e = set_lds(k_dual_price<true, true, true>, vec2);
        if (e != hipSuccess) return e;
    }
    if (cfg->update_lds) {
        e = set_lds(k_dual_update<true, 0, true>, vec2);
        if (e != hipSuccess) return e;
    }
    if (cfg->se_update_lds) {
        e = se_rho_lds ? set_lds(k_dual_update<true, 1, true>, vec3) : set_lds(k_dual_update<true, 2, true>, vec2);
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

hipError_t launch_dual_step(const Params& P, const DualBoxArgs& D, bool se, bool box, bool finish_only,
                            hipStream_t s) {
    const DualSeArgs& D1 = D;
    const DualArgs& D0 = D;
    const int fin = finish_only ? 1 : 0;
    if (box && se) hipLaunchKernelGGL(k_dual_step_se_box, dim3(1), dim3(1024), 0, s, P, D, fin);
    else if (box) hipLaunchKernelGGL(k_dual_step_box, dim3(1), dim3(1024), 0, s, P, D, fin);
    else if (se) hipLaunchKernelGGL(k_dual_step_se, dim3(1), dim3(1024), 0, s, P, D1, fin);
    else hipLaunchKernelGGL(k_dual_step, dim3(1), dim3(1024), 0, s, P, D0, fin);
    return hipGetLastError();
}

hipError_t launch_dual_price(const Params& P, const DualBoxArgs& D, const DualCfg& c, bool box, hipStream_t s,
                             hipEvent_t e0, hipEvent_t e1) {
    const size_t lds = c.price_lds ? (size_t)P.L * 16 : 0;
    if (box) {
        if (c.price_lds) return launch_timed(k_dual_price<true, true>, c.price_grid, lds, s, e0, e1, P, D);
        return launch_timed(k_dual_price<false, true>, c.price_grid, 0, s, e0, e1, P, D);
    }
    const DualArgs& D0 = D;
    if (c.price_lds) return launch_timed(k_dual_price<true, false>, c.price_grid, lds, s, e0, e1, P, D0);
    return launch_timed(k_dual_price<false, false>, c.price_grid, 0, s, e0, e1, P, D0);
}

hipError_t launch_dual_update(const Params& P, const DualSeArgs& D, const DualCfg& c, bool se, hipStream_t s,
                              hipEvent_t e0, hipEvent_t e1) {
    if (se) {
        if (!c.se_update_lds) return launch_timed(k_dual_update<false, 2>, c.update_grid, 0, s, e0, e1, P, D);
        if (c.se_rho_lds) return launch_timed(k_dual_update<true, 1>, c.update_grid, (size_t)P.L * 24, s, e0, e1, P, D);
        return launch_timed(k_dual_update<true, 2>, c.update_grid, (size_t)P.L * 16, s, e0, e1, P, D);
    }
    const DualArgs& D0 = D;
    if (c.update_lds) return launch_timed(k_dual_update<true, 0>, c.update_grid, (size_t)P.L * 16, s, e0, e1, P, D0);
    return launch_timed(k_dual_update<false, 0>, c.update_grid, 0, s, e0, e1, P, D0);
}

hipError_t launch_dual_step_long(const Params& P, const DualLongArgs& D, bool se, bool finish_only, hipStream_t s) {
    const int fin = finish_only ? 1 : 0;
    if (se) hipLaunchKernelGGL(k_dual_step_se_long, dim3(1), dim3(1024), 0, s, P, D, fin);
    else hipLaunchKernelGGL(k_dual_step_long, dim3(1), dim3(1024), 0, s, P, D, fin);
    return hipGetLastError();
}

hipError_t launch_dual_price_long(const Params& P, const DualLongArgs& D, const DualCfg& c, hipStream_t s,
                                  hipEvent_t e0, hipEvent_t e1) {
    if (c.price_lds)
        return launch_timed(k_dual_price<true, true, true>, c.price_grid, (size_t)P.L * 16, s, e0, e1, P, D);
    return launch_timed(k_dual_price<false, true, true>, c.price_grid, 0, s, e0, e1, P, D);
}

hipError_t launch_dual_long(const Params& P, const DualLongArgs& D, hipStream_t s) {
    hipLaunchKernelGGL(k_dual_long, dim3(1), dim3(LONG_BLOCK), 0, s, P, D);
    return hipGetLastError();
}

hipError_t launch_dual_flips(const Params& P, const DualLongArgs& D, double* b_eff, hipStream_t s) {
    const int grid = (int)((P.L + BOX_BLOCK - 1) / BOX_BLOCK);
    hipLaunchKernelGGL(k_dual_flips, dim3(grid), dim3(BOX_BLOCK), 0, s, P, D, b_eff);
    return hipGetLastError();
}

hipError_t launch_dual_update_long(const Params& P, const DualLongArgs& D, const DualCfg& c, bool se, hipStream_t s,
                                   hipEvent_t e0, hipEvent_t e1) {
    if (se) {
        if (!c.se_update_lds) return launch_timed(k_dual_update<false, 2, true>, c.update_grid, 0, s, e0, e1, P, D);
        if (c.se_rho_lds)
            return launch_timed(k_dual_update<true, 1, true>, c.update_grid, (size_t)P.L * 24, s, e0, e1, P, D);
        return launch_timed(k_dual_update<true, 2, true>, c.update_grid, (size_t)P.L * 16, s, e0, e1, P, D);
    }
    if (c.update_lds) return launch_timed(k_dual_update<true, 0, true>, c.update_grid, (size_t)P.L * 16, s, e0, e1, P, D);
    return launch_timed(k_dual_update<false, 0, true>, c.update_grid, 0, s, e0, e1, P, D);
}

hipError_t launch_dual_norms(const Params& P, const DualSeArgs& D, const DualCfg& c, hipStream_t s) {
    hipLaunchKernelGGL(k_dual_norms, dim3(c.update_grid), dim3(DUAL_BLOCK), 0, s, P, D);
    return hipGetLastError();
}

hipError_t launch_box_rhs(const Params& P, const DualBoxArgs& D, const double* b_user, double* b_eff, hipStream_t s) {
    const int grid = (int)((P.L + BOX_BLOCK - 1) / BOX_BLOCK);
    hipLaunchKernelGGL(k_box_rhs, dim3(grid), dim3(BOX_BLOCK), 0, s, P, D, b_user, b_eff);
    return hipGetLastError();
}

hipError_t launch_box_rhs_lu(const Params& P, const DualBoxArgs& D, const double* lsh, const double* b_user,
                             double* b_eff, hipStream_t s) {
    const int grid = (int)((P.L + BOX_BLOCK - 1) / BOX_BLOCK);
    hipLaunchKernelGGL(k_box_rhs_lu, dim3(grid), dim3(BOX_BLOCK), 0, s, P, D, lsh, b_user, b_eff);
    return hipGetLastError();
}

hipError_t launch_box_xb(const Params& P, const DualCfg& c, hipStream_t s) {
    hipLaunchKernelGGL(k_box_xb, dim3(c.update_grid), dim3(DUAL_BLOCK), 0, s, P);
    return hipGetLastError();
}

}  // namespace spx
