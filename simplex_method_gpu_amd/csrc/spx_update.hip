// spx_update.hip — the FTRAN launch of a loop pass (the pass is described at
// the head of spx_kernels.h): k_update (explicit B^-1, eta window, row
// shards), k_ftran_bc (the compact operand), k_tab_update (the window
// tableau), the one-workgroup tail kernels, and their launchers.  The partials
// and the pivot tail they share with k_price are in spx_handoff.h.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>

#include <atomic>

#include "spx_device.h"
#include "spx_common.h"
#include "spx_handoff.h"
#include "spx_kernels.h"
#include "spx_tabdev.h"

namespace spx {

#ifndef SPX_WIN_U1
#define SPX_WIN_U1 8  // eta-window FTRAN stream, 1 row per wave: dbl2 loads per lane per round trip
#endif
// compact FTRAN (Params::bc): dbl2 chunks of each compact row requested at
// k_update entry (256 columns), and column-list entries per thread requested
// ahead of the entering column (1,024 columns at 512 threads)
#ifndef SPX_BC_PF
#define SPX_BC_PF 1  // C3 A/B (round-2 tools/r02_abbench.sh, in git history): 1 chunk 12.45k it/s, 2 chunks 12.31-12.34k
#endif
#ifndef SPX_BC_PF2
#define SPX_BC_PF2 4
#endif
constexpr int BC_PF = SPX_BC_PF;
constexpr int BC_PF2 = SPX_BC_PF2;  // chunks requested once S is known (up to 512 columns)
constexpr int BC_APC = 8192;  // A_p gathered onto the list in LDS blocks of this many columns
constexpr int BC_RL = 2;

// ---------------------------------------------------------------------------
// Fused: pending rank-1 update + FTRAN + x_b update + ratio test + leaving
// argmin + pivot tail
// ---------------------------------------------------------------------------
// Explicit in-place update (v4:331-333): the pivot row r, A_p and b are
// staged in LDS once per workgroup (read from L2 per element they were three
// operand streams beside the B stream), and each wave loads its next chunk of
// B rows before storing this one (vmcnt counts stores too, so loads issued
// behind a chunk's stores could not be waited for without them).  Needs the
// three vectors in LDS and whole 4-chunk steps; from L = 2048 (C3 8.16k ->
// 8.59k it/s, k_update 56 -> 47 us; at C2, L = 1024, the fill cost 1 %).
__host__ __device__ inline bool upd_xlds(const Params& P) {
    return !P.win && !P.row_shard && P.L >= 2048 && P.L * 24 <= 96 * 1024 && ((P.L >> 1) % 256) == 0;
}

// Eta-window FTRAN rows: acc[u] += B_w[row u,:] . A_p for R full rows, U dbl2
// loads of B per lane per round trip.  a: A_p (read through L1/L2; staged in
// LDS it measured within 1 us or slower, DESIGN_HISTORY.md).
template <int U, int R, int BNT>
__device__ __forceinline__ void win_rows(const dbl2* __restrict__ a, const dbl2* __restrict__ src, int64_t base,
                                         int64_t L2, int lane, double (&acc)[R], const dbl2 (*pre)[R],
                                         const dbl2 (&apre)[U], bool have_apre) {
    int64_t k = lane;
    if (pre) {  // the first U chunks were loaded at kernel entry (A_p's too when have_apre)
        dbl2 av[U];
#pragma unroll
        for (int t = 0; t < U; ++t) av[t] = have_apre ? apre[t] : a[k + t * 64];
#pragma unroll
        for (int t = 0; t < U; ++t) {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                acc[u] = fma(pre[t][u].x, av[t].x, acc[u]);
                acc[u] = fma(pre[t][u].y, av[t].y, acc[u]);
            }
        }
        k += U * 64;
    }
    for (; k + (U - 1) * 64 < L2; k += U * 64) {
        dbl2 av[U], bv[U][R];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            av[t] = a[k + t * 64];
#pragma unroll
            for (int u = 0; u < R; ++u) bv[t][u] = ld2<BNT>(&src[base + u * L2 + k + t * 64]);
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                acc[u] = fma(bv[t][u].x, av[t].x, acc[u]);
                acc[u] = fma(bv[t][u].y, av[t].y, acc[u]);
            }
        }
    }
    for (; k < L2; k += 64) {
        const dbl2 av = a[k];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const dbl2 bv = src[base + u * L2 + k];
            acc[u] = fma(bv.x, av.x, acc[u]);
            acc[u] = fma(bv.y, av.y, acc[u]);
        }
    }
}

// row i clamped into [0, m): an unconditional prefetch of a row past the end
// reads the last row instead, and is never consumed
__device__ __forceinline__ int64_t clamp_row(int64_t i, int64_t m) { return i < m ? i : m - 1; }

template <int BLOCK, int R, bool RS, bool WIN, int BNT, bool BC>
__global__ __launch_bounds__(BLOCK) void k_update(Params P) {
    DevState* st = P.st;
    using Lds = UpdLds<BLOCK>;
    constexpr int WAVES = BLOCK / 64;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // eta window: B_w is read-only, so this wave's rows can be in flight
    // before anything else is known (status, entering column, pivot state);
    // a short-lived wave otherwise starts its stream after that chain of
    // dependent loads (tools/stream_bench.hip: the bare 134 MB one-shot
    // stream takes 23 us)
    // (the explicit in-place update measured slower with its old rows loaded
    // this way: C3 59 -> 66 us, so window only)
    // Issue order (vmcnt retires in issue order): the deferred pricing
    // partials, then this wave's first B_w chunks -- unconditional with
    // clamped indices, so the waits below count exactly and the price
    // reduction does not wait for the B prefetch -- then the loop state,
    // field by field (scalar loads: still in the entry block, after no store;
    // a whole-struct snapshot's dead registers were reused at once, and as
    // vector loads the uniform values were moved to scalar registers at once,
    // both waits that held the prefetch), then the multi-rank candidate
    // records and A_p's first chunks.  The status check comes after the price
    // reduction; no store precedes it.
    const int pgi = tid < P.price_grid ? tid : P.price_grid - 1;
    const PricePartial pwl = P.price_partials[pgi];
    constexpr int PFU = WIN ? ((R == 1) ? SPX_WIN_U1 : ((R == 2) ? 8 : ((R == 4) ? 4 : 2))) : ((R >= 4) ? 2 : 4);
    dbl2 pfb[PFU][R];
    const int64_t pf_row = ((int64_t)blockIdx.x * WAVES + wave) * R;
    const bool pf_ok = WIN && !RS && !BC && pf_row + R <= P.m && (P.L >> 1) >= PFU * 64;
    if constexpr (WIN && !RS) {
        const int64_t L2c = P.L >> 1;
        // (compact FTRAN, P.bc: the first BC_PF chunks of this wave's
        // compact rows, the later ones re-requesting chunk 0 (cache hits), so
        // the loads stay unconditional and the waits below exact)
        // (each row clamped on its own: in a partly filled last wave, row u <
        // nvalid must be row pf_row + u, which the compact path consumes)
        const dbl2* b0 = reinterpret_cast<const dbl2*>(BC ? bc_buf(P, P.bc_n[2]) : P.B0);
        const int64_t ld2r = BC ? (int64_t)(P.bc_n[1] >> 1) : L2c;  // row pitch (compact: bc_pitch)
#pragma unroll
        for (int t = 0; t < PFU; ++t) {
            const int64_t k = (BC && t >= BC_PF) ? lane : (lane + t * 64 < L2c ? lane + t * 64 : L2c - 1);
#pragma unroll
            for (int u = 0; u < R; ++u) pfb[t][u] = ld2<BNT>(&b0[clamp_row(pf_row + u, P.m) * ld2r + k]);
        }
    }
    // compact FTRAN: the column list and this wave's unit flags, ahead of p
    int32_t rlv[BC_RL];
    int32_t rmv[R];
    if constexpr (BC) {
#pragma unroll
        for (int j = 0; j < BC_RL; ++j) {
            const int64_t c = tid + (int64_t)j * BLOCK;
            rlv[j] = P.rlist[c < P.m ? c : 0];
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int64_t i = pf_row + u;
            rmv[u] = P.rmap[i < P.m ? i : 0];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    struct {
        int32_t status, nb_count, nw;
        int64_t iter, limit, q, xb_applied;
        double aq;
    } Sv;
    Sv.status = st->status;
    Sv.nb_count = st->nb_count;
    Sv.iter = st->iter;
    Sv.limit = st->limit;
    Sv.q = st->q;
    Sv.aq = st->aq;
    Sv.xb_applied = st->xb_applied;
    Sv.nw = st->nw;
    const unsigned long long t_wg0 = (P.stamps && blockIdx.x == 0) ? rtime() : 0ull;
    PricePartial pw0{INFINITY, INT64_MAX, 0.0, 0.0};
    if (P.defer_price && tid < P.price_grid) pw0 = pwl;
    // the merged entering candidates (k_price's last workgroup, one record
    // per rank: MINLOC, v4:294-302), and then A_p's first chunks
    double min_e0 = INFINITY;
    int64_t p0 = INT64_MAX;
    int gw0 = 0;
    if (!P.defer_price) {
        for (int g = 0; g < P.nin; ++g) {
            const ArgMinEntry e = P.price_in[g * P.pr_stride];
            if (argmin_better(e.val, e.idx, min_e0, p0)) { min_e0 = e.val; p0 = e.idx; gw0 = g; }
        }
    }
    dbl2 apf[PFU];
    const bool apf_ok = pf_ok && !P.defer_price && p0 >= 0 && p0 < P.n;
    if (apf_ok) {
        const dbl2* a0 = reinterpret_cast<const dbl2*>(P.A + p0 * P.L);
#pragma unroll
        for (int t = 0; t < PFU; ++t) apf[t] = a0[lane + t * 64];
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    // entering column: MINLOC over all ranks' candidates (v4:294-302), or,
    // with the pricing tail deferred, over k_price's workgroup partials
    // (every workgroup the same reduction: the same winner)
    double min_e = INFINITY, e_enter = 0.0;
    int64_t p = INT64_MAX;
    int gw = 0;
    if (P.defer_price) {
        PricePartial w = pw0;
        for (int g = tid + BLOCK; g < P.price_grid; g += BLOCK) {
            const PricePartial v = P.price_partials[g];
            if (argmin_better(v.val, v.idx, w.val, w.idx)) w = v;
        }
        // DPP argmin; the winner's reduced cost from its lane (cross-lane
        // reads outside the lane-0 branch)
        double bv = w.val;
        int64_t bj = w.idx;
        lane_argmin<64>(bv, bj);
        bv = readlane_d(bv, 63);
        bj = readlane_l(bj, 63);
        const uint64_t hit = __ballot(w.val == bv && w.idx == bj);
        const double be = readlane_d(w.pad, hit ? (int)__builtin_ctzll(hit) : 0);
        __shared__ PricePartial s_pw[WAVES];
        if (lane == 0) s_pw[wave] = PricePartial{bv, bj, 0.0, be};
        lds_barrier();  // (not __syncthreads: its vmcnt(0) would wait for the B prefetch)
        PricePartial t = s_pw[0];
        for (int i = 1; i < WAVES; ++i)
            if (argmin_better(s_pw[i].val, s_pw[i].idx, t.val, t.idx)) t = s_pw[i];
        min_e = t.val;
        p = t.idx;
        e_enter = t.pad;
    } else {
        min_e = min_e0;
        p = p0;
        gw = gw0;
    }
    const bool dvx_grp = P.devex && P.nin > 1;
    double wp_grp = 1.0;
    if (dvx_grp) {
        const double* ex = dvx_payload(P, gw);
        e_enter = ex[0];
        wp_grp = ex[1];
    }
    if (Sv.status != ST_RUNNING || Sv.iter >= Sv.limit) return;
    wg0_mark(P, 0, t_wg0);
    unsigned long long* const slot = P.stamps ? P.stamps + 4 : nullptr;
    stamp_start(slot);
    wg0_mark(P, 1, t_wg0);
    if (no_entering(P, min_e, p)) {  // OptimumFound (v4:299-302)
        if (blockIdx.x == 0 && tid == 0) {
            st->p = p;
            st->min_e = (P.devex && (P.defer_price || dvx_grp)) ? e_enter : min_e;
            st->status = ST_OPTIMAL;
        }
        return;
    }

    // compact FTRAN (BC): with p known, the operands that depend on it or on
    // S are requested now, ahead of the row scalars (vmcnt retires in order):
    // this row's chunks BC_PF..BC_PF2-1 (chunks past S re-request chunk 0, a
    // cache hit, so the loads stay unconditional), A_p on the column list
    // and A_p[i] for the unit term
    int Sbc = 0;
    dbl2 pf2[BC_PF2 - BC_PF][R];
    double apv[BC_RL], auv[R];
    if constexpr (BC) {
        Sbc = P.bc_n[0];
        const int64_t L2c = P.L >> 1;
        const int64_t ld2r = P.bc_n[1] >> 1;
        const dbl2* b0 = reinterpret_cast<const dbl2*>(bc_buf(P, P.bc_n[2]));
#pragma unroll
        for (int t = BC_PF; t < BC_PF2; ++t) {
            const int k2 = lane + 64 * t;
            const int kk = (2 * k2 < Sbc && k2 < L2c) ? k2 : lane;
#pragma unroll
            for (int u = 0; u < R; ++u) pf2[t - BC_PF][u] = b0[clamp_row(pf_row + u, P.m) * ld2r + kk];
        }
        const double* apd = P.A + p * P.L;
#pragma unroll
        for (int j = 0; j < BC_RL; ++j) apv[j] = apd[rlv[j]];
#pragma unroll
        for (int u = 0; u < R; ++u) auv[u] = apd[clamp_row(pf_row + u, P.m)];
    }
    const int64_t it = Sv.iter;
    const int par = (int)(it & 1);
    const int64_t m = P.m, L = P.L, L2 = L >> 1;
    // row-sharded storage always ping-pongs (its tail recomputes the winner
    // row from the old rows); replicated storage is one buffer, updated in
    // place (the pivot row the stream needs is staged into P.rbuf by k_price)
    constexpr bool INPL = !RS;
    const double* S = INPL ? P.B0 : (par ? P.B1 : P.B0);
    const dbl2* src = reinterpret_cast<const dbl2*>(S);
    dbl2* dst = reinterpret_cast<dbl2*>(INPL ? P.B0 : (par ? P.B0 : P.B1));
    const double* a_prev = par ? P.alpha1 : P.alpha0;  // alpha of pivot it-1
    double* a_new = par ? P.alpha0 : P.alpha1;
    // the pending pivot it-1: r = S[q,:], E from a_prev and aq
    const int nw = WIN ? Sv.nw : 0;
    const int tau = nw - 1;  // eta window: the pending pivot
    const bool pend = WIN ? nw > 0 : it > 0;
    const int64_t qp = Sv.q;
    const double aqp = Sv.aq;
    const double* rrow = !pend ? P.zeros : P.rbuf;
    const dbl2* __restrict__ rp = reinterpret_cast<const dbl2*>(rrow);
    const dbl2* __restrict__ ap = reinterpret_cast<const dbl2*>(P.A + p * L);
    const bool upd_x = Sv.xb_applied < it;

    // s_x = r.b (v4:347) for the deferred x_b update is accumulated inside the
    // row stream (every wave streams all of r; lane-strided, k ascending, then
    // a 64-lane butterfly: the same bits in every wave and in k_flush)
    const dbl2* __restrict__ bp = reinterpret_cast<const dbl2*>(P.b);
    double sxa = 0.0;

    // rows of this wave: local storage rows lr0.., global rows gr0..
    const int64_t nrows = RS ? P.mloc : m;
    const int64_t lr0 = ((int64_t)blockIdx.x * WAVES + wave) * R;
    const int64_t gr0 = (RS ? P.r0 : 0) + lr0;
    const int nvalid = (int)((lr0 >= nrows) ? 0 : ((nrows - lr0 < R) ? (nrows - lr0) : R));
    double ei[R], acc[R], cbv[R], xbv[R];
    int64_t bixv[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
        ei[u] = (pend && u < nvalid) ? eta_entry(a_prev[gr0 + u], gr0 + u, qp, aqp) : 0.0;
        acc[u] = 0.0;
        // row scalars of the epilogue, loaded ahead of the stream
        cbv[u] = u < nvalid ? P.c_B[gr0 + u] : 0.0;
        xbv[u] = u < nvalid ? P.x_b[gr0 + u] : 0.0;
        bixv[u] = u < nvalid ? P.b_ixs[gr0 + u] : -1;
    }
    double ucv[R];  // eta window: this row's U coefficients of the earlier window pivots
#pragma unroll
    for (int u = 0; u < R; ++u)
        ucv[u] = (WIN && u < nvalid && lane < tau) ? P.U[(lr0 + u) * P.win + lane] : 0.0;
    TailPre tpre{0, 0.0, 0, -1, -1, 0.0, 0, 0.0, 0};
    if (!RS && tid == 0 && !P.split_tail) tpre = tail_prefetch(P, Sv.nw, Sv.nb_count, p);
    if (P.defer_price || dvx_grp) {
        tpre.has_e = true;
        tpre.e_enter = e_enter;
    }
    if (dvx_grp) tpre.wp = wp_grp;
    const int64_t base = lr0 * L2;
    unsigned long long* const win = slot ? P.stamps + 16 : nullptr;
    stamp_stream(win, true);
    wg0_mark(P, 2, t_wg0);
    // explicit update with r / A_p / b in LDS (upd_xlds): the whole workgroup
    // stages them (every wave, whatever its rows)
    const bool xl = !WIN && !RS && upd_xlds(P);
    const dbl2* xr = reinterpret_cast<const dbl2*>(smem + Lds::bytes);
    const dbl2* xa = xr + L2;
    const dbl2* xb = xa + L2;
    if constexpr (!WIN && !RS) {
        if (xl) {
            dbl2* d = reinterpret_cast<dbl2*>(smem + Lds::bytes);
            for (int64_t kk = tid; kk < L2; kk += BLOCK) {
                const dbl2 r2 = rp[kk], a2 = ap[kk], b2 = bp[kk];
                d[kk] = r2;
                d[L2 + kk] = a2;
                d[2 * L2 + kk] = b2;
            }
            lds_barrier();
        }
    }
    if constexpr (WIN) {
        // eta window: B_w is only read; alpha_i = B_w[i,:] . A_p +
        // sum_tau U[i][tau] Wt[p][tau], the window terms (lane tau) joining the
        // lane partials; the pending pivot's eta column is stored into U
        const int KW = P.win;
        const double* wrec = P.nin > 1 ? reinterpret_cast<const double*>(P.price_in + gw * P.pr_stride + 1)
                                       : P.Wt + p * KW;
        const double wl = lane < nw ? wrec[lane] : 0.0;
        // s_x = r_tau . b = xw[q] + sum_{s<tau} U[q][s] Wt[n][s] (v4:347), also
        // kept as Wt[n][tau] for later pivots and the fold: the operands are
        // loaded here, the sum is formed after the stream (a dependent load +
        // butterfly here delayed every wave's stream)
        double sx_u = 0.0, sx_w = 0.0, sx_x = 0.0;
        if (pend) {
            if (lane < tau) {
                sx_u = P.U[qp * KW + lane];
                sx_w = P.Wt[P.n * KW + lane];
            }
            sx_x = P.xw[qp];
        }
        if constexpr (BC) {
            // compact FTRAN: B_w[i,:].A_p = sum_c bc[i][c] A_p[rlist[c]] (+ A_p[i]
            // when column i is e_i).  Per lane: the unit term first (lane 0),
            // then its dbl2 chunks lane + 64 t ascending, .x before .y: one
            // order for every geometry and dispatch.  A_p gathered onto the
            // list in LDS; the first BC_PF chunks of each row were requested at
            // kernel entry (pfb), the rest here.
            double* apc = reinterpret_cast<double*>(smem + Lds::bytes);
            const int S = Sbc;
            const double* apd = P.A + p * L;
            const dbl2* apc2 = reinterpret_cast<const dbl2*>(apc);
            double a[R];
#pragma unroll
            for (int u = 0; u < R; ++u) a[u] = (u < nvalid && lane == 0 && rmv[u] < 0) ? auv[u] : 0.0;
            // column blocks of BC_APC (one at S <= 8192): A_p on the block's
            // list entries into LDS, then every row's chunks of the block
            for (int cb = 0; cb < S || cb == 0; cb += BC_APC) {
                const int ce = S < cb + BC_APC ? S : cb + BC_APC;
                if (cb > 0) lds_barrier();  // the previous block's reads are done
#pragma unroll
                for (int j = 0; j < BC_RL; ++j) {
                    const int c = tid + j * BLOCK;
                    if (cb == 0 && c < ce) apc[c] = apv[j];
                }
                for (int c = cb + (cb == 0 ? BC_RL * BLOCK : 0) + tid; c < ce; c += BLOCK) apc[c - cb] = apd[P.rlist[c]];
                lds_barrier();
                const int kb = cb >> 1, ke = (ce + 1) >> 1;  // this block's dbl2 chunks
#pragma unroll
                for (int u = 0; u < R; ++u) {
                    if (u < nvalid) {
                        // the active buffer (bc_n[2]), as the prefetches above read it
                        const dbl2* brow = reinterpret_cast<const dbl2*>(bc_buf(P, P.bc_n[2])) +
                                           (lr0 + u) * (int64_t)(P.bc_n[1] >> 1);
                        auto take = [&](dbl2 v, int k2) {
                            const dbl2 w = apc2[k2 - kb];
                            if (2 * k2 < S) a[u] = fma(v.x, w.x, a[u]);
                            if (2 * k2 + 1 < S) a[u] = fma(v.y, w.y, a[u]);
                        };
                        if (cb == 0) {
#pragma unroll
                            for (int t = 0; t < BC_PF; ++t) {
                                const int k2 = lane + 64 * t;
                                if (k2 < ke) take(pfb[t][u], k2);
                            }
#pragma unroll
                            for (int t = BC_PF; t < BC_PF2; ++t) {
                                const int k2 = lane + 64 * t;
                                if (k2 < ke) take(pf2[t - BC_PF][u], k2);
                            }
                        }
                        for (int k0 = (cb == 0 ? BC_PF2 * 64 : kb); k0 < ke; k0 += 8 * 64) {
                            dbl2 v[8];
#pragma unroll
                            for (int t = 0; t < 8; ++t) {
                                const int k2 = k0 + lane + 64 * t;
                                v[t] = brow[k2 < ke ? k2 : kb];
                            }
#pragma unroll
                            for (int t = 0; t < 8; ++t) {
                                const int k2 = k0 + lane + 64 * t;
                                if (k2 < ke) take(v[t], k2);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < R; ++u)
                if (u < nvalid) acc[u] = a[u];
        } else {
        if (nvalid == R) {
            // 16 dbl2 loads of B per lane in flight: a 32 KiB row is two round trips
            constexpr int U = (R == 1) ? SPX_WIN_U1 : ((R == 2) ? 8 : ((R == 4) ? 4 : 2));
            static_assert(U == PFU, "prefetch and stream chunking agree");
            win_rows<U, R, BNT>(ap, src, base, L2, lane, acc, pf_ok ? pfb : nullptr, apf, apf_ok);
        } else if (nvalid > 0) {
            for (int64_t k = lane; k < L2; k += 64) {
                const dbl2 av = ap[k];
                for (int u = 0; u < nvalid; ++u) {
                    const dbl2 bv = src[base + u * L2 + k];
                    acc[u] = fma(bv.x, av.x, acc[u]);
                    acc[u] = fma(bv.y, av.y, acc[u]);
                }
            }
        }
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            if (u < nvalid) {
                const int64_t li = lr0 + u;
                const double cu = lane < tau ? ucv[u] : (lane == tau ? ei[u] : 0.0);
                acc[u] = fma(cu, wl, acc[u]);
                if (pend && lane == 0) P.U[li * KW + tau] = ei[u];
            }
        }
        double sxw = 0.0;
        if (pend) {
            sxw = sx_x + wave_sum(mul_nc(sx_u, sx_w));
            if (blockIdx.x == 0 && tid == 0) P.Wt[P.n * KW + tau] = sxw;
            if (lane == 0) {
                // the exact Wt entries of the basic columns for the pending
                // pivot: r_tau . A_j = aq for its entering column, 0 for the
                // others (their B^-1 A_j is a unit vector)
                for (int u = 0; u < nvalid; ++u) {
                    const int64_t i = gr0 + u;
                    P.Wt[bixv[u] * KW + tau] = (i == qp) ? aqp : 0.0;
                }
            }
        }
        if (upd_x) sxa = sxw;
    } else if (xl && nvalid == R) {
        // r / A_p / b from LDS, B rows one 4-chunk step ahead (upd_xlds)
        constexpr int U = (R >= 4) ? 2 : 4;
        const int nit = (int)(L2 / (U * 64));
        dbl2 bc[U][R], bn[U][R];
        int64_t k = lane;
#pragma unroll
        for (int t = 0; t < U; ++t)
#pragma unroll
            for (int u = 0; u < R; ++u) bc[t][u] = ld2<SPX_NT_BLOAD>(&src[base + u * L2 + k + t * 64]);
        for (int itn = 0; itn < nit; ++itn, k += U * 64) {
            // the next step's rows (the first step's again on the last one:
            // an unconditional load keeps the waits exact)
            const int64_t kn = (itn + 1 < nit) ? k + U * 64 : (int64_t)lane;
#pragma unroll
            for (int t = 0; t < U; ++t)
#pragma unroll
                for (int u = 0; u < R; ++u) bn[t][u] = ld2<SPX_NT_BLOAD>(&src[base + u * L2 + kn + t * 64]);
            dbl2 rv[U], av[U], bb[U];
#pragma unroll
            for (int t = 0; t < U; ++t) {
                rv[t] = xr[k + t * 64];
                av[t] = xa[k + t * 64];
                bb[t] = xb[k + t * 64];
            }
#pragma unroll
            for (int t = 0; t < U; ++t) {
                sxa = fma(rv[t].x, bb[t].x, sxa);
                sxa = fma(rv[t].y, bb[t].y, sxa);
#pragma unroll
                for (int u = 0; u < R; ++u) {
                    dbl2 nv;
                    nv.x = fma(ei[u], rv[t].x, bc[t][u].x);
                    nv.y = fma(ei[u], rv[t].y, bc[t][u].y);
                    st2<SPX_NT_BSTORE>(nv, &dst[base + u * L2 + k + t * 64]);
                    acc[u] = fma(nv.x, av[t].x, acc[u]);
                    acc[u] = fma(nv.y, av[t].y, acc[u]);
                }
            }
#pragma unroll
            for (int t = 0; t < U; ++t)
#pragma unroll
                for (int u = 0; u < R; ++u) bc[t][u] = bn[t][u];
        }
    } else if (nvalid == R) {
        constexpr int U = (R >= 4) ? 2 : 4;
        static_assert(WIN || U == PFU, "prefetch and stream chunking agree");
        int64_t k = lane;
        bool first = pf_ok;
        for (; k + (U - 1) * 64 < L2; k += U * 64) {
            dbl2 rv[U], av[U], bb[U], bv[U][R];
#pragma unroll
            for (int t = 0; t < U; ++t) {
                rv[t] = rp[k + t * 64];
                av[t] = ap[k + t * 64];
                bb[t] = bp[k + t * 64];
#pragma unroll
                for (int u = 0; u < R; ++u)
                    bv[t][u] = first ? pfb[t < PFU ? t : 0][u] : ld2<SPX_NT_BLOAD>(&src[base + u * L2 + k + t * 64]);
            }
            first = false;
#pragma unroll
            for (int t = 0; t < U; ++t) {
                sxa = fma(rv[t].x, bb[t].x, sxa);
                sxa = fma(rv[t].y, bb[t].y, sxa);
#pragma unroll
                for (int u = 0; u < R; ++u) {
                    dbl2 nv;
                    nv.x = fma(ei[u], rv[t].x, bv[t][u].x);
                    nv.y = fma(ei[u], rv[t].y, bv[t][u].y);
                    st2<SPX_NT_BSTORE>(nv, &dst[base + u * L2 + k + t * 64]);
                    acc[u] = fma(nv.x, av[t].x, acc[u]);
                    acc[u] = fma(nv.y, av[t].y, acc[u]);
                }
            }
        }
        for (; k < L2; k += 64) {
            const dbl2 rv = rp[k], av = ap[k], bb = bp[k];
            sxa = fma(rv.x, bb.x, sxa);
            sxa = fma(rv.y, bb.y, sxa);
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const dbl2 bv = src[base + u * L2 + k];
                dbl2 nv;
                nv.x = fma(ei[u], rv.x, bv.x);
                nv.y = fma(ei[u], rv.y, bv.y);
                dst[base + u * L2 + k] = nv;
                acc[u] = fma(nv.x, av.x, acc[u]);
                acc[u] = fma(nv.y, av.y, acc[u]);
            }
        }
    } else if (nvalid > 0) {
        for (int64_t k = lane; k < L2; k += 64) {
            const dbl2 rv = rp[k], av = ap[k], bb = bp[k];
            sxa = fma(rv.x, bb.x, sxa);
            sxa = fma(rv.y, bb.y, sxa);
            for (int u = 0; u < nvalid; ++u) {
                const dbl2 bv = src[base + u * L2 + k];
                dbl2 nv;
                nv.x = fma(ei[u], rv.x, bv.x);
                nv.y = fma(ei[u], rv.y, bv.y);
                dst[base + u * L2 + k] = nv;
                acc[u] = fma(nv.x, av.x, acc[u]);
                acc[u] = fma(nv.y, av.y, acc[u]);
            }
        }
    }

    stamp_stream(win, false);
    wg0_mark(P, 3, t_wg0);
    const double s_x = (upd_x && nvalid > 0) ? (WIN ? sxa : wave_sum(sxa)) : 0.0;

    // x_b += s_x E (v4:348) for the owned rows; alpha_i, theta_i
    // (compute_theta, v4:199-208) and the wave's ratio-test partial
    UpdPartial wp = upd_empty();
#pragma unroll
    for (int u = 0; u < R; ++u) {
        if (u < nvalid) {
            const double a = wave_sum(acc[u]);
            const int64_t i = gr0 + u;
            const double cb = cbv[u];
            double xb = xbv[u];
            if (upd_x) xb = fma(s_x, ei[u], xb);
            if (lane == 0) {
                a_new[i] = a;  // read back by the next pass (own row) / k_flush
                if (upd_x) P.x_b[i] = xb;
            }
            const bool pos = a > P.piv_tol;  // 0 for the reference rule (v4:202)
            const double th = ratio_key(P, xb, a);
            wp.nonpos += !pos;
            wp.T = fma(cb, a, wp.T);
            if (argmin_better(th, i, wp.theta, wp.idx)) {
                wp.theta = th;
                wp.idx = i;
                wp.a_w = a;
                wp.cb_w = cb;
                wp.bix_w = bixv[u];
            }
        }
    }
    UpdPartial* red = reinterpret_cast<UpdPartial*>(smem + Lds::red);
    int* s_last = reinterpret_cast<int*>(smem + Lds::last);
    if (lane == 0) red[wave] = wp;
    // only the partial crosses workgroups inside the launch (thread 0 drains
    // it below), so the barrier waits for LDS only; the row-sharded tail
    // reads other workgroups' alpha: full barrier
    if constexpr (RS) __syncthreads();
    else lds_barrier();
    if (P.split_tail) {  // k_tail merges after the kernel boundary: plain stores, no fan-in
        if (tid == 0) {
            UpdPartial w = red[0];
            for (int i = 1; i < WAVES; ++i) upd_merge(w, red[i]);
            upd_publish(P, blockIdx.x, w);
        }
        return;
    }
    if (!RS && P.upd_tag) {  // tagged hand-off to the last workgroup (upd_publish_tagged)
        const uint32_t tag = (uint32_t)(it + 1);
        if (wave == 0) {
            UpdPartial w = red[0];
            for (int i = 1; i < WAVES; ++i) upd_merge(w, red[i]);
            upd_publish_tagged(P, blockIdx.x, w, tag, lane);
            wg0_mark(P, 4, t_wg0);
        }
        if (blockIdx.x != gridDim.x - 1) return;
        const unsigned long long t_tail = slot ? rtime() : 0;
        update_tail<BLOCK>(P, st, p, min_e, it, smem, gridDim.x, &tpre, tag);
        stamp_tail(slot, t_tail, win);
        return;
    }
    if (tid == 0) {
        UpdPartial w = red[0];
        for (int i = 1; i < WAVES; ++i) upd_merge(w, red[i]);
        upd_publish(P, blockIdx.x, w);
        drain_vmem();  // the partial is visible before the ticket
        *s_last = arrive_last(arrive_group(P.arrive, ARR_UPDATE), gridDim.x, blockIdx.x);
    }
    if constexpr (RS) __syncthreads();
    else lds_barrier();
    if (!*s_last) return;
    const unsigned long long t_tail = slot ? rtime() : 0;
    if constexpr (RS)
        update_tail_rs<BLOCK>(P, st, it, par, a_prev, smem, gridDim.x);
    else
        update_tail<BLOCK>(P, st, p, min_e, it, smem, gridDim.x, &tpre);
    stamp_tail(slot, t_tail, win);
}

// Compact-operand FTRAN pass, one B_w row per wave (the default window
// geometry at C3 / C4: k_update<512, 1, false, true, 0, true>'s work, term for
// term and in the same per-lane order, so the same bits).  What changes is the
// dependency chain.  Everything that does not depend on the entering column
// is requested at kernel entry: the pricing partials, the loop state and the
// list size S, the column list, this row's unit flag, both alpha parities,
// c_B / x_b / b_ixs, its U row, the first BC_PF2 chunks of its compact row
// (chunks past S re-request chunk 0: unconditional loads, exact waits) and the
// s_x operands.  Once p is known a single round trip remains: A_p on the
// column list, A_p[i] and the winner's window coefficients Wt[p][.].  (In
// k_update the chunks past the first waited for S, A_p's gather for the row
// prefetch, and alpha for A_p's gather.)
// (launch bounds: 4 waves per SIMD, <= 128 VGPRs, so two 512-thread
// workgroups share a CU and the C3 grid, 512 workgroups, is resident at once:
// at 130 VGPRs it ran in two rounds, 11.6 -> 17.0 us)
//
// RPW > 1 (deferred tail only; SPX_FTRAN_RPW): each wave takes RPW rows, so
// a workgroup covers RPW of the one-row grid's slots -- slot g = blockIdx.x *
// RPW + r holds rows g * WAVES + wave, exactly the rows the one-row grid's
// workgroup g holds -- and publishes one partial per slot, merged over its
// waves in the same order.  Every row's terms, every slot's partial and the
// next pass's reduction over the slots are therefore those of RPW = 1, bit
// for bit; what changes is that the per-workgroup work (the pricing
// partials' reduction, A_p's gather on the list) is done by RPW times fewer
// workgroups, each wave keeps RPW rows' loads in flight, and the grid fits
// one workgroup per CU (<= 256 VGPRs).
// SEF (steepest edge, Params::se_fused): its own instantiation, so the
// Dantzig / Devex pass keeps its code
template <int BLOCK, bool DEFER, int RPW, bool SEF = false>
__global__ __launch_bounds__(BLOCK, RPW == 1 ? 4 : 2) void k_ftran_bc(Params P) {
    static_assert(RPW == 1 || DEFER, "several rows per wave: the deferred-tail form only");
    DevState* st = P.st;
    using Lds = UpdLds<BLOCK>;
    constexpr int WAVES = BLOCK / 64;
    constexpr int NCH = BC_PF2;  // dbl2 chunks of the compact row requested at entry
    // LDS: the RPW x WAVES wave partials, then A_p on the list
    constexpr size_t RED_BYTES = RPW == 1 ? Lds::bytes : sizeof(UpdPartial) * WAVES * RPW + 16;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t m = P.m, L2 = P.L >> 1;
    const int KW = P.win;
    int64_t irow[RPW], icl[RPW];
    bool rowv[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        irow[r] = ((int64_t)blockIdx.x * RPW + r) * WAVES + wave;  // this wave's rows
        rowv[r] = irow[r] < m;
        icl[r] = rowv[r] ? irow[r] : m - 1;
    }
    // ---- entry: everything independent of p (issue order = retire order)
    const int pgi = tid < P.price_grid ? tid : P.price_grid - 1;
    const PricePartial pwl = P.price_partials[pgi];
    int32_t rlv[BC_RL];
#pragma unroll
    for (int j = 0; j < BC_RL; ++j) {
        const int64_t c = tid + (int64_t)j * BLOCK;
        rlv[j] = P.rlist[c < m ? c : 0];
    }
    int32_t rmv[RPW];
    double al0[RPW], al1[RPW], cbv[RPW], xb0[RPW], urow[RPW];
    int64_t bix[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        rmv[r] = P.rmap[icl[r]];
        al0[r] = P.alpha0[icl[r]];
        al1[r] = P.alpha1[icl[r]];
        cbv[r] = P.c_B[icl[r]];
        xb0[r] = P.x_b[icl[r]];
        bix[r] = P.b_ixs[icl[r]];
    }
    const double sxw_w = P.Wt[P.n * KW + (lane < KW ? lane : 0)];
    struct {
        int32_t status, nb_count, nw;
        int64_t iter, limit, q, xb_applied;
        double aq;
    } Sv;
    Sv.status = st->status;
    Sv.nb_count = st->nb_count;
    Sv.iter = st->iter;
    Sv.limit = st->limit;
    Sv.q = st->q;
    Sv.aq = st->aq;
    Sv.xb_applied = st->xb_applied;
    Sv.nw = st->nw;
    const int Sbc = P.bc_n[0];
    const int64_t ldc = P.bc_n[1];  // compact row pitch (k_bc_list)
    const double* const bcb = bc_buf(P, P.bc_n[2]);  // the active buffer
    // (the entry clock goes here: taken first, its kernel-argument test ahead
    // of the loads reordered them, 11.7 -> 13.0 us)
    const unsigned long long t_wg_entry = P.stamps ? rtime() : 0ull;
    // the compact rows' first NCH chunks (S and the state are scalars: one wait)
    const dbl2* brow[RPW];
    dbl2 pf[RPW][NCH];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        brow[r] = reinterpret_cast<const dbl2*>(bcb + icl[r] * ldc);
#pragma unroll
        for (int t = 0; t < NCH; ++t) {
            const int k2 = lane + 64 * t;
            const int kk = t == 0 ? (k2 < L2 ? k2 : (int)L2 - 1) : ((2 * k2 < Sbc && k2 < L2) ? k2 : lane);
            pf[r][t] = brow[r][kk];
        }
    }
    // The U row only up to the window's pending pivots, requested after the
    // state arrives (since round 6: PMC read per launch 5.27 -> 3.70 MB, C3 pass
    // 74.76 -> 74.75 us, tools/ftran_ab.sh, profiles/r06_ftran_ab.txt).  Trimming
    // the compact row's chunks to S as well (lanes past it re-reading the row's
    // first line) read 2.91 MB but took 75.16 us: not kept.
#pragma unroll
    for (int r = 0; r < RPW; ++r) urow[r] = P.U[icl[r] * KW + (lane < Sv.nw - 1 ? lane : 0)];
    const int64_t qp = Sv.q;
    const bool pend = Sv.nw > 0;
    const int tau = Sv.nw - 1;
    const double sxw_u = P.U[(pend ? qp : 0) * KW + (lane < KW ? lane : 0)];
    const double sx_x = P.xw[pend ? qp : 0];
    __builtin_amdgcn_sched_barrier(0);
    // ---- entering column (v4:294-302): k_price's workgroup partials (every
    // workgroup the same reduction), or the ranks' merged candidates
    double min_e = INFINITY, e_enter = 0.0;
    int64_t p = INT64_MAX;
    int gw = 0;
    // (fused exchange: the polled entries, the winner's record after its
    // entry -- KW window coefficients, then Devex's two -- and a timeout flag)
    __shared__ uint32_t s_fh[4 * MBOX_FUSED_MAX_G];
    __shared__ double s_fw[64 + 2];
    __shared__ int s_fto;
    if (P.defer_price) {
        PricePartial w = tid < P.price_grid ? pwl : PricePartial{INFINITY, INT64_MAX, 0.0, 0.0};
        for (int g = tid + BLOCK; g < P.price_grid; g += BLOCK) {
            const PricePartial v = P.price_partials[g];
            if (argmin_better(v.val, v.idx, w.val, w.idx)) w = v;
        }
        double bv = w.val;
        int64_t bj = w.idx;
        lane_argmin<64>(bv, bj);
        bv = readlane_d(bv, 63);
        bj = readlane_l(bj, 63);
        const uint64_t hit = __ballot(w.val == bv && w.idx == bj);
        const double be = readlane_d(w.pad, hit ? (int)__builtin_ctzll(hit) : 0);
        __shared__ PricePartial s_pw[WAVES];
        if (lane == 0) s_pw[wave] = PricePartial{bv, bj, 0.0, be};
        lds_barrier();
        if constexpr (WAVES <= 8) {
            // every wave's entry requested, then a branch-free scan (a branch
            // per step on the uniform LDS values waited for each read in turn)
            double pv[WAVES], pe[WAVES];
            int64_t pj[WAVES];
#pragma unroll
            for (int k = 0; k < WAVES; ++k) {
                pv[k] = s_pw[k].val;
                pj[k] = s_pw[k].idx;
                pe[k] = s_pw[k].pad;
            }
            min_e = pv[0];
            p = pj[0];
            e_enter = pe[0];
#pragma unroll
            for (int k = 1; k < WAVES; ++k) {
                const bool b = argmin_better(pv[k], pj[k], min_e, p);
                min_e = b ? pv[k] : min_e;
                p = b ? pj[k] : p;
                e_enter = b ? pe[k] : e_enter;
            }
        } else {  // (16 waves: the preloaded entries spilled)
            PricePartial t = s_pw[0];
            for (int k = 1; k < WAVES; ++k)
                if (argmin_better(s_pw[k].val, s_pw[k].idx, t.val, t.idx)) t = s_pw[k];
            min_e = t.val;
            p = t.idx;
            e_enter = t.pad;
        }
    } else if (P.mbox_fused) {
        // fused exchange: wave 0 polls the ranks' entries in this rank's
        // mailbox, every wave merges them (the same rule as the all-gather's
        // consumers), then wave 0 polls the winner's window coefficients and
        // Devex payload; both reach the other waves through LDS
        const int G = P.nin;
        const bool live = Sv.status == ST_RUNNING && Sv.iter < Sv.limit;
        const uint32_t tag = mbox_tag(st->mbox_epoch, Sv.iter);
        const int64_t par = Sv.iter & 1;
        if (tid == 0) s_fto = 0;
        if (wave == 0 && live) {
            bool ok = true;
            for (int k = lane; k < 4 * G; k += 64) {
                uint32_t hf = 0u;
                ok = mbox_poll(P, par, k >> 2, k & 3, tag, &hf) && ok;
                s_fh[k] = hf;
            }
            if (!ok) s_fto = 1;  // (a benign race: every writer stores 1)
        }
        lds_barrier();
        if (live) {
            for (int g = 0; g < G; ++g) {
                const double v = __longlong_as_double((long long)(((uint64_t)s_fh[4 * g + 1] << 32) | s_fh[4 * g]));
                const int64_t j = (int64_t)(((uint64_t)s_fh[4 * g + 3] << 32) | s_fh[4 * g + 2]);
                if (argmin_better(v, j, min_e, p)) { min_e = v; p = j; gw = g; }
            }
            const int nw2 = P.pr_stride * 2 - 2;  // 8-byte fields after the entry: KW (+ 2 with Devex)
            if (wave == 0 && !s_fto) {
                bool ok = true;
                for (int k = lane; k < nw2; k += 64) {
                    uint32_t lo = 0u, hi = 0u;
                    ok = mbox_poll(P, par, gw, 4 + 2 * k, tag, &lo) && ok;
                    ok = mbox_poll(P, par, gw, 5 + 2 * k, tag, &hi) && ok;
                    s_fw[k] = __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
                }
                if (!ok) s_fto = 1;
            }
            lds_barrier();
            if (s_fto) {
                if (tid == 0) {
                    st->status = ST_HANDOFF_TIMEOUT;
                    if (DEFER) P.trec->fresh = 0;
                }
                return;
            }
        }
    } else {
        for (int g = 0; g < P.nin; ++g) {
            const ArgMinEntry e = P.price_in[g * P.pr_stride];
            if (argmin_better(e.val, e.idx, min_e, p)) { min_e = e.val; p = e.idx; gw = g; }
        }
    }
    const bool dvx_grp = P.devex && P.nin > 1;
    double wp_grp = 1.0;
    if (dvx_grp) {
        const double* ex = P.mbox_fused ? s_fw + KW : dvx_payload(P, gw);
        e_enter = ex[0];
        wp_grp = ex[1];
    }
    if (Sv.status != ST_RUNNING || Sv.iter >= Sv.limit) {
        if (DEFER && blockIdx.x == 0 && tid == 0) P.trec->fresh = 0;  // no pivot: nothing deferred
        return;
    }
    // (diagnostics: plain per-workgroup stores only -- the atomic phase
    // stamps of the other kernels, 512 workgroups on one address, would
    // themselves delay this kernel's waits)
    unsigned long long* const slot = nullptr;
    unsigned long long* const wgt =
        (P.stamps && tid == 0 && blockIdx.x < 4096) ? P.stamps + STAMP_FTRAN + (Sv.iter & 1) * 4 * 4096 + 4 * (int64_t)blockIdx.x
                                                    : nullptr;
    if (wgt) {
        wgt[0] = t_wg_entry;
        wgt[1] = rtime();
    }
    if (no_entering(P, min_e, p)) {  // OptimumFound (v4:299-302)
        if (blockIdx.x == 0 && tid == 0) {
            st->p = p;
            st->min_e = (P.devex && (P.defer_price || dvx_grp)) ? e_enter : min_e;
            st->status = ST_OPTIMAL;
            if (DEFER) P.trec->fresh = 0;
        }
        return;
    }
    // ---- the one p-dependent round trip: A_p on the list and at row i, the
    // winner's window coefficients, the bookkeeping scalars (thread 0)
    // (only the S list slots: every workgroup gathers the same column, so
    // slots past S would multiply the L2 requests for nothing)
    const double* apd = P.A + p * P.L;
    double apv[BC_RL];
#pragma unroll
    for (int j = 0; j < BC_RL; ++j) apv[j] = (tid + j * BLOCK < Sbc) ? apd[rlv[j]] : 0.0;
    double auv[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) auv[r] = apd[icl[r]];
    const double* wrec = P.mbox_fused ? s_fw
                                      : (P.nin > 1 ? reinterpret_cast<const double*>(P.price_in + gw * P.pr_stride + 1)
                                                   : P.Wt + p * KW);
    const double wlr = wrec[lane < KW ? lane : 0];
    TailPre tpre{0, 0.0, 0, -1, -1, 0.0, 0, 0.0, 0};
    if (!DEFER && tid == 0 && !P.split_tail) tpre = tail_prefetch(P, Sv.nw, Sv.nb_count, p);
    // deferred tail: workgroup 0 records tail_prefetch's scalars (as scalars:
    // the record written from tpre kept tpre in scratch)
    double rc_p = 0.0, rwp = 0.0;
    int32_t rkp = -1, rlast = -1;
    if (DEFER && blockIdx.x == 0 && tid == 0) {
        rc_p = P.c[p];
        if (owns_col(P, p)) {
            rkp = P.nb_pos[p];
            rlast = P.nb_list[Sv.nb_count - 1];
        }
        if (P.devex) rwp = dvx_grp ? wp_grp : P.W[p];
    }
    if (P.defer_price || dvx_grp) {
        tpre.has_e = true;
        tpre.e_enter = e_enter;
    }
    if (dvx_grp) tpre.wp = wp_grp;
    const int64_t it = Sv.iter;
    const int par = (int)(it & 1);
    double* a_new = par ? P.alpha0 : P.alpha1;
    const double aqp = Sv.aq;
    const bool upd_x = Sv.xb_applied < it;
    double ei[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) ei[r] = (pend && rowv[r]) ? eta_entry(par ? al1[r] : al0[r], irow[r], qp, aqp) : 0.0;
    unsigned long long* const win = nullptr;
    // ---- compact FTRAN (as k_update BC): the unit term first (lane 0), then
    // this lane's chunks lane + 64 t ascending, .x before .y; A_p gathered
    // onto the list in LDS blocks of BC_APC columns
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* apc = reinterpret_cast<double*>(smem + RED_BYTES);
    const dbl2* apc2 = reinterpret_cast<const dbl2*>(apc);
    const int S = Sbc;
    double a[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) a[r] = (rowv[r] && lane == 0 && rmv[r] < 0) ? auv[r] : 0.0;
    for (int cb = 0; cb < S || cb == 0; cb += BC_APC) {
        const int ce = S < cb + BC_APC ? S : cb + BC_APC;
        if (cb > 0) lds_barrier();  // the previous block's reads are done
#pragma unroll
        for (int j = 0; j < BC_RL; ++j) {
            const int c = tid + j * BLOCK;
            if (cb == 0 && c < ce) apc[c] = apv[j];
        }
        for (int c = cb + (cb == 0 ? BC_RL * BLOCK : 0) + tid; c < ce; c += BLOCK) apc[c - cb] = apd[P.rlist[c]];
        lds_barrier();
        if (wgt && cb == 0) wgt[2] = rtime();
        const int kb = cb >> 1, ke = (ce + 1) >> 1;  // this block's dbl2 chunks
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            if (rowv[r]) {
                auto take = [&](dbl2 v, int k2) {
                    const dbl2 w = apc2[k2 - kb];
                    if (2 * k2 < S) a[r] = fma(v.x, w.x, a[r]);
                    if (2 * k2 + 1 < S) a[r] = fma(v.y, w.y, a[r]);
                };
                if (cb == 0) {
#pragma unroll
                    for (int t = 0; t < NCH; ++t) {
                        const int k2 = lane + 64 * t;
                        if (k2 < ke) take(pf[r][t], k2);
                    }
                }
                for (int k0 = (cb == 0 ? NCH * 64 : kb); k0 < ke; k0 += 8 * 64) {
                    dbl2 v[8];
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        const int k2 = k0 + lane + 64 * t;
                        v[t] = brow[r][k2 < ke ? k2 : kb];
                    }
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        const int k2 = k0 + lane + 64 * t;
                        if (k2 < ke) take(v[t], k2);
                    }
                }
            }
        }
    }
    // ---- window terms, the pending eta column, s_x (the row's stores wait
    // until the partial is out: a wave's vmcnt counts its stores, so stores
    // issued before the merge put their write acknowledgements on the path
    // to the publish)
    const double wl = lane < Sv.nw ? wlr : 0.0;
    double acc[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        acc[r] = 0.0;
        if (rowv[r]) {
            const double cu = lane < tau ? urow[r] : (lane == tau ? ei[r] : 0.0);
            acc[r] = fma(cu, wl, a[r]);
        }
    }
    double sxw = 0.0;
    if (pend) sxw = sx_x + wave_sum(lane < tau ? mul_nc(sxw_u, sxw_w) : 0.0);
    const double s_x = upd_x ? sxw : 0.0;

    // ---- x_b += s_x E (v4:348), alpha_i, theta_i (v4:199-208), the partials
    // (the RPW rows' butterflies interleaved: each value's own bits)
    auto rows_step = [&](auto off_t) {
        constexpr int OFF = decltype(off_t)::value;
        double t[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) t[r] = xor_partner<OFF>(acc[r]);
#pragma unroll
        for (int r = 0; r < RPW; ++r) acc[r] += t[r];
    };
    rows_step(std::integral_constant<int, 32>());
    rows_step(std::integral_constant<int, 16>());
    rows_step(std::integral_constant<int, 8>());
    rows_step(std::integral_constant<int, 4>());
    rows_step(std::integral_constant<int, 2>());
    rows_step(std::integral_constant<int, 1>());
    UpdPartial wp[RPW];
    double al[RPW], xb[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        wp[r] = upd_empty();
        al[r] = 0.0;
        xb[r] = xb0[r];
        if (rowv[r]) {
            al[r] = acc[r];
            if (upd_x) xb[r] = fma(s_x, ei[r], xb[r]);
            const bool pos = al[r] > P.piv_tol;
            const double th = ratio_key(P, xb[r], al[r]);
            wp[r].nonpos += !pos;
            wp[r].T = fma(cbv[r], al[r], wp[r].T);
            if (argmin_better(th, irow[r], wp[r].theta, wp[r].idx)) {
                wp[r].theta = th;
                wp[r].idx = irow[r];
                wp[r].a_w = al[r];
                wp[r].cb_w = cbv[r];
                wp[r].bix_w = bix[r];
            }
        }
    }
    // alpha_i (read back by the next pass / k_flush), x_b, the pending eta
    // entry into U, and the basic columns' Wt entries (s_x in Wt[n])
    auto store_row = [&]() {
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            if (rowv[r] && lane == 0) {
                const int64_t i = irow[r];
                if (pend) P.U[i * KW + tau] = ei[r];
                a_new[i] = al[r];
                if (upd_x) P.x_b[i] = xb[r];
                if (pend) P.Wt[bix[r] * KW + tau] = (i == qp) ? aqp : 0.0;
            }
        }
        if (pend && blockIdx.x == 0 && tid == 0) P.Wt[P.n * KW + tau] = sxw;
    };
    // (the counted and tagged hand-offs: stores first, as their tail's polls
    // would otherwise wait behind them; deferred: after the publish)
    if constexpr (!DEFER) store_row();
    UpdPartial* red = reinterpret_cast<UpdPartial*>(smem + Lds::red);
    int* s_last = reinterpret_cast<int*>(smem + Lds::last);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < RPW; ++r) red[r * WAVES + wave] = wp[r];
    }
    lds_barrier();
    if (P.split_tail) {  // k_tail merges after the kernel boundary
        if (tid == 0) {
            UpdPartial w = red[0];
            for (int k = 1; k < WAVES; ++k) upd_merge(w, red[k]);
            upd_publish(P, blockIdx.x, w);
        }
        return;
    }
    if constexpr (DEFER) {  // the next pricing pass (or k_apply_tail) reduces the partials
        if (tid < RPW) {
            const int r = tid;
            const int g = blockIdx.x * RPW + r;
            UpdPartial w = red[r * WAVES];
            for (int k = 1; k < WAVES; ++k) upd_merge(w, red[r * WAVES + k]);
            if (g < P.tail_parts) upd_publish<true>(P, g, w);
            if (wgt) wgt[3] = rtime();
            if (g == 0) {
                TailRec* rec = P.trec;
                rec->it = it;
                rec->p = p;
                rec->e_rep = !P.devex ? min_e : ((P.defer_price || dvx_grp) ? e_enter : *P.dvx_e);
                rec->c_p = rc_p;
                rec->wp = rwp;
                rec->cnt = Sv.nb_count;
                rec->kp = rkp;
                rec->last = rlast;
                rec->nw = Sv.nw;
                rec->fresh = 1;
            }
        }
        if constexpr (SEF && RPW == 1) {
            {
                // steepest edge, k_se_part's sums fused (the pending pivot is
                // this pass's: alpha = al, U[i][s] for s <= tau = cu): this
                // workgroup's rows' terms of M^T alpha for M = [B_w at the S
                // listed columns | U[:, s < nw] | alpha], summed over its waves
                // in row order, in LDS blocks of sec columns (the A_p list's
                // space: every wave has passed its last read of it)
                const int64_t Ls = P.L;
                const int ncol = S + KW + 1;
                const int sec = (int)((Ls < BC_APC ? Ls : BC_APC) / WAVES);
                const double av = rowv[0] ? al[0] : 0.0;
                const double cuv = rowv[0] ? (lane < tau ? urow[0] : (lane == tau ? ei[0] : 0.0)) : 0.0;
                const double* rowp = bcb + icl[0] * ldc;
                double* outp = P.se_part + (int64_t)blockIdx.x * (Ls + KW + 1);
                double* sp = apc + wave * sec;
                for (int c0 = 0; c0 < ncol; c0 += sec) {
                    const int c1 = ncol < c0 + sec ? ncol : c0 + sec;
                    if (c0 > 0) lds_barrier();  // the previous block's sums are read
                    for (int c = c0 + lane; c < c1; c += 64) {
                        if (c < S) sp[c - c0] = rowp[c] * av;
                        else if (c == S + KW) sp[c - c0] = av * av;
                    }
                    if (lane < KW && S + lane >= c0 && S + lane < c1) sp[S + lane - c0] = cuv * av;
                    lds_barrier();
                    for (int c = c0 + tid; c < c1; c += BLOCK) {
                        double t = apc[c - c0];
#pragma unroll
                        for (int w = 1; w < WAVES; ++w) t += apc[w * sec + c - c0];
                        outp[c] = t;
                    }
                }
            }
        }
        store_row();
        return;
    }
    if (P.upd_tag) {  // tagged hand-off to the last workgroup
        const uint32_t tag = (uint32_t)(it + 1);
        if (wave == 0) {
            UpdPartial w = red[0];
            for (int k = 1; k < WAVES; ++k) upd_merge(w, red[k]);
            upd_publish_tagged(P, blockIdx.x, w, tag, lane);
            if (wgt) wgt[3] = rtime();
        }
        if (blockIdx.x != gridDim.x - 1) return;
        const unsigned long long t_tail = slot ? rtime() : 0;
        update_tail<BLOCK>(P, st, p, min_e, it, smem, gridDim.x, &tpre, tag);
        stamp_tail(slot, t_tail, win);
        if (wgt) P.stamps[STAMP_TAIL + (it & 1)] = rtime();  // the bookkeeping is issued
        return;
    }
    if (tid == 0) {
        UpdPartial w = red[0];
        for (int k = 1; k < WAVES; ++k) upd_merge(w, red[k]);
        upd_publish(P, blockIdx.x, w);
        drain_vmem();  // the partial is visible before the ticket
        *s_last = arrive_last(arrive_group(P.arrive, ARR_UPDATE), gridDim.x, blockIdx.x);
    }
    lds_barrier();
    if (!*s_last) return;
    const unsigned long long t_tail = slot ? rtime() : 0;
    update_tail<BLOCK>(P, st, p, min_e, it, smem, gridDim.x, &tpre);
    stamp_tail(slot, t_tail, win);
}
// Window tableau FTRAN (spx_tabdev.h): one lane per row,
// alpha_i = T_w[i,p] + sum_s U[i][s] Wt[p][s] — no B_w stream — then the
// pending eta column into U, the basic columns' Wt entries, x_b, the ratio
// test (v4:199-208) and, in the last workgroup, k_update's tail.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_tab_update(Params P) {
    DevState* st = P.st;
    if (stopped(st)) return;
    constexpr int WAVES = BLOCK / 64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double s_wp[64];
    // entering column, as k_update
    double min_e = INFINITY, e_enter = 0.0;
    int64_t p = INT64_MAX;
    if (P.defer_price) {
        PricePartial w{INFINITY, INT64_MAX, 0.0, 0.0};
        for (int g = tid; g < P.price_grid; g += BLOCK) {
            const PricePartial v = P.price_partials[g];
            if (argmin_better(v.val, v.idx, w.val, w.idx)) w = v;
        }
        wave_price_min(w.val, w.idx, w.w, w.pad);
        __shared__ PricePartial s_pw[WAVES];
        if (lane == 0) s_pw[wave] = w;
        __syncthreads();
        PricePartial t = s_pw[0];
        for (int i = 1; i < WAVES; ++i)
            if (argmin_better(s_pw[i].val, s_pw[i].idx, t.val, t.idx)) t = s_pw[i];
        min_e = t.val;
        p = t.idx;
        e_enter = t.pad;
    } else {
        for (int g = 0; g < P.nin; ++g) {
            const ArgMinEntry e = P.price_in[g * P.pr_stride];
            if (argmin_better(e.val, e.idx, min_e, p)) { min_e = e.val; p = e.idx; }
        }
    }
    if (no_entering(P, min_e, p)) {  // OptimumFound (v4:299-302)
        if (blockIdx.x == 0 && tid == 0) {
            st->p = p;
            st->min_e = (P.devex && P.defer_price) ? e_enter : min_e;
            st->status = ST_OPTIMAL;
        }
        return;
    }
    const int64_t it = st->iter;
    const int par = (int)(it & 1);
    const int64_t m = P.m, L = P.L;
    const int KW = P.win;
    const double* a_prev = par ? P.alpha1 : P.alpha0;
    double* a_new = par ? P.alpha0 : P.alpha1;
    const int nw = st->nw;
    const int tau = nw - 1;
    const bool pend = nw > 0;
    const int64_t qp = st->q;
    const double aqp = st->aq;
    const bool upd_x = st->xb_applied < it;
    if (tid < 64) s_wp[tid] = (tid < nw) ? P.Wt[p * KW + tid] : 0.0;
    // s_x = r_tau . b = xw[q] + sum_{s<tau} U[q][s] Wt[n][s] (v4:347), as k_update
    double sxw = 0.0;
    if (pend) {
        sxw = lane < tau ? mul_nc(P.U[qp * KW + lane], P.Wt[P.n * KW + lane]) : 0.0;
        sxw = P.xw[qp] + wave_sum(sxw);
        if (blockIdx.x == 0 && tid == 0) P.Wt[P.n * KW + tau] = sxw;
    }
    const double s_x = upd_x ? sxw : 0.0;
    TailPre tpre{0, 0.0, 0, -1, -1, 0.0, 0, 0.0, 0};
    if (tid == 0 && !P.split_tail) tpre = tail_prefetch(P, st->nw, st->nb_count, p);
    if (P.defer_price) {
        tpre.has_e = true;
        tpre.e_enter = e_enter;
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLOCK + tid;
    const bool rv = i < m;
    UpdPartial wp = upd_empty();
    if (rv) {
        const double t = P.T[p * L + i];
        const double ei = pend ? eta_entry(a_prev[i], i, qp, aqp) : 0.0;
        const double a = tab_ftran_row(t, tau, ei, s_wp, [&](int s2) { return P.U[i * KW + s2]; });
        const int64_t bix = P.b_ixs[i];
        const double cb = P.c_B[i];
        double x = P.x_b[i];
        if (pend) {
            P.U[i * KW + tau] = ei;
            P.Wt[bix * KW + tau] = (i == qp) ? aqp : 0.0;  // r_tau.A_j of the basic columns
        }
        if (upd_x) {
            x = fma(s_x, ei, x);
            P.x_b[i] = x;
        }
        a_new[i] = a;
        // one row: the candidate whatever its key (first index on ties, as
        // k_update's argmin_better against the empty partial)
        wp.theta = ratio_key(P, x, a);
        wp.idx = i;
        wp.nonpos = !(a > P.piv_tol);
        wp.T = cb * a;
        wp.a_w = a;
        wp.cb_w = cb;
        wp.bix_w = bix;
    }
    wp = wave_upd_merge(wp);
    UpdPartial* red = reinterpret_cast<UpdPartial*>(smem + UpdLds<BLOCK>::red);
    int* s_last = reinterpret_cast<int*>(smem + UpdLds<BLOCK>::last);
    if (lane == 0) red[wave] = wp;
    __syncthreads();
    if (tid == 0) {
        UpdPartial w = red[0];
        for (int k = 1; k < WAVES; ++k) upd_merge(w, red[k]);
        if (P.split_tail) {
            upd_publish(P, blockIdx.x, w);
        } else {
            upd_publish(P, blockIdx.x, w);
            drain_vmem();
            *s_last = arrive_last(arrive_group(P.arrive, ARR_UPDATE), gridDim.x, blockIdx.x);
        }
    }
    if (P.split_tail) return;  // k_tail merges after the kernel boundary
    __syncthreads();
    if (!*s_last) return;
    update_tail<BLOCK>(P, st, p, min_e, it, smem, gridDim.x, &tpre);
}

// The pivot tail as its own one-workgroup launch (split_tail): the k_update
// workgroups stored their partials plainly and returned; the kernel boundary
// makes them visible here.
__global__ __launch_bounds__(1024) void k_tail(Params P, int nparts) {
    DevState* st = P.st;
    if (stopped(st)) return;  // also when k_update found the optimum
    __shared__ __attribute__((aligned(16))) unsigned char smem[UpdLds<1024>::bytes];
    double min_e = INFINITY;
    int64_t p = INT64_MAX;
    for (int g = 0; g < P.nin; ++g) {
        const ArgMinEntry e = P.price_in[g * P.pr_stride];
        if (argmin_better(e.val, e.idx, min_e, p)) { min_e = e.val; p = e.idx; }
    }
    const int64_t it = st->iter;
    if (P.row_shard)
        update_tail_rs<1024>(P, st, it, (int)(it & 1), (it & 1) ? P.alpha1 : P.alpha0, smem, nparts);
    else if (P.ratio == RATIO_HARRIS)
        harris_tail<1024>(P, st, p, min_e, it, smem, nparts);
    else
        update_tail<1024>(P, st, p, min_e, it, smem, nparts);
}

// A pending deferred tail applied on its own (before a fold, at the end of a
// batch of passes, before any readback): one workgroup of 512 threads, the
// reduction shape of the FTRAN tail and of k_price (the same bits).  Clears
// the record either way.
__global__ __launch_bounds__(512) void k_apply_tail(Params P) {
    DevState* st = P.st;
    const TailRec R = *P.trec;
    if (!R.fresh) return;
    if (R.it == st->iter) {  // not yet applied by a pricing pass
        __shared__ UpdPartial s_ured[9];
        const UpdPartial t = reduce_update_partials<512, true>(P, s_ured, P.tail_parts);
        if (threadIdx.x == 0) apply_deferred_tail(P, st, R, t);
    }
    if (threadIdx.x == 0) P.trec->fresh = 0;
}

// Row-sharded pivot finalisation (one workgroup, after the ratio-test
// all-gather): global leaving row q = MINLOC over the ranks' headers
// (v4:324), Unbounded if every alpha_i <= 0 (v4:317-322), the pivot row into
// rbuf, s_y (v4:352-355; c_B_new.E_q evaluated from the gathered sum
// T = sum_i c_B[i] alpha_i as -(T - c_Bq alpha_q)/alpha_q + c_p (1/alpha_q - 1),
// since alpha is distributed), and the basis bookkeeping (v4:339-342).
__global__ __launch_bounds__(256) void k_finalize_rs(Params P) {
    DevState* st = P.st;
    if (stopped(st)) return;
    const int tid = threadIdx.x;
    double min_e = INFINITY;
    int64_t p = INT64_MAX;
    for (int g = 0; g < P.nin; ++g) {
        const ArgMinEntry e = P.price_in[g * P.pr_stride];
        if (argmin_better(e.val, e.idx, min_e, p)) { min_e = e.val; p = e.idx; }
    }
    // merge the ranks' ratio-test headers (rank order: deterministic T sum)
    double th = INFINITY, T = 0.0;
    int64_t q = INT64_MAX, nonpos = 0;
    int w = -1;
    for (int g = 0; g < P.nin; ++g) {
        const RsHeader* h = reinterpret_cast<const RsHeader*>(P.rs_recv + g * P.rs_stride);
        if (argmin_better(h->theta, h->idx, th, q)) { th = h->theta; q = h->idx; w = g; }
        nonpos += h->nonpos;
        T += h->T;
    }
    const int64_t it = st->iter;
    if (nonpos == P.m || q < 0 || q >= P.m || w < 0) {
        if (tid == 0) {
            st->p = p;
            st->min_e = min_e;
            st->status = ST_UNBOUNDED;
        }
        return;
    }
    const RsHeader* hw = reinterpret_cast<const RsHeader*>(P.rs_recv + w * P.rs_stride);
    const dbl2* row = reinterpret_cast<const dbl2*>(P.rs_recv + w * P.rs_stride + sizeof(RsHeader));
    dbl2* rb = reinterpret_cast<dbl2*>(P.rbuf);
    for (int64_t k = tid; k < (P.L >> 1); k += 256) rb[k] = row[k];
    if (tid == 0)
        pivot_bookkeeping(P, st, p, q, hw->bix_w, hw->a_w, y_scalar(T, hw->a_w, hw->cb_w, P.c[p]), min_e, it);
}

// ---------------------------------------------------------------------------
// Host-side launchers
// ---------------------------------------------------------------------------
template <int BLOCK, int R, bool RS, bool WIN, int BNT = 1, bool BC = false>
static hipError_t launch_update_k(const Params& P, int grid, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    const size_t lds = UpdLds<BLOCK>::bytes +
                       ((WIN && BC) ? (size_t)(P.L < BC_APC ? P.L : BC_APC) * 8 : 0) +
                       ((!WIN && !RS && upd_xlds(P)) ? (size_t)P.L * 24 : 0);
    if (lds > 65536) {  // once per instantiation and device (idempotent; not a stream operation)
        static std::atomic<uint64_t> raised{0};
        int dev = 0;
        const hipError_t ed = hipGetDevice(&dev);
        if (ed != hipSuccess) return ed;
        const uint64_t bit = 1ull << (dev & 63);
        if (!(raised.load(std::memory_order_acquire) & bit)) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_update<BLOCK, R, RS, WIN, BNT, BC>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024);
            if (e != hipSuccess) return e;
            raised.fetch_or(bit, std::memory_order_release);
        }
    }
    if (e0 || e1) {
        hipExtLaunchKernelGGL((k_update<BLOCK, R, RS, WIN, BNT, BC>), dim3(grid), dim3(BLOCK), (uint32_t)lds, s, e0, e1, 0,
                              P);
    } else {
        hipLaunchKernelGGL((k_update<BLOCK, R, RS, WIN, BNT, BC>), dim3(grid), dim3(BLOCK), lds, s, P);
    }
    return hipGetLastError();
}

// grid: the one-row grid's workgroups (= partial slots); RPW rows per wave
// take ceil(grid / RPW) workgroups
template <int BLOCK, bool DEFER, int RPW, bool SEF = false>
static hipError_t launch_ftran_bc_t(const Params& P, int grid, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    const size_t red = RPW == 1 ? UpdLds<BLOCK>::bytes : sizeof(UpdPartial) * (BLOCK / 64) * RPW + 16;
    const size_t lds = red + (size_t)(P.L < BC_APC ? P.L : BC_APC) * 8;
    const int g = (grid + RPW - 1) / RPW;
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ftran_bc<BLOCK, DEFER, RPW, SEF>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024);
        if (e != hipSuccess) return e;
    }
    if (e0 || e1)
        hipExtLaunchKernelGGL((k_ftran_bc<BLOCK, DEFER, RPW, SEF>), dim3(g), dim3(BLOCK), (uint32_t)lds, s, e0, e1, 0, P);
    else
        hipLaunchKernelGGL((k_ftran_bc<BLOCK, DEFER, RPW, SEF>), dim3(g), dim3(BLOCK), lds, s, P);
    return hipGetLastError();
}

// deferred ratio-test tail: its own instantiation (no tail code, and the
// tail's registers stay out of the hand-off kernel); rows per wave (the
// deferred form only; bc_entry = SPX_FTRAN_RPW, UpdateCfg)
template <int BLOCK>
static hipError_t launch_ftran_bc(const Params& P, int grid, int rpw, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (!P.defer_tail) return launch_ftran_bc_t<BLOCK, false, 1>(P, grid, s, e0, e1);
    if constexpr (BLOCK == 512) {
        if (rpw == 2) return launch_ftran_bc_t<BLOCK, true, 2>(P, grid, s, e0, e1);
        if (rpw == 4) return launch_ftran_bc_t<BLOCK, true, 4>(P, grid, s, e0, e1);
        if (P.se_fused) return launch_ftran_bc_t<BLOCK, true, 1, true>(P, grid, s, e0, e1);
    }
    return launch_ftran_bc_t<BLOCK, true, 1>(P, grid, s, e0, e1);
}

template <int BLOCK, int R>
static hipError_t launch_update_t(const Params& P, int grid, int bc_entry, hipStream_t s, hipEvent_t e0,
                                  hipEvent_t e1) {
    if (P.row_shard) return launch_update_k<BLOCK, R, true, false>(P, grid, s, e0, e1);
    if (!P.win) return launch_update_k<BLOCK, R, false, false>(P, grid, s, e0, e1);
    // B_w loads: default policy while B_w fits the Infinity Cache beside the
    // window state (spx_common.h SPX_NT_BWIN), non-temporal beyond
    if (P.bc) {  // compact FTRAN
        if (R == 1 && bc_entry) return launch_ftran_bc<BLOCK>(P, grid, bc_entry, s, e0, e1);
        return launch_update_k<BLOCK, R, false, true, 0, true>(P, grid, s, e0, e1);
    }
    if (win_b_cached(P)) return launch_update_k<BLOCK, R, false, true, 0>(P, grid, s, e0, e1);
    return launch_update_k<BLOCK, R, false, true, 1>(P, grid, s, e0, e1);
}

hipError_t launch_tail(const Params& P, int nparts, hipStream_t s) {
    hipLaunchKernelGGL(k_tail, dim3(1), dim3(1024), 0, s, P, nparts);
    return hipGetLastError();
}

hipError_t launch_apply_tail(const Params& P, hipStream_t s) {
    if (!P.trec) return hipSuccess;
    hipLaunchKernelGGL(k_apply_tail, dim3(1), dim3(512), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_finalize_rs(const Params& P, hipStream_t s) {
    hipLaunchKernelGGL(k_finalize_rs, dim3(1), dim3(256), 0, s, P);
    return hipGetLastError();
}

template <int BLOCK>
static hipError_t launch_update_b(const Params& P, const UpdateCfg& c, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    switch (c.rows) {
        case 1: return launch_update_t<BLOCK, 1>(P, c.grid, c.bc_entry, s, e0, e1);
        case 2: return launch_update_t<BLOCK, 2>(P, c.grid, c.bc_entry, s, e0, e1);
        case 4: return launch_update_t<BLOCK, 4>(P, c.grid, c.bc_entry, s, e0, e1);
        case 8:
            if constexpr (BLOCK <= 512) return launch_update_t<BLOCK, 8>(P, c.grid, c.bc_entry, s, e0, e1);
            break;
    }
    return hipErrorInvalidValue;
}

// Diagnostic (SPX_DIAG_MARK=1 with stamps): a one-wave kernel before the
// FTRAN launch records when it starts, splitting the pricing -> FTRAN
// boundary into the pricing kernel's end and the FTRAN kernel's start
__global__ __launch_bounds__(64) void k_mark(Params P) {
    const unsigned long long now = rtime();
    if (threadIdx.x == 0 && P.stamps) P.stamps[STAMP_TAIL + 2 + (P.st->iter & 1)] = now;
}

hipError_t launch_update(const Params& P, const UpdateCfg& c, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (P.stamps && c.mark) hipLaunchKernelGGL(k_mark, dim3(1), dim3(64), 0, s, P);
    if (P.tab) {  // window tableau: k_tab_update, 256 rows per workgroup
        const size_t lds = UpdLds<256>::bytes;
        if (e0 || e1)
            hipExtLaunchKernelGGL((k_tab_update<256>), dim3(c.grid), dim3(256), (uint32_t)lds, s, e0, e1, 0, P);
        else
            hipLaunchKernelGGL((k_tab_update<256>), dim3(c.grid), dim3(256), lds, s, P);
        return hipGetLastError();
    }
    switch (c.block) {
        case 256: return launch_update_b<256>(P, c, s, e0, e1);
        case 512: return launch_update_b<512>(P, c, s, e0, e1);
        case 1024: return launch_update_b<1024>(P, c, s, e0, e1);
    }
    return hipErrorInvalidValue;
}

}  // namespace spx
