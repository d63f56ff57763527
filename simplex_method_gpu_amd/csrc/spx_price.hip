// spx_price.hip — k_price, the pricing launch of a loop pass (the pass is
// described at the head of spx_kernels.h), its pricing-only build switches
// and its launchers.  The deferred tail and the mailbox record it shares with
// the FTRAN kernels are in spx_handoff.h.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>

#include "spx_device.h"
#include "spx_common.h"
#include "spx_cprows.h"
#include "spx_handoff.h"
#include "spx_kernels.h"
#include "spx_tabdev.h"

namespace spx {

#ifndef SPX_LDS_BATCH
#define SPX_LDS_BATCH 4  // eta-window pricing: y / base-row LDS reads issued together
#endif
#ifndef SPX_PRICE_CH
#define SPX_PRICE_CH 8  // chunks of a column's start prefetched (8-wave workgroups)
#endif
#ifndef SPX_PRICE_DEEP
#define SPX_PRICE_DEEP 1  // deferred tail: the first column's first 16 chunks requested before the reduction
#endif
#ifndef SPX_SE_LDS_BATCH
// steepest edge (WM 4): its LDS operand batch (0 = SPX_LDS_BATCH); 2 frees
// the registers its two-batch deep prefetch needs (248 VGPRs, no spills)
#define SPX_SE_LDS_BATCH 2
#endif
#ifndef SPX_PRICE_DEEP_SE
// steepest edge (WM 4): the first column's first 8 (1) or 16 (2, the default
// since round 6: k_price 0.711 -> 0.721 of 8 TB/s, pass 87.9 -> 86.4 us,
// profiles/r06_steepest_ab.txt) chunks requested before the deferred-tail reduction
#define SPX_PRICE_DEEP_SE 2
#endif
#ifndef SPX_PRICE_DYN_PCT
#define SPX_PRICE_DYN_PCT 85  // the share of the columns handed out statically (grid stride)
#endif
#ifndef SPX_PRICE_PIPE
#define SPX_PRICE_PIPE 1  // eta-window pricing: two 8-chunk batches of a column in flight
#endif

// ---------------------------------------------------------------------------
// Pricing + entering argmin
// ---------------------------------------------------------------------------
// The workgroup's best wave partial, chosen on (val, idx) scalars and read
// back from LDS by index: selecting whole PricePartial structs in a loop put
// the running winner in scratch, and a kernel with a private segment paid
// about 4 us more at its kernel boundary
template <int WAVES>
__device__ __forceinline__ int best_wave(const PricePartial* red) {
    double bv = red[0].val;
    int64_t bi = red[0].idx;
    int bk = 0;
#pragma unroll
    for (int i = 1; i < WAVES; ++i) {
        const double v = red[i].val;
        const int64_t x = red[i].idx;
        if (argmin_better(v, x, bv, bi)) {
            bv = v;
            bi = x;
            bk = i;
        }
    }
    return bk;
}

// WM: 0 = explicit B^-1 (y updated in the LDS fill); 1 = eta window with the
// pending base row in LDS next to y; 2 = eta window, base row read from global
// (L2) when y and the row do not both fit; 3 = window tableau (P.tab): no A
// stream, each column reads T_w[q_tau, j], dw[j] and its Wt row; 4 / 5 = 1 / 2
// with steepest-edge pricing (P.steep): a third dot v.A_j per column, v =
// B_w^T alpha (P.se_v) in LDS beside y and the base row (4) or from global (5).
// TK: the ticketed tail compiled in for WM 1 (a separate instantiation, so the
// static C3 pass keeps its code: carrying the disabled ticket branches cost
// it 0.5 us per pass); WM 2 always carries it
// WM 6 = compact pricing (P.AS, spx_device.h): no A stream; a column's base
// row dot comes from the listed rows of A, y_w . A_j - c_j from dw[j].
// WM 7 = WM 6 with the row form of the column loop (spx_cprows.h) for lists
// within the row limit, the gather form for the others.  An instantiation of
// its own: compiled beside the row form, the whole pass (its prologue as
// well) is allocated and scheduled differently and the gather form runs 1.6
// us slower at C3, so a context without the row form (SPX_CPRICE_ROWS=0)
// launches WM 6, whose code stays what it was.
// DW: the dense pass (WM 1 / 2) that opens a compact-priced window: it also
// stores dw[j] for every column it prices and marks dw valid (its own
// instantiations, so the plain dense pass keeps its code)
template <int BLOCK, bool LDS_Y, int WM, bool TK = false, bool DW = false>
__global__ __launch_bounds__(BLOCK) void k_price(Params P) {
    DevState* st = P.st;
    constexpr int WAVES = BLOCK / 64;
    constexpr bool WIN = WM != 0;
    constexpr bool CP = WM == 6 || WM == 7;
    constexpr bool CPR = WM == 7;  // compact pricing with the row form beside the gather form
    static_assert(!DW || WM == 1 || WM == 2, "dw is stored by the dense window passes");
    constexpr bool LDS_R = WM == 1 || WM == 4;
    constexpr bool SE = WM == 4 || WM == 5;
    constexpr bool LDS_V = WM == 4;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int idx0 = blockIdx.x * WAVES + wave;
    // speculative: this wave's first non-basic column, loaded together with the
    // status word (index clamped into the list; validated against nb_count)
    int64_t j0 = P.nb_list[idx0 < P.n ? idx0 : P.n - 1];
    const unsigned long long t_pw0 = P.stamps ? rtime() : 0ull;
    // Deferred tail: the record and this thread's partial(s) are requested at
    // entry beside the column and the state -- unconditionally (clamped
    // slot), so no test of the record or the state sits between them: a
    // branch there made the compiler wait for the state, then for the
    // record, before the partials were even requested (three round trips)
    // (a record of zeros when there is none: a branch around these loads
    // moved the record's uniform fields into SGPRs inside it, i.e. waited)
    // Only the compact window passes defer the tail (the explicit form and the
    // tableau never do: no record, no partials, no loads)
    constexpr bool PAIR = BLOCK == 256;  // (two partials of the 512-thread shape per thread)
    constexpr bool DT = WM != 0 && WM != 3;
    TailRec R{};
    if constexpr (DT) R = *(P.defer_tail ? P.trec : reinterpret_cast<const TailRec*>(P.zeros));
    // compact pricing: the list's shape, the operand's active buffer and pitch,
    // and whether dw belongs to this y_w (uniform loads, beside the record's)
    int cp_S = 0, cp_ld = 64, cp_sel = 0, cp_dw = 0;
    if constexpr (CP) {
        cp_S = P.bc_n[0];
        cp_ld = P.bc_n[1];
        cp_sel = P.bc_n[2];
        cp_dw = P.bc_n[5];
    }
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    constexpr int SW = (int)(sizeof(DevState) / 16);
    u32x4 sw[SW];  // the state as raw words (st_snapshot's loads)
#pragma unroll
    for (int i = 0; i < SW; ++i) sw[i] = reinterpret_cast<const u32x4*>(st)[i];
    UpdPartial w0 = upd_empty(), w1 = upd_empty();
    if constexpr (DT) {
        const int tp = P.tail_parts > 0 ? P.tail_parts : 1;
        w0 = upd_fetch<true>(P, tid < tp ? tid : tp - 1);
        if constexpr (PAIR) w1 = upd_fetch<true>(P, tid + BLOCK < tp ? tid + BLOCK : tp - 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    // (every state word held until here: a dead word's register, reused
    // early, made the partials' loads wait for the state)
#pragma unroll
    for (int i = 0; i < SW; ++i) asm volatile("" ::"v"(sw[i]));
    const DevState S = __builtin_bit_cast(DevState, sw);
    // the fields the pass prices with (fresh: derived from the deferred tail;
    // kept as scalars -- assigning into the snapshot put it in scratch)
    int64_t s_iter = S.iter, s_q = S.q, s_leave = S.leave;
    double s_aq = S.aq, s_sy = S.s_y, s_wp = S.wp;
    int32_t s_nb = S.nb_count, s_nw = S.nw;
    // Deferred ratio-test tail (TailRec, P.defer_tail): the previous FTRAN
    // pass left its workgroup partials and this record.  Every workgroup
    // reduces the partials itself (the same reduction as the FTRAN tail, so
    // the same bits) and prices with the state the bookkeeping produces;
    // workgroup 0 applies that bookkeeping meanwhile.  No workgroup reads a
    // state word workgroup 0 writes: the list is read through the two slots
    // the pivot changes (nbl), SY[tau] is the derived s_y.
    bool fresh = false;
    int32_t pk_a = -1, pk_b = -1;
    int64_t pv_a = 0, pv_b = 0;
    constexpr int CH = (BLOCK <= 512 && WM != 3) ? SPX_PRICE_CH : 8;
    constexpr int LB = (WM == 4 && SPX_SE_LDS_BATCH > 0) ? SPX_SE_LDS_BATCH : SPX_LDS_BATCH;  // LDS operand batch
    // SPX_PRICE_DEEP (deferred tail): the first column's first 2 CH chunks are
    // requested as soon as the tail's record says which column this slot
    // holds after the pivot's list edit -- before the partials are reduced
    // and the base row staged -- so HBM streams during the prologue instead
    // of idling (only the end-of-list slot depends on q; it is left out)
    // Only with y_w and the base row both staged in LDS (WM 1, the C3 / C4
    // shape): with the base row read from L2 (WM 2, C5) it measured 4.6 %
    // slower per pass (1,071 against 1,022 us, tools/pass_ab.py).
    // (only run_pipe consumes vd0 / vd1, so DEEP needs the pipelined loop)
    // (steepest edge, WM 4: both batches with its LDS operand batch at 2,
    // SPX_SE_LDS_BATCH; at the default batch the second one spilled)
    constexpr bool DEEP2 = SPX_PRICE_DEEP && SPX_PRICE_PIPE && BLOCK <= 512 && CH == 8 &&
                           (WM == 1 || (SPX_PRICE_DEEP_SE == 2 && WM == 4));
    constexpr bool DEEP = DEEP2 || (SPX_PRICE_DEEP_SE && SPX_PRICE_PIPE && WM == 4 && BLOCK <= 512 && CH == 8);
    dbl2 vd0[DEEP ? CH : 1], vd1[DEEP2 ? CH : 1];
    int64_t jdeep = -1;  // the column the deep prefetch holds (-1: none)
    // the bookkeeping's inputs for workgroup 0's thread 0, which applies them
    // after its columns (issued first, its stores would hold up the waits for
    // its own staging loads: vmcnt retires in order)
    __shared__ TailRec s_rec;
    __shared__ UpdPartial s_tp;
    if (DT && P.defer_tail) {
        fresh = R.fresh != 0;
        if constexpr (DEEP) {
            // slots below cnt0 hold the same column before and after the
            // list edit, except p's slot R.kp, which takes the last entry.
            // The loads are unconditional buffer loads: behind a branch, the
            // compiler's waits for the partials below covered these loads too
            // (the wait counts of the two paths merge).  Their range is the
            // prefetched chunks when the record is fresh and the slot prices
            // a column, else 0 bytes: out-of-range lanes read 0 and send no
            // request, so a pass after the optimum (the rest of an iterate()
            // call; it prices nothing) no longer streams 16-32 KB per wave
            const int64_t L2d = P.L >> 1;
            const int32_t cnt0 = R.kp >= 0 ? R.cnt - 1 : R.cnt;
            const bool dv = fresh && idx0 < cnt0 && (L2d & 511) == 0 && L2d >= 2 * CH * 64;
            int64_t jd = (R.kp >= 0 && idx0 == R.kp) ? (int64_t)R.last : j0;
            jd = (uint64_t)jd < (uint64_t)P.n ? jd : 0;
            constexpr int NB = (DEEP2 ? 2 : 1) * CH * 64 * (int)sizeof(dbl2);
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<double*>(P.A + jd * P.L), 0, dv ? NB : 0, SPX_BUF_DW3);
#pragma unroll
            for (int u = 0; u < CH; ++u)
                vd0[u] = ldbuf2<SPX_NT_A>(rs, (lane + u * 64) * (int)sizeof(dbl2));
            if constexpr (DEEP2) {
#pragma unroll
                for (int u = 0; u < CH; ++u)
                    vd1[u] = ldbuf2<SPX_NT_A>(rs, (CH * 64 + lane + u * 64) * (int)sizeof(dbl2));
            }
            jdeep = dv ? jd : -1;
        }
        // slots past the FTRAN pass's partials: empty (after the deep loads'
        // issue: the selects wait for the partials)
        if (tid >= P.tail_parts) w0 = upd_empty();
        if constexpr (PAIR) {
            if (tid + BLOCK >= P.tail_parts) w1 = upd_empty();
        }
        if (fresh) {
            __shared__ UpdPartial s_ured[(PAIR ? 2 * WAVES : WAVES) + 1];
            UpdPartial t;
            if constexpr (PAIR) {
                for (int g = tid + 2 * BLOCK; g < P.tail_parts; g += 2 * BLOCK) {
                    upd_merge(w0, upd_fetch<true>(P, g));
                    if (g + BLOCK < P.tail_parts) upd_merge(w1, upd_fetch<true>(P, g + BLOCK));
                }
                t = reduce_partial_pair<BLOCK>(w0, w1, s_ured);
            } else {
                for (int g = tid + BLOCK; g < P.tail_parts; g += BLOCK) upd_merge(w0, upd_fetch<true>(P, g));
                t = reduce_partial_block<BLOCK, true>(w0, s_ured);
            }
            const int64_t q = t.idx;
            const bool unb = t.nonpos == P.m || q < 0 || q >= P.m;
            if (blockIdx.x == 0 && tid == 0) {
                if (unb) apply_deferred_tail(P, st, R, t);
                s_rec.it = R.it;  // (field by field: a struct copy went through scratch)
                s_rec.p = R.p;
                s_rec.e_rep = R.e_rep;
                s_rec.c_p = R.c_p;
                s_rec.wp = R.wp;
                s_rec.cnt = R.cnt;
                s_rec.kp = R.kp;
                s_rec.last = R.last;
                s_rec.nw = R.nw;
                s_tp.idx = t.idx;
                s_tp.nonpos = t.nonpos;
                s_tp.T = t.T;
                s_tp.a_w = t.a_w;
                s_tp.cb_w = t.cb_w;
                s_tp.bix_w = t.bix_w;
            }
            if (unb) return;  // Unbounded (v4:319-322; workgroup 0 has recorded it)
            s_iter = R.it + 1;
            s_q = q;
            s_aq = t.a_w;
            s_sy = y_scalar(t.T, t.a_w, t.cb_w, R.c_p);
            s_nw = R.nw + 1;
            if (P.devex) {
                s_leave = t.bix_w;
                s_wp = R.wp;
            }
            // pivot_bookkeeping's list edit: p's slot takes the last entry,
            // the leaving column joins at the end
            int32_t c1 = R.cnt;
            if (R.kp >= 0) {
                --c1;
                if (R.kp != c1) {
                    pk_b = R.kp;
                    pv_b = R.last;
                }
            }
            if (owns_col(P, t.bix_w)) {
                pk_a = c1;
                pv_a = t.bix_w;
                ++c1;
            }
            s_nb = c1;
            if (idx0 == pk_a) j0 = pv_a;
            else if (idx0 == pk_b) j0 = pv_b;
        }
    }
    const unsigned long long t_pw1 = P.stamps ? rtime() : 0ull;  // the deferred tail is reduced
    auto nbl = [&](int idx) -> int64_t {
        return idx == pk_a ? pv_a : (idx == pk_b ? pv_b : (int64_t)P.nb_list[idx]);
    };
    if (S.status != ST_RUNNING || s_iter >= S.limit) {
        if (fresh && blockIdx.x == 0 && tid == 0) apply_deferred_tail(P, st, s_rec, s_tp);
        return;
    }
    unsigned long long* const slot = P.stamps;
    if (!P.defer_price) stamp_start(slot);  // (deferred passes: per-workgroup clocks only, below)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int64_t L = P.L;
    const int64_t L2 = L >> 1;
    double* ys = reinterpret_cast<double*>(smem);
    double* rs = reinterpret_cast<double*>(smem + (LDS_Y ? L * 8 : 0));
    double* vs = reinterpret_cast<double*>(smem + (LDS_Y ? L * 8 : 0) + (LDS_R ? L * 8 : 0));
    PricePartial* red = reinterpret_cast<PricePartial*>(smem + (LDS_Y ? L * 8 : 0) + (LDS_R ? L * 8 : 0) +
                                                        (LDS_V ? L * 8 : 0));
    int* s_last = reinterpret_cast<int*>(red + WAVES);
    const int nb = s_nb;

    const int64_t it = s_iter;
    const bool wg0 = blockIdx.x == 0;
    constexpr int YB = 4;
    const dbl2* yin = reinterpret_cast<const dbl2*>(S.y_buf ? P.y1 : P.y0);
    // explicit B^-1: current y = ybuf + s_y r while the last pivot's y update is
    // pending (workgroup 0 also persists that y and, in place, stages r for
    // k_update).  Eta window: y_w is fixed between folds; the pending pivot's
    // base row B_w[q,:] is staged next to it (workgroup 0 also keeps it, and
    // U[q][s<tau], in Qrows/Urows for k_fold).  Loads are batched YB deep per
    // thread so the fill is one memory round trip, not one per element.
    const int KW = P.win;
    const int nw = WIN ? s_nw : 0;
    if (WIN && nw >= KW) {  // the host folds before this can happen
        if (wg0 && tid == 0) {
            if (fresh) apply_deferred_tail(P, st, s_rec, s_tp);
            st->status = ST_WINDOW_FULL;
        }
        return;
    }
    if constexpr (CP || DW) {
        // compact pricing never prices from a short AS or a stale dw, and dw
        // is y_w . A_j - c_j only while no earlier pivot of the window rides
        // on the sum (tau <= 0): the host enqueues neither (a state error)
        const bool bad = CP ? (cp_S > P.as_cap || cp_dw != 1) : nw > 1;
        if (bad) {
            if (wg0 && tid == 0) {
                if (fresh) apply_deferred_tail(P, st, s_rec, s_tp);
                st->status = ST_CPRICE_STATE;
            }
            return;
        }
        if constexpr (DW) {
            if (wg0 && tid == 0) P.bc_n[5] = 1;  // (read by the next launch)
        }
    }
    const bool pend = WIN ? nw > 0 : it > 0;
    const int tau = nw - 1;  // pending pivot of the window
    const int64_t qq = pend ? s_q : 0;
    const bool upd_y = !WIN && S.y_applied < it;
    const double s_y = s_sy;
    dbl2* yout = reinterpret_cast<dbl2*>(S.y_buf ? P.y0 : P.y1);
    // the pending pivot row: row q of the stored B^-1 (replicated storage), or
    // rbuf, staged by k_finalize_rs from the all-gather (row-sharded storage)
    const dbl2* rr = reinterpret_cast<const dbl2*>(
        !pend ? P.zeros : (P.row_shard ? P.rbuf : P.B0 + qq * L));
    const bool stage_r = WIN ? (pend && wg0) : (pend && wg0 && !P.row_shard);
    const bool stage = LDS_Y || LDS_R || wg0;
    const dbl2* vin = reinterpret_cast<const dbl2*>(P.se_v);  // steepest edge: B_w^T alpha
    const bool load_y = LDS_Y || (!WIN && wg0);
    const bool need_r = WIN ? (pend && (LDS_R || stage_r)) : (upd_y || stage_r);

    // Issue order (vmcnt retires in issue order): the first batch of y /
    // base-row loads, then the first CH chunks of this wave's first column,
    // which stay in flight across the LDS fill and the barrier.  Every load
    // here is unconditional with a clamped index (rr is always a valid row),
    // so the fill waits for its own loads only, not for the A prefetch.
    static_assert(CH >= 1 && CH <= 8, "the pipelined column loop consumes at most one 8-chunk batch of prefetch");
    const bool deep_hit = DEEP && jdeep >= 0 && jdeep == j0;  // (else the first column goes the usual way)
    const bool pre = WM != 3 && !CP && idx0 < nb && L2 >= CH * 64;
    dbl2 yv[YB], rv[YB], vv[YB];
    double uqrow = 0.0;  // U[q][tid] for Urows (window, workgroup 0)
    if (stage) {
#pragma unroll
        for (int u = 0; u < YB; ++u) {
            const int64_t k = (int64_t)u * BLOCK + tid;
            const int64_t kc = k < L2 ? k : L2 - 1;
            if (load_y) yv[u] = yin[kc];
            rv[u] = rr[kc];
            if constexpr (LDS_V) vv[u] = vin[kc];
        }
        if constexpr (WIN) uqrow = P.U[qq * KW + (tid < KW ? tid : KW - 1)];
    }
    __builtin_amdgcn_sched_barrier(0);  // (the scheduler would hoist the A loads)
    dbl2 v0[CH];
    if constexpr (WM != 3 && !CP) {
        if (!deep_hit) {
            const dbl2* c0 = reinterpret_cast<const dbl2*>(P.A + j0 * L);
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int64_t k = lane + u * 64;
                v0[u] = ld2<SPX_NT_A>(&c0[k < L2 ? k : L2 - 1]);
            }
        }
    }
    if (stage) {
        // the staging values are taken here, behind the A prefetch's issue
        // (otherwise the loads sink into the conditional stores below and
        // their waits cover the prefetch too)
#pragma unroll
        for (int u = 0; u < YB; ++u) {
            if (load_y) asm volatile("" ::"v"(yv[u].x), "v"(yv[u].y));
            asm volatile("" ::"v"(rv[u].x), "v"(rv[u].y));
            if constexpr (LDS_V) asm volatile("" ::"v"(vv[u].x), "v"(vv[u].y));
        }
        if constexpr (WIN) asm volatile("" ::"v"(uqrow));
        dbl2* yl = reinterpret_cast<dbl2*>(ys);
        dbl2* rl = reinterpret_cast<dbl2*>(rs);
        dbl2* vl = reinterpret_cast<dbl2*>(vs);
        dbl2* rb = reinterpret_cast<dbl2*>(WIN ? P.Qrows + (int64_t)tau * L : P.rbuf);
        for (int64_t k0 = 0; k0 < L2; k0 += (int64_t)YB * BLOCK) {
            if (k0 > 0) {  // later batches (L2 > YB * BLOCK)
#pragma unroll
                for (int u = 0; u < YB; ++u) {
                    const int64_t k = k0 + (int64_t)u * BLOCK + tid;
                    const int64_t kc = k < L2 ? k : L2 - 1;
                    if (load_y) yv[u] = yin[kc];
                    if (need_r) rv[u] = rr[kc];
                    if constexpr (LDS_V) vv[u] = vin[kc];
                }
            }
#pragma unroll
            for (int u = 0; u < YB; ++u) {
                const int64_t k = k0 + (int64_t)u * BLOCK + tid;
                if (k < L2) {
                    if constexpr (!WIN) {
                        const dbl2 v = upd_y ? y_apply(s_y, rv[u], yv[u]) : yv[u];
                        if constexpr (LDS_Y) yl[k] = v;
                        if (upd_y && wg0) yout[k] = v;  // flipped in by k_update's tail
                    } else {
                        if constexpr (LDS_Y) yl[k] = yv[u];
                        if constexpr (LDS_R) {
                            if (pend) rl[k] = rv[u];
                        }
                        if constexpr (LDS_V) {
                            if (pend) vl[k] = vv[u];
                        }
                    }
                    if (stage_r) rb[k] = rv[u];
                }
            }
        }
        if (WIN && stage_r && tid < tau) P.Urows[(int64_t)tau * KW + tid] = uqrow;
    }
    // LDS only: the A prefetch stays in flight across the barrier (the staged
    // Qrows / rbuf stores are read after the kernel boundary)
    if constexpr (LDS_Y || LDS_R) lds_barrier();
    auto Y = [&](int64_t k) -> dbl2 {
        if constexpr (LDS_Y) return reinterpret_cast<const dbl2*>(ys)[k];
        else if constexpr (WIN) return yin[k];
        else return upd_y ? y_apply(s_y, rr[k], yin[k]) : yin[k];
    };
    auto Rw = [&](int64_t k) -> dbl2 {
        if constexpr (LDS_R) return reinterpret_cast<const dbl2*>(rs)[k];
        else return rr[k];
    };
    auto Vw = [&](int64_t k) -> dbl2 {
        if constexpr (LDS_V) return reinterpret_cast<const dbl2*>(vs)[k];
        else return vin[k];
    };
    // window coefficients of this lane (lane s < tau: pivot s of the window)
    double uq = 0.0, syl = 0.0, syp = 0.0;
    double csl = 0.0, se_gp = 0.0;  // steepest edge: U[:, s] . alpha (lane s), gamma_p
    if constexpr (WIN) {
        if (pend) {
            if (lane < tau) {
                uq = P.U[qq * KW + lane];
                syl = P.SY[lane];
                if constexpr (SE) csl = P.se_cg[lane];
            }
            syp = fresh ? s_sy : P.SY[tau];  // (fresh: workgroup 0 is writing SY[tau])
            if constexpr (SE) se_gp = P.se_cg[KW];
        }
    }
    double best = INFINITY, bw = 0.0, be = 0.0;
    int64_t bj = INT64_MAX;
    const int64_t dvx_leave = s_leave;
    const double dvx_wp = s_wp, dvx_aq = s_aq;
    unsigned long long* const win = (slot && !P.defer_price) ? P.stamps + 20 : nullptr;
    stamp_stream(win, true);
    const unsigned long long t_pw2 = P.stamps ? rtime() : 0ull;  // the staging is in LDS
    const int nlist = nb;
    const int stride = gridDim.x * WAVES;
    // Dynamic tail (P.price_dyn: WM 2, C5, and WM 1 where a wave prices many
    // columns, C4): the first SPX_PRICE_DYN_PCT % of the list in grid-stride
    // rounds as before, the rest one column per ticket.  P.tk_shards
    // counters (a 128-byte line each, per pass parity): counter k hands out
    // the slots s_lim + k + SHARDS t, and a wave draws from counter
    // (wave + workgroup) mod SHARDS: workgroups b .. b + 7 all reach counter
    // b + 7, so every counter serves waves of all eight XCDs (blockIdx % 8),
    // and every counter has waves when WAVES + grid - 1 >= SHARDS (the host
    // caps the count so; a counter nobody draws from would leave its slots
    // unpriced, which the pass after this one checks on the device: every
    // counter's last value must reach the slots it hands out, else
    // DevState::uncovered is set and the host fails the call).  No address
    // takes more than 1/SHARDS of the
    // fetch-adds (one address: same-address atomics run one after another in
    // their L2 channel, ~8 ns each).  A wave takes each ticket one column
    // ahead -- the first as it starts its last static column, the next as it
    // starts a ticketed one -- so the round trip overlaps a column's stream.
    // Every column's terms and the argmin's total order are unchanged, so the
    // same bits.  Workgroup 0 writes how many tickets of each counter this
    // pass needs (word 1 of its line); at its end it checks the previous
    // pass's counters (the other parity) against theirs and zeroes them for
    // the next pass.
    constexpr bool DYN = WM == 2 || (TK && WM == 1);
    const int TKS = P.tk_shards;  // (1..16, the host's choice per pricing mode)
    int s_lim = nlist;
    uint32_t* tkc = nullptr;
    const int tk_k = (int)((wave + blockIdx.x) % TKS);
    if (DYN && P.price_dyn) {
        s_lim = stride * (int)(((int64_t)nlist * SPX_PRICE_DYN_PCT / 100) / stride);
        if (s_lim < stride) s_lim = stride;
        if (s_lim < nlist) {
            tkc = P.tickets + ((it & 1) * TKS + tk_k) * 32;
            if (wg0 && tid < TKS) {  // counter tid hands out slots s_lim + tid + TKS t < nlist
                const int rem = nlist - s_lim - tid;
                P.tickets[((it & 1) * TKS + tid) * 32 + 1] = rem > 0 ? (uint32_t)((rem + TKS - 1) / TKS) : 0u;
            }
        }
    }
    uint32_t tk_pend = 0;  // the ticket taken ahead (lane 0)
    // candidate update shared by every mode: Devex key, then the argmin
    auto consider = [&](int64_t j, double e, double wn, double dd) {
        double key = e;
        if (WIN && P.devex) {
            // Devex (include/simplex.h SPX_PRICING_DEVEX): the pending pivot's
            // row entry wn = r.A_j updates this column's reference weight.
            // Steepest edge (SPX_PRICING_STEEPEST, oracle se_choose): the
            // Goldfarb-Reid recurrence with dd = A_j . B^-T alpha
            double w = P.W[j];
            if (pend) {
                if constexpr (SE) {
                    if (j == dvx_leave) w = fmax(se_gp / (dvx_aq * dvx_aq), 1.0);
                    else {
                        const double g = wn / dvx_aq;
                        const double t = fma(g * g, se_gp, fma(-2.0 * g, dd, w));
                        w = fmax(t, fma(g, g, 1.0));
                    }
                } else {
                    if (j == dvx_leave) w = fmax(dvx_wp / (dvx_aq * dvx_aq), 1.0);
                    else {
                        const double g = wn / dvx_aq;
                        w = fmax(w, g * g * dvx_wp);
                    }
                }
                if (lane == 0) {
                    // (a group's last pricing workgroup reads the winner's weight back)
                    if (P.nin > 1) st_agent(&P.W[j], w);
                    else P.W[j] = w;
                }
            }
            key = (e < -P.eps) ? -(e * e) / w : INFINITY;
        }
        if (argmin_better(key, j, best, bj)) { best = key; bj = j; bw = wn; be = e; }
    };
    if constexpr (WM == 3) {
        // window tableau (spx_tabdev.h): one lane per non-basic column, the
        // window sums in pivot order inside the lane; a wave takes 64
        // consecutive list slots
        __shared__ double s_sy[64], s_uq[64];
        if (tid < 64) {
            s_sy[tid] = (pend && tid <= tau) ? P.SY[tid] : 0.0;
            s_uq[tid] = (pend && tid < tau) ? P.U[qq * KW + tid] : 0.0;
        }
        __syncthreads();
        for (int base = (blockIdx.x * WAVES + wave) * 64; base < nlist; base += stride * 64) {
            const int idx = base + lane;
            const bool cv = idx < nlist;
            const int64_t j = cv ? (int64_t)P.nb_list[idx] : 0;
            const double tq = (pend && cv) ? P.T[j * L + qq] : 0.0;
            const double dv = cv ? P.dw[j] : 0.0;
            double w, e;
            tab_price_column(tq, dv, cv ? tau : -1, s_sy, s_uq, [&](int s2) { return P.Wt[j * KW + s2]; }, w, e);
            if (!cv) continue;
            if (pend) P.Wt[j * KW + tau] = w;
            double key = e;
            if (P.devex) {  // include/simplex.h SPX_PRICING_DEVEX
                double wt = P.W[j];
                if (pend) {
                    if (j == dvx_leave) wt = fmax(dvx_wp / (dvx_aq * dvx_aq), 1.0);
                    else {
                        const double g = w / dvx_aq;
                        wt = fmax(wt, g * g * dvx_wp);
                    }
                    P.W[j] = wt;
                }
                key = (e < -P.eps) ? -(e * e) / wt : INFINITY;
            }
            if (argmin_better(key, j, best, bj)) { best = key; bj = j; bw = w; be = e; }
        }
        wave_price_min(best, bj, bw, be);
    } else if constexpr (CP) {
        // Compact pricing: one wave per column, as the stream, and the
        // stream's own sum.  The dense pass gives lane l the elements
        // 2 k, 2 k + 1 of B_w[q,:] and A_j with k = l (mod 64), an fma chain
        // per parity in ascending k, then b0 + b1, the window term of lane
        // s < tau, and the butterfly.  Every element off the list (and off q
        // while column q is unit) is an exact zero of B_w[q,:], and fma(a, 0,
        // acc) = acc: so a lane that adds only its listed rows, in ascending
        // row order (as_ord / as_off, k_as_order: the list sorted by lane,
        // then row; row q's unit entry put in at its place), holds the dense
        // lane's b0 and b1 bit for bit, and r_tau . A_j, the Wt entry it
        // becomes, the Devex weights and through FTRAN every later state are
        // those of dense pricing.  No grid, block, dispatch or group count
        // enters that order.  Only e_j is associated anew: dw[j] joins lane
        // 0's window term before the butterfly (it decides the entering
        // column and is reported, nothing else).
        double* cf = reinterpret_cast<double*>(smem + WAVES * sizeof(PricePartial) + 16);
        const int capp = (P.as_cap + 1) & ~1;
        int* cpos = reinterpret_cast<int*>(cf + capp);
        int* crow = cpos + capp;
        __shared__ int c_off[65];
        const int Sn = pend ? cp_S : 0;
        {
            const double* bq = bc_buf(P, cp_sel) + qq * (int64_t)cp_ld;
            for (int i = tid; i < Sn; i += BLOCK) {
                const int c = P.as_ord[i];
                cpos[i] = c;
                crow[i] = P.rlist[c];
                cf[i] = bq[c];
            }
            if (tid < 65) c_off[tid] = pend ? P.as_off[tid] : 0;
        }
        const bool unitq = pend && P.rmap[qq] < 0 && lane == (int)((qq >> 1) & 63);
        __syncthreads();
        // (runs clamped into the entries staged above: offsets that do not
        // belong to this list -- there is none right after a reset -- can
        // neither reach unstaged LDS nor, through it, an address outside AS)
        const int i0 = min(max(c_off[lane], 0), Sn), i1 = min(max(c_off[lane + 1], i0), Sn);
        const int64_t ald = P.as_ld;
        // The lane's first KR terms (the same for every column) in registers,
        // in the order above, the unit entry among them as position -1: a
        // column's loads then go out together, one round trip.  An unused slot
        // reads entry 0 against a zero coefficient, and each term goes to both
        // parities, to the other one with a zero coefficient: fma(a, 0, acc)
        // = acc.  Longer runs take their rest from LDS, term by term.
        constexpr int KR = 8;
        double rc0[KR], rc1[KR];
        int rp[KR];
        int iR = i0;
        bool qrem = unitq;
#pragma unroll
        for (int u = 0; u < KR; ++u) {
            const bool takeq = qrem && (iR >= i1 || crow[iR] > (int)qq);
            double cv = 0.0;
            int par = 0;
            rp[u] = 0;
            if (takeq) {
                rp[u] = -1;
                cv = 1.0;
                par = (int)(qq & 1);
                qrem = false;
            } else if (iR < i1) {
                rp[u] = cpos[iR];
                cv = cf[iR];
                par = crow[iR] & 1;
                ++iR;
            }
            rc0[u] = par ? 0.0 : cv;
            rc1[u] = par ? cv : 0.0;
        }
        if constexpr (CPR) {
            // Row form (spx_cprows.h): a column's listed entries are one contiguous
            // run of AS, so the wave reads it as NC coalesced chunks (lane l takes
            // entries l + 64 t, indices past the list re-read entry 0), stores the
            // chunks to its private LDS slot and every lane takes its terms from
            // there: av[u] = slot[rp[u]], a long run's rest slot[cpos[i]].  The
            // same operands enter the same fma chain in the same order as in the
            // gather form below, so the bits are its bits.  The slot belongs to
            // one wave, whose LDS instructions execute in program order: the store,
            // the reads and the next column's store need no workgroup barrier
            // (wave_barrier keeps the compiler from moving one across another).
            // D columns in flight: once column k's operands have arrived and its
            // row is in the slot, column k + D - 1 is requested into the registers
            // that held it, and column k is summed from the slot while D - 1
            // requests fly.  Every request is unconditional (a column past the
            // wave's last one re-reads the list's last column; a lane without a
            // Wt, dw or unit entry reads one and drops it when the column is
            // summed): the wait for a column then counts the loads issued behind
            // it and leaves them in flight, where a request behind a branch makes
            // that count zero, i.e. a wait for every load.  For the same reason
            // the list entries of the wave's next 64 columns are one load (lane l:
            // the wave's column l) read by lane index, not a load per column whose
            // wait would cover the operands in flight.
            // (A re-read column may be one another wave is pricing, whose Wt entry
            // that wave is storing: the value read is dropped, never summed.  The
            // pipeline drains and refills at every 64th column of a wave: one more
            // round trip per 64 columns.)
            // (DV: Devex.  Its weight load sits in consider; compiled into the
            // Dantzig loop behind a branch, the wait for that load's register at
            // the branch's end is a wait for every operand in flight.)
            // consider's last line, its argmin update, alone: what consider does
            // under Dantzig.  (Calling one such lambda from consider as well
            // changed the code of every dense instantiation, which is to stay
            // instruction for instruction what it was.)
            auto consider_plain = [&](int64_t j, double e, double wn) {
                if (argmin_better(e, j, best, bj)) { best = e; bj = j; bw = wn; be = e; }
            };
            auto run_rows = [&](auto nc_t, auto dv_t) {
                constexpr int NC = decltype(nc_t)::value;
                constexpr bool DV = decltype(dv_t)::value;
                constexpr int D = spx_cprows::depth(NC);
                constexpr int MASK = 64 * NC - 1;
                if (idx0 >= nlist) return;
                double* slot = reinterpret_cast<double*>(crow + capp) + wave * spx_cprows::slot_doubles(P.cp_rows);
                const int lim = min(cp_S, (int)ald);
                // the register terms' places in the slot; the unit entry (position
                // -1) is the slot's entry past the row, where the unit lane puts
                // its A[q, j]
                int pu[KR];
#pragma unroll
                for (int u = 0; u < KR; ++u) pu[u] = rp[u] < 0 ? 64 * NC : (rp[u] & MASK);
                const bool has_w = pend && lane < tau;
                const int wl = has_w ? lane : 0;
                // dw[j] (lane 0 adds it) and A[q, j] (the unit lane's term) share a
                // register: lane 0 loads dw[j], every other lane A[q, j]; a unit
                // lane 0 takes its A[q, j] from lane 1
                constexpr int R = D - 1;  // operand buffers: the columns requested ahead
                double xr[R][NC], xw[R], xo[R];
                int jr[R];
                auto request = [&](int64_t jj, double (&r)[NC], double& w, double& o) {
                    const double* as = P.AS + jj * ald;
                    w = P.Wt[jj * KW + wl];
                    o = *(lane == 0 ? P.dw + jj : P.A + jj * L + qq);
#pragma unroll
                    for (int t = 0; t < NC; ++t) {
                        const int i = lane + 64 * t;
                        r[t] = as[i < lim ? i : 0];
                    }
                };
                const int ilast = nlist - 1;
                auto list64 = [&](int k0) -> int {  // lane l: the list entry of the wave's column k0 + l
                    const int64_t i = (int64_t)idx0 + ((int64_t)k0 + lane) * stride;
                    return (int)nbl(i < nlist ? (int)i : ilast);
                };
                int jl = 0, idx = idx0, k = 0;  // the wave's column k0 + k at list index idx
                auto step = [&](auto d_t) {
                    constexpr int d = decltype(d_t)::value;
                    const int64_t j = jr[d];
                    const double wv = has_w ? xw[d] : 0.0;
                    const double dv = lane == 0 ? xo[d] : 0.0;
                    const double aqj = unitq ? (lane == 0 ? readlane_d(xo[d], 1) : xo[d]) : 0.0;
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int t = 0; t < NC; ++t) slot[lane + 64 * t] = xr[d][t];
                    if (unitq) slot[64 * NC] = aqj;
                    __builtin_amdgcn_wave_barrier();
                    jr[d] = __builtin_amdgcn_readlane(jl, min(k + R, 63));
                    request(jr[d], xr[d], xw[d], xo[d]);
                    double av[KR];
#pragma unroll
                    for (int u = 0; u < KR; ++u) av[u] = slot[pu[u]];
                    double b0 = 0.0, b1 = 0.0;
#pragma unroll
                    for (int u = 0; u < KR; ++u) {
                        b0 = fma(av[u], rc0[u], b0);
                        b1 = fma(av[u], rc1[u], b1);
                    }
                    bool qdone = !qrem;
                    auto unit_term = [&]() {
                        if (qq & 1) b1 = fma(aqj, 1.0, b1);
                        else b0 = fma(aqj, 1.0, b0);
                        qdone = true;
                    };
                    for (int i = iR; i < i1; ++i) {
                        const int r = crow[i];
                        if (!qdone && r > (int)qq) unit_term();
                        const double a = slot[cpos[i] & MASK];
                        if (r & 1) b1 = fma(a, cf[i], b1);
                        else b0 = fma(a, cf[i], b0);
                    }
                    if (!qdone) unit_term();
                    __builtin_amdgcn_wave_barrier();
                    double sa = fma(syl, wv, dv);
                    double wn = fma(uq, wv, b0 + b1);
                    wave_sum2(sa, wn);
                    if (pend && lane == 0) P.Wt[j * KW + tau] = wn;
                    const double e_j = pend ? fma(syp, wn, sa) : sa;
                    if constexpr (DV) consider(j, e_j, wn, 0.0);
                    else consider_plain(j, e_j, wn);
                    idx += stride;
                    ++k;
                };
                // 64 columns of the wave per list load; the pipeline drains at its
                // end (the requests past it re-read its last column)
                int k0 = 0;
                while (idx < nlist) {
                    jl = list64(k0);
                    k0 += 64;
#pragma unroll
                    for (int d = 0; d < R; ++d) {
                        jr[d] = __builtin_amdgcn_readlane(jl, d);
                        request(jr[d], xr[d], xw[d], xo[d]);
                    }
                    // (whole rounds of R columns in a loop without a branch, the
                    // rest behind it: a step behind a condition inside the loop
                    // has the compiler copy the operands in flight where the paths
                    // join, which waits for them)
                    const int64_t left = ((int64_t)nlist - idx + stride - 1) / stride;
                    const int ng = (int)(left < 64 ? left : 64);
                    k = 0;
                    while (k + R <= ng) {
                        step(std::integral_constant<int, 0>());
                        if constexpr (R == 3) {
                            step(std::integral_constant<int, 1>());
                            step(std::integral_constant<int, 2>());
                        } else {
                            static_assert(R == 1, "one or three columns requested ahead");
                        }
                    }
                    if constexpr (R == 3) {
                        const int rem = ng - k;
                        if (rem >= 1) step(std::integral_constant<int, 0>());
                        if (rem >= 2) step(std::integral_constant<int, 1>());
                    }
                }
            };
            const int cp_nc = spx_cprows::chunks(cp_S, P.cp_rows);
            const bool cp_dv = P.devex != 0;
            if (cp_nc == 2 && !cp_dv) run_rows(std::integral_constant<int, 2>(), std::false_type());
            else if (cp_nc == 4 && !cp_dv) run_rows(std::integral_constant<int, 4>(), std::false_type());
            else if (cp_nc == 8 && !cp_dv) run_rows(std::integral_constant<int, 8>(), std::false_type());
            else if (cp_nc == 2) run_rows(std::integral_constant<int, 2>(), std::true_type());
            else if (cp_nc == 4) run_rows(std::integral_constant<int, 4>(), std::true_type());
            else if (cp_nc == 8) run_rows(std::integral_constant<int, 8>(), std::true_type());
            // (a jump, not a condition around the gather form: WM 6 then compiles
            // to the code it had)
            if (cp_nc != 0) goto cp_priced;
        }
        {
            // Two columns in flight: a column's operands are requested while the
            // one before it is summed, and its list entry a column earlier still
            // (indices clamped into the list: every load is unconditional)
            double av[KR], wv = 0.0, dv = 0.0, aqj = 0.0;
            auto request = [&](int64_t jj, double (&xa)[KR], double& xw, double& xd, double& xq) {
                const double* as = P.AS + jj * ald;
                const double* aq = P.A + jj * L + qq;
                xw = (pend && lane < tau) ? P.Wt[jj * KW + lane] : 0.0;
                xd = lane == 0 ? P.dw[jj] : 0.0;
#pragma unroll
                for (int u = 0; u < KR; ++u) xa[u] = *(rp[u] < 0 ? aq : as + rp[u]);
                xq = qrem ? *aq : 0.0;
            };
            const int ilast = nlist > 0 ? nlist - 1 : 0;
            int64_t jn = nbl(idx0 + stride < nlist ? idx0 + stride : ilast);
            if (idx0 < nlist) request(j0, av, wv, dv, aqj);
            int64_t jc = j0;
            for (int idx = idx0; idx < nlist; idx += stride) {
                const int64_t j = jc;
                const double* as = P.AS + j * ald;
                const int64_t jn2 = nbl(idx + 2 * stride < nlist ? idx + 2 * stride : ilast);
                double avn[KR], wvn = 0.0, dvn = 0.0, aqn = 0.0;
                const bool more = idx + stride < nlist;
                if (more) request(jn, avn, wvn, dvn, aqn);
                double b0 = 0.0, b1 = 0.0;
#pragma unroll
                for (int u = 0; u < KR; ++u) {
                    b0 = fma(av[u], rc0[u], b0);
                    b1 = fma(av[u], rc1[u], b1);
                }
                bool qdone = !qrem;
                auto unit_term = [&]() {
                    if (qq & 1) b1 = fma(aqj, 1.0, b1);
                    else b0 = fma(aqj, 1.0, b0);
                    qdone = true;
                };
                for (int i = iR; i < i1; ++i) {
                    const int r = crow[i];
                    if (!qdone && r > (int)qq) unit_term();
                    const double a = as[cpos[i]];
                    if (r & 1) b1 = fma(a, cf[i], b1);
                    else b0 = fma(a, cf[i], b0);
                }
                if (!qdone) unit_term();
                double sa = fma(syl, wv, dv);
                double wn = fma(uq, wv, b0 + b1);
                wave_sum2(sa, wn);
                if (pend && lane == 0) P.Wt[j * KW + tau] = wn;
                const double e = pend ? fma(syp, wn, sa) : sa;
                consider(j, e, wn, 0.0);
                if (more) {
#pragma unroll
                    for (int u = 0; u < KR; ++u) av[u] = avn[u];
                    wv = wvn;
                    dv = dvn;
                    aqj = aqn;
                }
                jc = jn;
                jn = jn2;
            }
        }
        [[maybe_unused]] cp_priced:;
    } else {
    // The first CH chunks of every column are loaded before the previous
    // column's reduction (and, for the first column, before the LDS fill), so
    // a wave's A stream does not stall at column boundaries.
    // slack columns (A[:, ns:] = I, P.slack_unit): the unit vector's dot
    // products without its stream (see below)
    auto unit_col = [&](int64_t jj) { return P.slack_unit && jj >= P.ns; };
    bool have = pre && !unit_col(j0);
    int idx_next = 0;
    for (int idx = idx0; idx < nlist; idx = idx_next) {
        const bool first = idx == idx0;
        if constexpr (DYN) {
            if (tkc && idx < s_lim && idx + stride >= s_lim) {  // the last static column: the first ticket
                uint32_t t = 0;
                if (lane == 0) t = __hip_atomic_fetch_add(tkc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                tk_pend = t;
            }
        }
        const int64_t j = first ? j0 : nbl(idx);
        const dbl2* __restrict__ col = reinterpret_cast<const dbl2*>(P.A + j * L);
        double wv = 0.0;
        if (WIN && pend && lane < tau) wv = P.Wt[j * KW + lane];
        double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0, d0 = 0.0, d1 = 0.0;
        int64_t k = lane;
        const bool unit = unit_col(j);
        // Two 8-chunk batches in flight through the column: the batch after
        // the prefetched first one is requested before that one is consumed,
        // and every later batch before its predecessor is (kb: the batch
        // base, uniform).  The fma order is the loop's below (the same bits).
        const bool pipe = SPX_PRICE_PIPE && BLOCK <= 512 && have && (L2 & 511) == 0 && L2 > CH * 64;
        auto run_pipe = [&](auto pend_t) {
            constexpr bool PD = decltype(pend_t)::value;
            auto consume = [&](const dbl2* vv, int nb8, int64_t kb) {
#pragma unroll
                for (int h = 0; h < 8; h += LB) {
                    if (h >= nb8) break;
                    dbl2 w[LB], r[LB], x[LB];
#pragma unroll
                    for (int u = 0; u < LB; ++u) {
                        w[u] = Y(kb + lane + (h + u) * 64);
                        if constexpr (PD) r[u] = Rw(kb + lane + (h + u) * 64);
                        if constexpr (PD && SE) x[u] = Vw(kb + lane + (h + u) * 64);
                    }
#pragma unroll
                    for (int u = 0; u < LB; ++u) {
                        a0 = fma(vv[h + u].x, w[u].x, a0);
                        a1 = fma(vv[h + u].y, w[u].y, a1);
                        if constexpr (PD) {
                            b0 = fma(vv[h + u].x, r[u].x, b0);
                            b1 = fma(vv[h + u].y, r[u].y, b1);
                        }
                        if constexpr (PD && SE) {
                            d0 = fma(vv[h + u].x, x[u].x, d0);
                            d1 = fma(vv[h + u].y, x[u].y, d1);
                        }
                    }
                }
            };
            int64_t kb = CH * 64;
            dbl2 vc[8];
            if (DEEP2 && first && deep_hit) {
                // the two deep-prefetched batches, the third requested first
                kb = 2 * CH * 64;
                if (kb < L2) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) vc[u] = ld2<SPX_NT_A>(&col[kb + lane + u * 64]);
                }
                consume(vd0, CH, 0);
                consume(vd1, CH, CH * 64);
                if (kb >= L2) {
                    k = L2;
                    return;
                }
            } else if (DEEP && first && deep_hit) {
                // (WM 4) the one deep-prefetched batch in place of v0
#pragma unroll
                for (int u = 0; u < 8; ++u) vc[u] = ld2<SPX_NT_A>(&col[kb + lane + u * 64]);
                consume(vd0, CH, 0);
            } else {
#pragma unroll
                for (int u = 0; u < 8; ++u) vc[u] = ld2<SPX_NT_A>(&col[kb + lane + u * 64]);
                consume(v0, CH, 0);
            }
            for (; kb + 8 * 64 < L2; kb += 8 * 64) {
                dbl2 vn[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) vn[u] = ld2<SPX_NT_A>(&col[kb + 8 * 64 + lane + u * 64]);
                consume(vc, 8, kb);
#pragma unroll
                for (int u = 0; u < 8; ++u) vc[u] = vn[u];
            }
            consume(vc, 8, kb);
            k = L2;
        };
        if (unit) {
            // column ns + i is e_i: every lane partial of the dense sum stays
            // +0 except the one holding element i, which is fma(1, y_i, +0)
            // (fma with the exact zeros of the other rows adds +-0), so
            // these are the dense loop's bits without its 8L-byte stream
            const int64_t i = j - P.ns, k2 = i >> 1;
            if (lane == (int)(k2 & 63)) {
                const dbl2 w = Y(k2);
                const double v = fma(1.0, (i & 1) ? w.y : w.x, 0.0);
                if (i & 1) a1 = v;
                else a0 = v;
                if (WIN && pend) {
                    const dbl2 r = Rw(k2);
                    const double u = fma(1.0, (i & 1) ? r.y : r.x, 0.0);
                    if (i & 1) b1 = u;
                    else b0 = u;
                    if constexpr (SE) {
                        const dbl2 x = Vw(k2);
                        const double t = fma(1.0, (i & 1) ? x.y : x.x, 0.0);
                        if (i & 1) d1 = t;
                        else d0 = t;
                    }
                }
            }
        } else if (pipe && WIN && pend) {
            run_pipe(std::true_type());
        } else if (pipe) {
            run_pipe(std::false_type());
        } else {
        if (have) {  // consume the prefetched chunks (same k order as the loop)
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const dbl2 w = Y(lane + u * 64);
                a0 = fma(v0[u].x, w.x, a0);
                a1 = fma(v0[u].y, w.y, a1);
                if (WIN && pend) {
                    const dbl2 r = Rw(lane + u * 64);
                    b0 = fma(v0[u].x, r.x, b0);
                    b1 = fma(v0[u].y, r.y, b1);
                    if constexpr (SE) {
                        const dbl2 x = Vw(lane + u * 64);
                        d0 = fma(v0[u].x, x.x, d0);
                        d1 = fma(v0[u].y, x.y, d1);
                    }
                }
            }
            k += CH * 64;
        }
        if (!WIN || !pend) {
            for (; k + 7 * 64 < L2; k += 8 * 64) {
                dbl2 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = ld2<SPX_NT_A>(&col[k + u * 64]);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const dbl2 w = Y(k + u * 64);
                    a0 = fma(v[u].x, w.x, a0);
                    a1 = fma(v[u].y, w.y, a1);
                }
            }
            for (; k < L2; k += 64) {
                const dbl2 v = ld2<SPX_NT_A>(&col[k]);
                const dbl2 w = Y(k);
                a0 = fma(v.x, w.x, a0);
                a1 = fma(v.y, w.y, a1);
            }
        } else {
            for (; k + 7 * 64 < L2; k += 8 * 64) {
                dbl2 v[8], w[8], r[8], x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = ld2<SPX_NT_A>(&col[k + u * 64]);
                // LDS operands fetched LB elements at a time (one
                // LDS latency per batch, not one per element)
#pragma unroll
                for (int h = 0; h < 8; h += LB) {
#pragma unroll
                    for (int u = h; u < h + LB; ++u) {
                        w[u] = Y(k + u * 64);
                        r[u] = Rw(k + u * 64);
                        if constexpr (SE) x[u] = Vw(k + u * 64);
                    }
#pragma unroll
                    for (int u = h; u < h + LB; ++u) {
                        a0 = fma(v[u].x, w[u].x, a0);
                        a1 = fma(v[u].y, w[u].y, a1);
                        b0 = fma(v[u].x, r[u].x, b0);
                        b1 = fma(v[u].y, r[u].y, b1);
                        if constexpr (SE) {
                            d0 = fma(v[u].x, x[u].x, d0);
                            d1 = fma(v[u].y, x[u].y, d1);
                        }
                    }
                }
            }
            for (; k < L2; k += 64) {
                const dbl2 v = ld2<SPX_NT_A>(&col[k]);
                const dbl2 w = Y(k);
                const dbl2 r = Rw(k);
                a0 = fma(v.x, w.x, a0);
                a1 = fma(v.y, w.y, a1);
                b0 = fma(v.x, r.x, b0);
                b1 = fma(v.y, r.y, b1);
                if constexpr (SE) {
                    const dbl2 x = Vw(k);
                    d0 = fma(v.x, x.x, d0);
                    d1 = fma(v.y, x.y, d1);
                }
            }
        }
        }
        // next column's first chunks in flight during this column's reduction
        int nidx = idx + stride;
        if constexpr (DYN) {
            if (tkc && nidx >= s_lim) {  // (wave-uniform) the next column comes by the ticket taken ahead
                nidx = s_lim + tk_k + TKS * (int)__builtin_amdgcn_readfirstlane(tk_pend);
                if (nidx < nlist) {
                    uint32_t t = 0;
                    if (lane == 0) t = __hip_atomic_fetch_add(tkc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    tk_pend = t;
                }
            }
        }
        idx_next = nidx;
        const int64_t jn = nidx < nlist ? nbl(nidx) : 0;
        have = nidx < nlist && L2 >= CH * 64 && !unit_col(jn);
        if (have) {
            const dbl2* cn = reinterpret_cast<const dbl2*>(P.A + jn * L);
#pragma unroll
            for (int u = 0; u < CH; ++u) v0[u] = ld2<SPX_NT_A>(&cn[lane + u * 64]);
        }
        double e, wn = 0.0, dd = 0.0;
        if (WIN && pend) {
            // r_tau . A_j = B_w[q,:] . A_j + sum_s U[q][s] Wt[j][s]; the window
            // terms join the lane partials before the butterflies
            double sa = fma(syl, wv, a0 + a1);
            wn = fma(uq, wv, b0 + b1);
            if constexpr (SE) {
                // A_j . B^-T alpha = v . A_j + sum_{s<tau} (U[:, s] . alpha) Wt[j][s]
                dd = fma(csl, wv, d0 + d1);
                wave_sum3(sa, wn, dd);
            } else {
                wave_sum2(sa, wn);
            }
            if (lane == 0) P.Wt[j * KW + tau] = wn;
            e = fma(syp, wn, sa) - P.c[j];
            if constexpr (DW) {  // tau = 0: sa is y_w . A_j, the stream's own bits
                if (lane == 0) P.dw[j] = sa - P.c[j];
            }
        } else {
            e = wave_sum(a0 + a1) - P.c[j];
            if constexpr (DW) {
                if (lane == 0) P.dw[j] = e;
            }
        }
        consider(j, e, wn, dd);
    }
    }

    stamp_stream(win, false);
    // workgroup argmin over waves (lane 0 of each wave holds the wave's best)
    if (lane == 0) red[wave] = PricePartial{best, bj, bw, be};
    __syncthreads();
    if constexpr (DYN || CP) {  // (compact passes hand out no tickets, but keep the counters' turn)
        // the previous pass's tickets (final: it ended at the kernel
        // boundary): every wave draws from its counter until it gets a slot
        // past the list, so a counter with waves ends above the slots it
        // hands out; one below them had slots nobody priced (a wrong entering
        // column, or a wrong optimum): stop loudly.  Then zero them.
        if (P.price_dyn && wg0 && tid < TKS) {
            uint32_t* o = P.tickets + (((it + 1) & 1) * TKS + tid) * 32;
            if (o[1] > o[0]) st->uncovered = 1u;
            o[0] = 0u;
            o[1] = 0u;
        }
    }
    if (P.stamps && tid == 0 && blockIdx.x < 4096) {  // diagnostics: this workgroup's start and end
        unsigned long long* pw = P.stamps + STAMP_PRICE + (it & 1) * 4 * 4096 + 4 * (int64_t)blockIdx.x;
        pw[0] = t_pw0;
        pw[1] = rtime();
        pw[2] = t_pw1;
        pw[3] = t_pw2;
    }
    if (P.defer_price) {  // k_update reduces the partials after the kernel boundary
        if (tid == 0) {
            P.price_partials[blockIdx.x] = red[best_wave<WAVES>(red)];
            if (fresh && blockIdx.x == 0) {
                apply_deferred_tail(P, st, s_rec, s_tp);
                if (P.stamps) P.stamps[STAMP_TAIL + 4 + (it & 1)] = rtime();  // the bookkeeping is issued
            }
        }
        return;
    }
    // multi-rank passes (the pricing tail in this launch, for the exchange):
    // workgroup 0 applies a deferred tail before it arrives; the fan-in below
    // reads no state word the bookkeeping writes
    if (fresh && blockIdx.x == 0 && tid == 0) apply_deferred_tail(P, st, s_rec, s_tp);
    if (P.price_tag) {
        // Tagged hand-off (as k_update's, upd_publish_tagged): wave 0
        // publishes the workgroup's partial as PRICE_WORDS {32-bit half, tag}
        // words with one sc1 store instruction, and the last workgroup polls
        // every slot until its words carry this pass's tag -- no drain and no
        // last-arrival count.  The winner's new Wt entry travels in the
        // partial; its earlier window entries were written by earlier kernels.
        const uint32_t tag = (uint32_t)(it + 1);
        if (wave == 0) {
            const PricePartial w = red[best_wave<WAVES>(red)];
            if (lane < PRICE_WORDS) {
                const int f = lane >> 1;
                const uint64_t u = f == 0 ? (uint64_t)__double_as_longlong(w.val)
                                 : f == 1 ? (uint64_t)w.idx
                                 : f == 2 ? (uint64_t)__double_as_longlong(w.w)
                                          : (uint64_t)__double_as_longlong(w.pad);
                const uint32_t half = (lane & 1) ? (uint32_t)(u >> 32) : (uint32_t)u;
                st_agent(&P.price_tag[(int64_t)lane * P.price_cap + blockIdx.x], ((uint64_t)tag << 32) | half);
            }
        }
        if (blockIdx.x != gridDim.x - 1) return;
        const unsigned long long t_tail = slot ? rtime() : 0;
        __shared__ bool s_to;
        if (tid == 0) s_to = false;
        lds_barrier();
        PricePartial w{INFINITY, INT64_MAX, 0.0, 0.0};
        for (int g = tid; g < (int)gridDim.x; g += BLOCK) {
            uint64_t wd[PRICE_WORDS];
            bool ok = false;
            for (uint32_t spins = 0; spins <= (1u << 20); ++spins) {
#pragma unroll
                for (int k = 0; k < PRICE_WORDS; ++k) wd[k] = ld_agent(&P.price_tag[(int64_t)k * P.price_cap + g]);
                ok = true;
#pragma unroll
                for (int k = 0; k < PRICE_WORDS; ++k) ok = ok && (uint32_t)(wd[k] >> 32) == tag;
                if (ok) break;
                __builtin_amdgcn_s_sleep(1);
            }
            if (!ok) {
                s_to = true;  // (a benign race: every writer stores true)
                break;
            }
            uint64_t f[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = (wd[2 * k] & 0xffffffffull) | (wd[2 * k + 1] << 32);
            const PricePartial v{__longlong_as_double((long long)f[0]), (int64_t)f[1],
                                 __longlong_as_double((long long)f[2]), __longlong_as_double((long long)f[3])};
            if (argmin_better(v.val, v.idx, w.val, w.idx)) w = v;
#pragma unroll
            for (int k = 0; k < PRICE_WORDS; ++k) P.price_tag[(int64_t)k * P.price_cap + g] = 0ull;
        }
        // wave DPP argmin; the winner's payload from its lane
        double bv = w.val;
        int64_t bj = w.idx;
        lane_argmin<64>(bv, bj);
        bv = readlane_d(bv, 63);
        bj = readlane_l(bj, 63);
        const uint64_t hit = __ballot(w.val == bv && w.idx == bj);
        const int wl = hit ? (int)__builtin_ctzll(hit) : 0;
        const PricePartial o{bv, bj, readlane_d(w.w, wl), readlane_d(w.pad, wl)};
        if (lane == 0) red[wave] = o;
        lds_barrier();
        PricePartial t = red[0];
        for (int i = 1; i < WAVES; ++i)
            if (argmin_better(red[i].val, red[i].idx, t.val, t.idx)) t = red[i];
        if (s_to) {  // a partial never arrived (a fault elsewhere): stop loudly
            if (tid == 0) st->status = ST_HANDOFF_TIMEOUT;
            return;
        }
        if (tid == 0) {
            P.price_out[0] = ArgMinEntry{t.val, t.idx};
            if (WIN && P.devex) *P.dvx_e = t.pad;
            if (WIN && P.devex && P.nin > 1) {  // the reduced cost and weight travel with the record
                double* ex = reinterpret_cast<double*>(P.price_out + 1 + KW / 2);
                ex[0] = t.pad;
                ex[1] = t.idx == INT64_MAX ? 1.0 : ld_agent(&P.W[t.idx]);
            }
        }
        if (WIN && P.nin > 1) {
            double* wo = reinterpret_cast<double*>(P.price_out + 1);
            if (tid < KW)
                wo[tid] = (t.idx == INT64_MAX || tid >= nw) ? 0.0 : (tid == tau ? t.w : P.Wt[t.idx * KW + tid]);
        }
        if (WIN && P.mbox_fused) {
            // fused exchange: the record (the same words k_exchange would
            // send: the entry, the winner's window coefficients, Devex's
            // reduced cost and weight) stored into every rank's mailbox
            // straight from here, one 32-bit half per thread and word
            const int nh = P.pr_stride * 4;
            const int G = P.nin;
            const uint32_t tag = mbox_tag(S.mbox_epoch, it);
            const int64_t par = it & 1;
            for (int h = tid; h < nh; h += BLOCK) {
                const int f = h >> 1;  // the record's 8-byte field
                uint64_t u;
                if (f == 0) u = (uint64_t)__double_as_longlong(t.val);
                else if (f == 1) u = (uint64_t)t.idx;
                else if (f < 2 + KW) {
                    const int d = f - 2;
                    const double v = (t.idx == INT64_MAX || d >= nw) ? 0.0 : (d == tau ? t.w : P.Wt[t.idx * KW + d]);
                    u = (uint64_t)__double_as_longlong(v);
                } else {
                    const double v = f == 2 + KW ? t.pad : (t.idx == INT64_MAX ? 1.0 : ld_agent(&P.W[t.idx]));
                    u = (uint64_t)__double_as_longlong(v);
                }
                const uint64_t w = ((uint64_t)tag << 32) | ((h & 1) ? (uint32_t)(u >> 32) : (uint32_t)u);
                for (int g = 0; g < G; ++g)
                    __hip_atomic_store(&P.mbox_peer[g][(par * G + P.mbox_rank) * nh + h], w, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        stamp_tail(slot, t_tail, win);
        return;
    }
    if (tid == 0) {
        PricePartial w = red[0];
        for (int i = 1; i < WAVES; ++i)
            if (argmin_better(red[i].val, red[i].idx, w.val, w.idx)) w = red[i];
        st_agent(&P.price_partials[blockIdx.x].val, w.val);
        st_agent(&P.price_partials[blockIdx.x].idx, w.idx);
        if constexpr (WIN) {
            st_agent(&P.price_partials[blockIdx.x].w, w.w);
            st_agent(&P.price_partials[blockIdx.x].pad, w.pad);
        }
        drain_vmem();
        *s_last = arrive_last(arrive_group(P.arrive, ARR_PRICE), gridDim.x, blockIdx.x);
    }
    __syncthreads();
    if (!*s_last) return;
    const unsigned long long t_tail = slot ? rtime() : 0;

    // last workgroup: reduce all partials
    PricePartial w{INFINITY, INT64_MAX, 0.0, 0.0};
    for (int g = tid; g < (int)gridDim.x; g += BLOCK) {
        const double v = ld_agent(&P.price_partials[g].val);
        const int64_t i = ld_agent(&P.price_partials[g].idx);
        if (argmin_better(v, i, w.val, w.idx))
            w = PricePartial{v, i, WIN ? ld_agent(&P.price_partials[g].w) : 0.0,
                             WIN ? ld_agent(&P.price_partials[g].pad) : 0.0};
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double v = __shfl_xor(w.val, off, 64);
        const int64_t i = __shfl_xor(w.idx, off, 64);
        const double ww = __shfl_xor(w.w, off, 64);
        const double we = __shfl_xor(w.pad, off, 64);
        if (argmin_better(v, i, w.val, w.idx)) w = PricePartial{v, i, ww, we};
    }
    __syncthreads();
    if (lane == 0) red[wave] = w;
    __syncthreads();
    PricePartial t = red[0];
    for (int i = 1; i < WAVES; ++i)
        if (argmin_better(red[i].val, red[i].idx, t.val, t.idx)) t = red[i];
    if (tid == 0) {
        P.price_out[0] = ArgMinEntry{t.val, t.idx};
        if (WIN && P.devex) *P.dvx_e = t.pad;
        if (WIN && P.devex && P.nin > 1) {  // the reduced cost and weight travel with the record
            double* ex = reinterpret_cast<double*>(P.price_out + 1 + KW / 2);
            ex[0] = t.pad;
            ex[1] = t.idx == INT64_MAX ? 1.0 : ld_agent(&P.W[t.idx]);
        }
    }
    if (WIN && P.nin > 1) {
        // the winner's window coefficients Wt[p][0..nw) travel with it (the
        // column may live on another rank's shard; one rank reads Wt directly)
        double* wo = reinterpret_cast<double*>(P.price_out + 1);
        if (tid < KW)
            wo[tid] = (t.idx == INT64_MAX || tid >= nw) ? 0.0 : (tid == tau ? t.w : P.Wt[t.idx * KW + tid]);
    }
    stamp_tail(slot, t_tail, win);
}

// ---------------------------------------------------------------------------
// Host-side launchers
// ---------------------------------------------------------------------------
template <int BLOCK, bool LDS_Y, int WM, bool TK = false, bool DW = false>
static hipError_t launch_price_t(const Params& P, int grid, size_t lds, hipStream_t s, hipEvent_t e0,
                                 hipEvent_t e1) {
    if (e0 || e1) {
        hipExtLaunchKernelGGL((k_price<BLOCK, LDS_Y, WM, TK, DW>), dim3(grid), dim3(BLOCK), (uint32_t)lds, s, e0, e1, 0, P);
    } else {
        hipLaunchKernelGGL((k_price<BLOCK, LDS_Y, WM, TK, DW>), dim3(grid), dim3(BLOCK), lds, s, P);
    }
    return hipGetLastError();
}

template <int BLOCK, bool LDS_Y, int WM, bool TK = false, bool DW = false>
static hipError_t prep_price_t(size_t lds, int* blocks_per_cu) {
    hipError_t e = hipSuccess;
    if (lds > 65536) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_price<BLOCK, LDS_Y, WM, TK, DW>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_price<BLOCK, LDS_Y, WM, TK, DW>, BLOCK, lds);
}

// (lds_y, wm) variants: (1,0) (0,0) explicit B^-1; (1,1) (1,2) (0,2) eta window
template <int BLOCK>
static hipError_t price_dispatch(const PriceCfg& c, const Params* P, hipStream_t s, hipEvent_t e0, hipEvent_t e1,
                                 int* blocks_per_cu) {
#define SPX_PV(LY, WM)                                                                  \
    return P ? launch_price_t<BLOCK, LY, WM>(*P, c.grid, c.lds_bytes, s, e0, e1)        \
             : prep_price_t<BLOCK, LY, WM>(c.lds_bytes, blocks_per_cu)
#define SPX_PVD(LY, WM, TK)                                                                    \
    return P ? launch_price_t<BLOCK, LY, WM, TK, true>(*P, c.grid, c.lds_bytes, s, e0, e1)     \
             : prep_price_t<BLOCK, LY, WM, TK, true>(c.lds_bytes, blocks_per_cu)
    if (c.dw) {  // the dense pass that opens a compact-priced window
        if (c.wm == 1 && c.lds_y) {
            if (c.tk) SPX_PVD(true, 1, true);
            SPX_PVD(true, 1, false);
        }
        if (c.wm == 2) {
            if (c.lds_y) SPX_PVD(true, 2, false);
            SPX_PVD(false, 2, false);
        }
        return hipErrorInvalidValue;
    }
    if (c.wm == 6) SPX_PV(false, 6);
    if (c.wm == 7) SPX_PV(false, 7);
    if (c.wm == 0) {
        if (c.lds_y) SPX_PV(true, 0);
        SPX_PV(false, 0);
    }
    if (c.wm == 1 && c.lds_y) {
        if (c.tk) return P ? launch_price_t<BLOCK, true, 1, true>(*P, c.grid, c.lds_bytes, s, e0, e1)
                           : prep_price_t<BLOCK, true, 1, true>(c.lds_bytes, blocks_per_cu);
        SPX_PV(true, 1);
    }
    if (c.wm == 2) {
        if (c.lds_y) SPX_PV(true, 2);
        SPX_PV(false, 2);
    }
    if (c.wm == 3) SPX_PV(false, 3);
    if (c.wm == 4 && c.lds_y) SPX_PV(true, 4);
    if (c.wm == 5) {
        if (c.lds_y) SPX_PV(true, 5);
        SPX_PV(false, 5);
    }
#undef SPX_PV
#undef SPX_PVD
    return hipErrorInvalidValue;
}

// dw for the basic columns (one may leave inside the window and is then
// priced from dw): after the dense pass that stored the non-basic ones, whose
// workgroup 0 has applied the pending pivot's bookkeeping, so b_ixs is the
// basis that pass priced for.  One wave per row; k_reduced_costs' dot (the
// lane partials and butterfly of the pricing stream), a unit column's single
// term without its stream
__global__ __launch_bounds__(256) void k_dw_basic(Params P) {
    const int lane = threadIdx.x & 63;
    const int64_t L2 = P.L >> 1;
    const double* y = P.st->y_buf ? P.y1 : P.y0;
    const dbl2* y2 = reinterpret_cast<const dbl2*>(y);
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < P.m;
         i += ((int64_t)gridDim.x * blockDim.x) >> 6) {
        const int64_t j = P.b_ixs[i];
        if ((uint64_t)j >= (uint64_t)P.n) continue;
        double s;
        if (P.slack_unit && j >= P.ns) {
            s = y[j - P.ns] - P.c[j];
        } else {
            const dbl2* col = reinterpret_cast<const dbl2*>(P.A + j * P.L);
            double a0 = 0.0, a1 = 0.0;
            for (int64_t k = lane; k < L2; k += 64) {
                const dbl2 v = col[k], w = y2[k];
                a0 = fma(v.x, w.x, a0);
                a1 = fma(v.y, w.y, a1);
            }
            s = wave_sum(a0 + a1) - P.c[j];
        }
        if (lane == 0) P.dw[j] = s;
    }
}

hipError_t launch_dw_basic(const Params& P, hipStream_t s) {
    const int64_t want = (P.m + 3) / 4;
    hipLaunchKernelGGL(k_dw_basic, dim3((unsigned)(want < 1024 ? want : 1024)), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t price_prepare(const PriceCfg& c, int* blocks_per_cu) {
    switch (c.block) {
        case 256: return price_dispatch<256>(c, nullptr, nullptr, nullptr, nullptr, blocks_per_cu);
        case 512: return price_dispatch<512>(c, nullptr, nullptr, nullptr, nullptr, blocks_per_cu);
        case 1024: return price_dispatch<1024>(c, nullptr, nullptr, nullptr, nullptr, blocks_per_cu);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_price(const Params& P, const PriceCfg& c, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    switch (c.block) {
        case 256: return price_dispatch<256>(c, &P, s, e0, e1, nullptr);
        case 512: return price_dispatch<512>(c, &P, s, e0, e1, nullptr);
        case 1024: return price_dispatch<1024>(c, &P, s, e0, e1, nullptr);
    }
    return hipErrorInvalidValue;
}

}  // namespace spx
