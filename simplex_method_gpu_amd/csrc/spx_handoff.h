// spx_handoff.h — device helpers of the hand-off between the two big kernels
// of a loop pass (internal to the kernel units; the host sees spx_kernels.h).
//
// k_price (spx_price.hip) and the FTRAN kernels (spx_update.hip) pass each
// other work: the FTRAN pass publishes its workgroups' ratio-test partials and
// either reduces them in its last workgroup (update_tail) or leaves them with
// a TailRec for the next pricing pass (apply_deferred_tail); on a column-shard
// group the pricing tail sends its record to the peers' mailboxes and the
// FTRAN entry polls for theirs.  Both sides of each protocol are defined here
// once, in definition order, so every consumer produces the same bits:
//   phase stamps (diagnostic) | peer mailboxes | partials: publish, fetch,
//   reduce | k_update's LDS carve-up | the pivot tail family
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "spx_device.h"
#include "spx_common.h"

namespace spx {

// Diagnostic phase stamps: slot[0] = earliest workgroup start of the current
// launch, slot[1] += (last-workgroup ticket - start), slot[2] += tail duration.
__device__ __forceinline__ void stamp_start(unsigned long long* slot) {
    if (slot && threadIdx.x == 0) atomicMin(&slot[0], rtime());
}
// Stream window per launch: slot[S+0] = earliest wave stream start, slot[S+1]
// = latest wave stream end; the tail adds prologue (earliest stream start -
// earliest workgroup start) to slot[S+2] and drain (last ticket - latest
// stream end) to slot[S+3].
__device__ __forceinline__ void stamp_stream(unsigned long long* s, bool begin) {
    if (s && threadIdx.x == 0) {  // one atomic per workgroup (wave 0 as its proxy)
        if (begin) atomicMin(&s[0], rtime());
        else atomicMax(&s[1], rtime());
    }
}
__device__ __forceinline__ void stamp_tail(unsigned long long* slot, unsigned long long t_tail,
                                           unsigned long long* win) {
    if (slot && threadIdx.x == 0) {
        const unsigned long long t_end = rtime();
        const unsigned long long t0 = __hip_atomic_load(&slot[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd(&slot[1], t_tail - t0);
        atomicAdd(&slot[2], t_end - t_tail);
        __hip_atomic_store(&slot[0], ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long b = __hip_atomic_load(&win[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long e = __hip_atomic_load(&win[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd(&win[2], b - t0);
        atomicAdd(&win[3], t_tail > e ? t_tail - e : 0ull);  // (tagged hand-off: the tail may start first)
        __hip_atomic_store(&win[0], ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&win[1], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// Workgroup 0 timeline of k_update (diagnostic): slot 24 + k accumulates
// the ticks from its start to mark k (thread 0 only).
__device__ __forceinline__ void wg0_mark(const Params& P, int k, unsigned long long t0) {
    if (P.stamps && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&P.stamps[24 + k], rtime() - t0);
}
// Sub-phase marks inside the update tail: slot 8+k accumulates the ticks since
// the previous mark (thread 0 only).
__device__ __forceinline__ unsigned long long tail_mark(const Params& P, int k, unsigned long long prev) {
    if (!P.stamps || threadIdx.x != 0) return prev;
    const unsigned long long now = rtime();
    atomicAdd(&P.stamps[8 + k], now - prev);
    return now;
}

// Peer mailboxes (k_exchange, spx_kernels.hip; the fused exchange in k_price's pricing
// tail and k_ftran_bc's entry).  A rank that polls for MBOX_TIMEOUT_TICKS
// without seeing a peer's word stops with ST_HANDOFF_TIMEOUT.
constexpr unsigned long long MBOX_TIMEOUT_TICKS = 3000000000ull;  // 30 s of s_memrealtime (100 MHz)
constexpr int MBOX_FUSED_MAX_G = 64;  // ranks the fused receiver merges (k_ftran_bc LDS)
// Fused exchange (Params::mbox_fused): a loop pass's record carries the tag
// (epoch << 24) | (iteration + 1) in every word; the epoch (DevState,
// advanced by every reset on every rank) keeps a record of an earlier solve
// from matching after the iteration count restarts.  k_exchange's seq tags
// stay below 2^24, so the two never match each other's words.
__device__ __forceinline__ uint32_t mbox_tag(uint32_t epoch, int64_t it) {
    return (epoch << 24) | ((uint32_t)(it + 1) & 0xFFFFFFu);
}
// word h of rank g's record in this rank's mailbox, polled until it carries tag
__device__ __forceinline__ bool mbox_poll(const Params& P, int64_t par, int g, int h, uint32_t tag,
                                          uint32_t* half) {
    const int64_t nh = (int64_t)P.pr_stride * 4;
    const uint64_t* q = &P.mbox[(par * P.nin + g) * nh + h];
    const unsigned long long t0 = rtime();
    for (;;) {
        const uint64_t w = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if ((uint32_t)(w >> 32) == tag) {
            *half = (uint32_t)w;
            return true;
        }
        if (rtime() - t0 > MBOX_TIMEOUT_TICKS) {
            *half = 0u;
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// Ratio-test partials of the k_update workgroups, stored field-major: field f
// of workgroup g at upd_soa[f * upd_cap + g].  A wave's loads of one field
// over 64 workgroups are then 512 contiguous bytes; with 64-byte records every
// lane's field load was a line of its own (7 x 512 line requests from the one
// CU that runs the tail).
// PLAIN: read only after the kernel boundary (the deferred tail)
template <bool PLAIN = false>
__device__ __forceinline__ void upd_publish(const Params& P, int g, const UpdPartial& w) {
    double* const s = P.upd_soa + g;
    const int64_t c = P.upd_cap;
    auto st = [](auto* q, auto v) {
        if constexpr (PLAIN) *q = v;
        else st_agent(q, v);
    };
    st(&s[0 * c], w.theta);
    st(reinterpret_cast<int64_t*>(&s[1 * c]), w.idx);
    st(reinterpret_cast<int64_t*>(&s[2 * c]), w.nonpos);
    st(&s[3 * c], w.T);
    st(&s[4 * c], w.a_w);
    st(&s[5 * c], w.cb_w);
    st(reinterpret_cast<int64_t*>(&s[6 * c]), w.bix_w);
}
// PLAIN: after a kernel boundary (the deferred tail) the partials are read
// with ordinary loads, so each XCD's L2 serves its workgroups after the first
// miss; inside the producing launch they need agent-scope loads
template <bool PLAIN = false>
__device__ __forceinline__ UpdPartial upd_fetch(const Params& P, int g) {
    const double* const s = P.upd_soa + g;
    const int64_t c = P.upd_cap;
    auto ld = [](const auto* q) { return PLAIN ? *q : ld_agent(q); };
    UpdPartial v;
    v.theta = ld(&s[0 * c]);
    v.idx = ld(reinterpret_cast<const int64_t*>(&s[1 * c]));
    v.nonpos = ld(reinterpret_cast<const int64_t*>(&s[2 * c]));
    v.T = ld(&s[3 * c]);
    v.a_w = ld(&s[4 * c]);
    v.cb_w = ld(&s[5 * c]);
    v.bix_w = ld(reinterpret_cast<const int64_t*>(&s[6 * c]));
    v.pad = 0;
    return v;
}

// Tagged hand-off (P.upd_tag, the default on replicated B^-1): wave 0 of every
// workgroup publishes its partial as UPD_WORDS 8-byte granules {32-bit half,
// tag} with one sc1 store instruction (lane l = word l; field-major, so the
// poll's loads coalesce), and the last workgroup polls each slot until all
// its words carry this pass's tag (MI355X_MICROARCH.md, handoff-1to1).  The
// slowest workgroup's partial then reaches the tail in one one-way hop; the
// counted form (upd_soa + arrive_last) pays a store drain and two atomic
// round trips first.  The tail clears every slot it consumed, so a slot holds
// a live tag only between its publish and the tail of the same pass.
__device__ __forceinline__ uint64_t upd_field_bits(const UpdPartial& w, int f) {
    switch (f) {
        case 0: return (uint64_t)__double_as_longlong(w.theta);
        case 1: return (uint64_t)w.idx;
        case 2: return (uint64_t)w.nonpos;
        case 3: return (uint64_t)__double_as_longlong(w.T);
        case 4: return (uint64_t)__double_as_longlong(w.a_w);
        case 5: return (uint64_t)__double_as_longlong(w.cb_w);
        default: return (uint64_t)w.bix_w;
    }
}
__device__ __forceinline__ void upd_publish_tagged(const Params& P, int g, const UpdPartial& w, uint32_t tag,
                                                   int lane) {
    if (lane < UPD_WORDS) {
        const uint64_t u = upd_field_bits(w, lane >> 1);
        const uint32_t half = (lane & 1) ? (uint32_t)(u >> 32) : (uint32_t)u;
        st_agent(&P.upd_tag[(int64_t)lane * P.upd_cap + g], ((uint64_t)tag << 32) | half);
    }
}
// Poll slot g until its UPD_WORDS words carry tag; false after ~2^20 rounds.
__device__ __forceinline__ bool upd_poll_tagged(const Params& P, int g, uint32_t tag, UpdPartial& v) {
    uint64_t w[UPD_WORDS];
    for (uint32_t spins = 0;; ++spins) {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < UPD_WORDS; ++k) w[k] = ld_agent(&P.upd_tag[(int64_t)k * P.upd_cap + g]);
#pragma unroll
        for (int k = 0; k < UPD_WORDS; ++k) ok = ok && (uint32_t)(w[k] >> 32) == tag;
        if (ok) break;
        if (spins > (1u << 20)) return false;
        __builtin_amdgcn_s_sleep(1);
    }
    uint64_t f[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) f[k] = (w[2 * k] & 0xffffffffull) | (w[2 * k + 1] << 32);
    v.theta = __longlong_as_double((long long)f[0]);
    v.idx = (int64_t)f[1];
    v.nonpos = (int64_t)f[2];
    v.T = __longlong_as_double((long long)f[3]);
    v.a_w = __longlong_as_double((long long)f[4]);
    v.cb_w = __longlong_as_double((long long)f[5]);
    v.bix_w = (int64_t)f[6];
    v.pad = 0;
    return true;
}
__device__ __forceinline__ void upd_clear_tagged(const Params& P, int g) {
#pragma unroll
    for (int k = 0; k < UPD_WORDS; ++k) P.upd_tag[(int64_t)k * P.upd_cap + g] = 0ull;
}

// Leaving argmin over the k_update workgroup partials + unbounded count
// (v4:317-325), carrying the winner's scalars.  One dependent round trip
// (the sc1 partial loads); result broadcast to every thread.  The T sum's
// order is fixed for a given launch geometry.
// The workgroup's merge of its threads' ratio-test partials (the second half
// of reduce_update_partials; the deferred tail calls it on partials it
// requested at kernel entry)
// wave: DPP argmin on (theta, idx) and DPP sums (no LDS round trips); the
// winner's scalars come from its lane by readlane
__device__ __forceinline__ UpdPartial wave_reduce_partial(const UpdPartial& w) {
    double th = w.theta;
    int64_t ix = w.idx;
    double T = w.T;
    int np = (int)w.nonpos;
    lane_argmin<64>(th, ix);
    lane_sum<64>(T);
    lane_isum<64>(np);
    th = readlane_d(th, 63);
    ix = readlane_l(ix, 63);
    const uint64_t hit = __ballot(w.theta == th && w.idx == ix);
    const int wl = hit ? (int)__builtin_ctzll(hit) : 0;
    UpdPartial o;  // (cross-lane reads outside the lane-0 branch)
    o.theta = th;
    o.idx = ix;
    o.nonpos = __builtin_amdgcn_readlane(np, 63);
    o.T = readlane_d(T, 63);
    o.a_w = readlane_d(w.a_w, wl);
    o.cb_w = readlane_d(w.cb_w, wl);
    o.bix_w = readlane_l(w.bix_w, wl);
    o.pad = 0;
    return o;
}
template <int BLOCK, bool PLAIN>
__device__ __forceinline__ UpdPartial reduce_partial_block(const UpdPartial& w, UpdPartial* red) {
    constexpr int WAVES = BLOCK / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const UpdPartial o = wave_reduce_partial(w);
    if (lane == 0) red[wave] = o;
    lds_barrier();
    if constexpr (PLAIN) {
        // the deferred tail (k_price's prologue, k_apply_tail): every wave
        // partial requested before a branch-free merge, and no closing
        // barrier (the callers pass an LDS array of their own).  (In the
        // FTRAN pass's tail the 8 partials in registers spilled.)
        UpdPartial r[WAVES];
#pragma unroll
        for (int k = 0; k < WAVES; ++k) r[k] = red[k];
        UpdPartial t = r[0];
#pragma unroll
        for (int k = 1; k < WAVES; ++k) upd_merge_sel(t, r[k]);
        return t;
    } else {
        UpdPartial t = red[0];
#pragma unroll
        for (int k = 1; k < WAVES; ++k) upd_merge(t, red[k]);
        lds_barrier();
        return t;
    }
}

// The 2*BLOCK-thread merge above (PLAIN) with BLOCK threads, bit for bit:
// thread tid holds the partials of that shape's threads tid (wa) and
// tid + BLOCK (wb), so its waves w and w + WAVES reduce the same lanes in the
// same order, and the 2*WAVES wave partials merge in the same order.
template <int BLOCK>
__device__ __forceinline__ UpdPartial reduce_partial_pair(const UpdPartial& wa, const UpdPartial& wb,
                                                          UpdPartial* red) {
    constexpr int WAVES = BLOCK / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const UpdPartial oa = wave_reduce_partial(wa);
    const UpdPartial ob = wave_reduce_partial(wb);
    if (lane == 0) {
        red[wave] = oa;
        red[wave + WAVES] = ob;
    }
    lds_barrier();
    UpdPartial r[2 * WAVES];
#pragma unroll
    for (int k = 0; k < 2 * WAVES; ++k) r[k] = red[k];
    UpdPartial t = r[0];
#pragma unroll
    for (int k = 1; k < 2 * WAVES; ++k) upd_merge_sel(t, r[k]);
    return t;
}

template <int BLOCK, bool PLAIN = false>
__device__ UpdPartial reduce_update_partials(const Params& P, UpdPartial* red, int nparts, uint32_t tag = 0,
                                             bool* timed_out = nullptr) {
    const int tid = threadIdx.x;
    UpdPartial w = upd_empty();
    if (tag) {  // tagged hand-off: poll, then clear the consumed slots
        bool ok = true;
        for (int g = tid; g < nparts; g += BLOCK) {
            UpdPartial v;
            if (!upd_poll_tagged(P, g, tag, v)) {
                ok = false;
                break;
            }
            upd_merge(w, v);
            upd_clear_tagged(P, g);
        }
        if (!ok) *timed_out = true;  // (a benign race: every writer stores true)
    } else {
        // every slot's seven fields are loaded before any is used (one round trip)
        w = (tid < nparts) ? upd_fetch<PLAIN>(P, tid) : upd_empty();
        for (int g = tid + BLOCK; g < nparts; g += BLOCK) upd_merge(w, upd_fetch<PLAIN>(P, g));
    }
    return reduce_partial_block<BLOCK, PLAIN>(w, red);
}

// LDS carve-up of k_update (dynamic, 16-byte aligned pieces)
template <int BLOCK>
struct UpdLds {
    static constexpr int WAVES = BLOCK / 64;
    static constexpr size_t red = 0;                                    // UpdPartial[WAVES]
    static constexpr size_t last = red + sizeof(UpdPartial) * WAVES;    // int
    static constexpr size_t bytes = last + 16;
};

// Basis bookkeeping (v4:339-342) + non-basic list swap-remove / append and
// the deferred pivot state (spx_device.h).  One thread.
// Scalars of the bookkeeping that only depend on the entering column, loaded
// by every k_update workgroup at its start so the last one's tail does not
// wait on a chain of dependent global loads.
// (32-bit flags: with bool members the partly-assigned struct was kept in
// scratch rather than registers)
struct TailPre {
    int32_t valid;
    double c_p;
    int32_t cnt, kp, last;
    double wp;  // Devex: the entering column's weight
    int32_t has_e;
    double e_enter;  // deferred pricing tail: the entering column's reduced cost
    int32_t nw;      // eta window: pivots in the window (stable until the tail)
};
// the list tail depends on cnt: loaded at the start of the tail, beside the
// partial loads, instead of as a dependent pair at kernel entry
__device__ __forceinline__ void tail_last(const Params& P, TailPre* t) {
    if (t && t->valid && t->kp >= 0) t->last = P.nb_list[t->cnt - 1];
}

// Devex / steepest edge on a column-shard group: the winning rank's record
// carries the entering column's reduced cost and weight after its window
// coefficients (Params::pr_stride), since only that rank prices the column
__device__ __forceinline__ const double* dvx_payload(const Params& P, int gw) {
    return reinterpret_cast<const double*>(P.price_in + gw * P.pr_stride + 1 + P.win / 2);
}

__device__ __forceinline__ TailPre tail_prefetch(const Params& P, int32_t nw, int32_t cnt, int64_t p) {
    TailPre t{0, 0.0, 0, -1, -1, 0.0, 0, 0.0, 0};
    if (p < 0 || p >= P.n) return t;
    if (P.win) t.nw = nw;
    t.c_p = P.c[p];
    t.cnt = cnt;
    if (owns_col(P, p)) t.kp = P.nb_pos[p];  // (nb_list[cnt - 1] is loaded by the tail: tail_last)
    if (P.devex) t.wp = P.W[p];
    t.valid = true;
    return t;
}

__device__ __forceinline__ void pivot_bookkeeping(const Params& P, DevState* st, int64_t p, int64_t q,
                                                  int64_t leave, double aq, double s_y, double min_e,
                                                  int64_t it, const TailPre* pre = nullptr) {
    P.c_B[q] = pre ? pre->c_p : P.c[p];
    P.b_ixs[q] = p;
    if (P.rleft) P.rleft[q] = 1;  // column q of B^-1 may stop being e_q
    int cnt = pre ? pre->cnt : st->nb_count;
    if (owns_col(P, p)) {
        const int kp = pre ? pre->kp : P.nb_pos[p];
        const int last = pre ? pre->last : P.nb_list[cnt - 1];
        P.nb_list[kp] = last;
        P.nb_pos[last] = kp;
        P.nb_pos[p] = -1;
        --cnt;
    }
    if (owns_col(P, leave)) {
        P.nb_list[cnt] = (int32_t)leave;
        P.nb_pos[leave] = cnt;
        ++cnt;
    }
    st->nb_count = cnt;
    st->aq = aq;
    st->s_y = s_y;
    if (P.win) {  // eta window: the pivot joins the window as its pending entry
        const int32_t nw = (pre && pre->valid) ? pre->nw : st->nw;
        P.SY[nw] = s_y;
        st->nw = nw + 1;
    } else {
        if (st->y_applied < it) st->y_buf ^= 1;  // k_price of this pass persisted y
        st->y_applied = it;
    }
    st->xb_applied = it;
    if (P.devex) {
        st->leave = leave;
        st->wp = pre ? pre->wp : P.W[p];
    }
    st->p = p;
    st->q = q;
    st->min_e = min_e;  // the entering reduced cost (callers resolve Devex's key)
    st->iter = it + 1;
    record_pivot(P, it, p, q);
}

// The last workgroup of k_update (single rank / replicated B^-1): leaving
// row q, unboundedness (v4:317-325), alpha_q, s_y and the bookkeeping.  The
// vector updates are deferred (spx_device.h).
template <int BLOCK>
__device__ void update_tail(const Params& P, DevState* st, int64_t p, double min_e, int64_t it,
                            unsigned char* smem, int nparts, TailPre* pre = nullptr, uint32_t tag = 0) {
    unsigned long long tm = P.stamps ? rtime() : 0;
    if (threadIdx.x == 0) tail_last(P, pre);
    UpdPartial* red = reinterpret_cast<UpdPartial*>(smem + UpdLds<BLOCK>::red);
    __shared__ bool s_to;
    if (threadIdx.x == 0) s_to = false;
    if (tag) lds_barrier();
    const UpdPartial t = reduce_update_partials<BLOCK>(P, red, nparts, tag, &s_to);
    tm = tail_mark(P, 0, tm);
    if (threadIdx.x != 0) return;
    if (tag && s_to) {  // a partial never arrived (a fault elsewhere): stop loudly
        st->status = ST_HANDOFF_TIMEOUT;
        return;
    }
    const int64_t q = t.idx;
    if (t.nonpos == P.m || q < 0 || q >= P.m) {
        // every alpha_i <= 0: Unbounded (v4:319-322).  A ratio test with no
        // valid candidate (NaN-poisoned x_b) stops the same way.  The deferred
        // state of the previous pivot (q, aq, s_y) is left intact for k_flush.
        st->p = p;
        st->min_e = min_e;
        st->status = ST_UNBOUNDED;
        return;
    }
    const double c_p = pre ? pre->c_p : P.c[p];
    const double e_rep = !P.devex ? min_e : (pre && pre->has_e ? pre->e_enter : *P.dvx_e);
    pivot_bookkeeping(P, st, p, q, t.bix_w, t.a_w, y_scalar(t.T, t.a_w, t.cb_w, c_p), e_rep, it, pre);
    tail_mark(P, 1, tm);
}

// The deferred tail's bookkeeping from the reduced partial t (update_tail's,
// with the FTRAN pass's TailRec in place of its prefetched scalars).  One
// thread: workgroup 0 of the next pricing pass, or k_apply_tail.
__device__ __forceinline__ void apply_deferred_tail(const Params& P, DevState* st, const TailRec& R,
                                                    const UpdPartial& t) {
    const int64_t q = t.idx;
    if (t.nonpos == P.m || q < 0 || q >= P.m) {  // Unbounded (v4:319-322)
        st->p = R.p;
        st->min_e = R.e_rep;
        st->status = ST_UNBOUNDED;
        return;
    }
    const TailPre pre{1, R.c_p, R.cnt, R.kp, R.last, R.wp, 0, 0.0, R.nw};
    pivot_bookkeeping(P, st, R.p, q, t.bix_w, t.a_w, y_scalar(t.T, t.a_w, t.cb_w, R.c_p), R.e_rep, R.it, &pre);
}

// Row-sharded tail (last workgroup of k_update on this rank): the local
// leaving candidate with its scalars, the local sum T of c_B[i] * alpha_i, and
// the candidate's row of B^-1_new — recomputed from the old rows exactly as the
// stream wrote it — into rs_send for the ratio-test all-gather.  No global
// state changes: k_finalize_rs does them after the exchange.
template <int BLOCK>
__device__ void update_tail_rs(const Params& P, DevState* st, int64_t it, int par, const double* a_prev,
                               unsigned char* smem, int nparts) {
    const int tid = threadIdx.x;
    UpdPartial* red = reinterpret_cast<UpdPartial*>(smem + UpdLds<BLOCK>::red);
    const UpdPartial t = reduce_update_partials<BLOCK>(P, red, nparts);
    RsHeader* h = reinterpret_cast<RsHeader*>(P.rs_send);
    double* row = reinterpret_cast<double*>(P.rs_send + sizeof(RsHeader));
    const bool have = t.idx >= P.r0 && t.idx < P.r0 + P.mloc;
    if (have) {
        const int64_t i = t.idx, L2 = P.L >> 1;
        const double e = (it > 0) ? eta_entry(a_prev[i], i, st->q, st->aq) : 0.0;
        const dbl2* sr = reinterpret_cast<const dbl2*>((par ? P.B1 : P.B0) + (i - P.r0) * P.L);
        const dbl2* rb = reinterpret_cast<const dbl2*>(it > 0 ? P.rbuf : P.zeros);
        dbl2* out = reinterpret_cast<dbl2*>(row);
        for (int64_t k = tid; k < L2; k += BLOCK) {
            const dbl2 bv = sr[k], rv = rb[k];
            dbl2 nv;
            nv.x = fma(e, rv.x, bv.x);
            nv.y = fma(e, rv.y, bv.y);
            out[k] = nv;
        }
    }
    if (tid == 0) {
        h->theta = t.theta;
        h->idx = have ? t.idx : INT64_MAX;
        h->nonpos = t.nonpos;
        h->T = t.T;
        h->a_w = t.a_w;
        h->cb_w = t.cb_w;
        h->bix_w = t.bix_w;
    }
}

// Harris ratio test, second pass (SPX_RATIO_HARRIS; runs in k_tail, after
// the k_update boundary made every row's alpha and updated x_b visible).  The
// partials carry theta_max = min (max(x_b,0) + feas_tol) / alpha_i, the
// nonpos count and T; the leaving row is the largest alpha_i among rows with
// max(x_b_i,0) / alpha_i <= theta_max, first index on ties (the same rule as
// oracle/simplex_oracle.c ratio_harris).
template <int BLOCK>
__device__ void harris_tail(const Params& P, DevState* st, int64_t p, double min_e, int64_t it,
                            unsigned char* smem, int nparts) {
    constexpr int WAVES = BLOCK / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    UpdPartial* red = reinterpret_cast<UpdPartial*>(smem + UpdLds<BLOCK>::red);
    const UpdPartial t = reduce_update_partials<BLOCK>(P, red, nparts);
    if (t.nonpos == P.m || t.idx < 0 || t.idx >= P.m) {
        if (tid == 0) {  // Unbounded (v4:319-322), as update_tail
            st->p = p;
            st->min_e = min_e;
            st->status = ST_UNBOUNDED;
        }
        return;
    }
    const double thmax = t.theta;
    const double* a_new = (it & 1) ? P.alpha0 : P.alpha1;
    double bv = INFINITY;  // -alpha of the best candidate
    int64_t bi = INT64_MAX;
    for (int64_t i = tid; i < P.m; i += BLOCK) {
        const double a = a_new[i];
        if (a > P.piv_tol) {
            const double xb = P.x_b[i];
            const double xc = xb > 0.0 ? xb : 0.0;
            if (xc / a <= thmax && argmin_better(-a, i, bv, bi)) { bv = -a; bi = i; }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double v = __shfl_xor(bv, off, 64);
        const int64_t i = __shfl_xor(bi, off, 64);
        if (argmin_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    __syncthreads();
    ArgMinEntry* wr = reinterpret_cast<ArgMinEntry*>(red);  // reuse the partial slots
    if (lane == 0) wr[wave] = ArgMinEntry{bv, bi};
    __syncthreads();
    if (tid != 0) return;
    ArgMinEntry w = wr[0];
    for (int k = 1; k < WAVES; ++k)
        if (argmin_better(wr[k].val, wr[k].idx, w.val, w.idx)) w = wr[k];
    const int64_t q = w.idx;  // exists: pass 1's winner satisfies the bound
    const double aq = a_new[q], cbq = P.c_B[q];
    pivot_bookkeeping(P, st, p, q, P.b_ixs[q], aq, y_scalar(t.T, aq, cbq, P.c[p]), P.devex ? *P.dvx_e : min_e, it);
}

}  // namespace spx
