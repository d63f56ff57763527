// spx_kernels.hip — the kernels around the hot loop's two launches (the pass
// and the kernel units are described at the head of spx_kernels.h): the
// deferred state's flush and the readbacks, setup (generate, reset), the
// mailbox MINLOC exchange, and steepest edge's preparation before a pricing
// pass.
#include <hip/hip_runtime.h>
#include <math.h>

#include "spx_device.h"
#include "spx_common.h"
#include "spx_handoff.h"
#include "spx_kernels.h"

namespace spx {

// Block-wide sum: wave butterflies, then the per-wave sums in wave order.
template <int BLOCK>
__device__ double block_sum(double a, double* sa) {
    constexpr int WAVES = BLOCK / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    a = wave_sum(a);
    if (lane == 0) sa[wave] = a;
    __syncthreads();
    double t = sa[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) t += sa[w];
    __syncthreads();
    return t;
}

// ---------------------------------------------------------------------------
// Deferred-state flush and readback kernels (off the hot loop)
// ---------------------------------------------------------------------------
// Applies the pending y and x_b updates of the last pivot (one workgroup).
__global__ __launch_bounds__(1024) void k_flush(Params P) {
    constexpr int BLOCK = 1024;
    DevState* st = P.st;
    const int tid = threadIdx.x;
    const int64_t it = st->iter, L = P.L, L2 = L >> 1, m = P.m;
    if (it == 0) return;
    // eta window: the host folded first, so at most the pending pivot is left
    // (nw <= 1) and the state has the explicit-B^-1 form with B_w as the
    // stored matrix (B0 either way; row shards keep the pivot row in rbuf)
    const double* r = P.row_shard ? P.rbuf : P.B0 + st->q * L;
    const bool upd_y = P.win ? st->nw == 1 : st->y_applied < it;
    const bool upd_x = st->xb_applied < it;
    if (upd_y) {
        const dbl2* yin = reinterpret_cast<const dbl2*>(st->y_buf ? P.y1 : P.y0);
        dbl2* yout = reinterpret_cast<dbl2*>(st->y_buf ? P.y0 : P.y1);
        const dbl2* r2 = reinterpret_cast<const dbl2*>(r);
        const double sy = P.win ? P.SY[0] : st->s_y;
        for (int64_t k = tid; k < L2; k += BLOCK) yout[k] = y_apply(sy, r2[k], yin[k]);
        // window tableau: dw = y_w A - c follows y_w; the pending pivot is
        // tau = 0 after the fold, so r.A_j = T_w[q, j]
        if (P.tab)
            for (int64_t j = tid; j < P.n; j += BLOCK) P.dw[j] = fma(sy, P.T[j * L + st->q], P.dw[j]);
    }
    if (upd_x) {
        // s_x exactly as k_update's row stream accumulates it (every wave alike)
        const dbl2* r2 = reinterpret_cast<const dbl2*>(r);
        const dbl2* b2 = reinterpret_cast<const dbl2*>(P.b);
        double sxa = 0.0;
        for (int64_t k = tid & 63; k < L2; k += 64) {
            sxa = fma(r2[k].x, b2[k].x, sxa);
            sxa = fma(r2[k].y, b2[k].y, sxa);
        }
        const double s_x = wave_sum(sxa);
        const double* a_prev = (it & 1) ? P.alpha1 : P.alpha0;
        const int64_t q = st->q;
        const double aq = st->aq;
        const int64_t i0 = P.row_shard ? P.r0 : 0, i1 = P.row_shard ? P.r0 + P.mloc : m;  // own rows
        for (int64_t i = i0 + tid; i < i1; i += BLOCK) P.x_b[i] = fma(s_x, eta_entry(a_prev[i], i, q, aq), P.x_b[i]);
    }
    __syncthreads();
    if (tid == 0) {
        if (upd_y) {
            st->y_buf ^= 1;
            st->y_applied = it;
            if (P.win) P.SY[0] = 0.0;  // y_w now includes the pending pivot
        }
        if (upd_x) st->xb_applied = it;
    }
}

// true B^-1 = S + E r^T into out (m x L row-major; row-sharded: own rows only,
// at their global positions)
__global__ void k_materialize(Params P, double* out) {
    const DevState* st = P.st;
    const int64_t it = st->iter;
    const bool rs = P.row_shard != 0;
    const double* S = rs ? ((it & 1) ? P.B1 : P.B0) : P.B0;  // (only row shards ping-pong)
    const double* r = rs ? P.rbuf : S + st->q * P.L;
    const double* a_prev = (it & 1) ? P.alpha1 : P.alpha0;
    const int64_t q = st->q;
    const double aq = st->aq;
    const int64_t r0 = rs ? P.r0 : 0;
    const int64_t total = (rs ? P.mloc : P.m) * P.L;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t li = t / P.L, k = t - li * P.L, i = r0 + li;
        out[r0 * P.L + t] = (it > 0) ? fma(eta_entry(a_prev[i], i, q, aq), r[k], S[t]) : S[t];
    }
}

// e_j for every column from the current (flushed) y, one wave per column
__global__ __launch_bounds__(256) void k_reduced_costs(Params P, double* e) {
    const int lane = threadIdx.x & 63;
    const int64_t L2 = P.L >> 1;
    const dbl2* y2 = reinterpret_cast<const dbl2*>(P.st->y_buf ? P.y1 : P.y0);
    for (int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; j < P.n;
         j += ((int64_t)gridDim.x * blockDim.x) >> 6) {
        const dbl2* col = reinterpret_cast<const dbl2*>(P.A + j * P.L);
        double a0 = 0.0, a1 = 0.0;
        for (int64_t k = lane; k < L2; k += 64) {
            const dbl2 v = col[k], w = y2[k];
            a0 = fma(v.x, w.x, a0);
            a1 = fma(v.y, w.y, a1);
        }
        const double s = wave_sum(a0 + a1) - P.c[j];
        if (lane == 0) e[j] = s;
    }
}

// z = c_B . x_b (v4:365), from the flushed x_b
__global__ __launch_bounds__(256) void k_objective(Params P) {
    __shared__ double sa[4];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < P.m; i += 256) s = fma(P.c_B[i], P.x_b[i], s);
    s = block_sum<256>(s, sa);
    if (threadIdx.x == 0) P.st->z = s;
}

// ---------------------------------------------------------------------------
// Setup kernels
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double uniform01(uint64_t seed, uint64_t stream, uint64_t idx) {
    const uint64_t key = (seed * 0x9E3779B97F4A7C15ULL) ^ (stream << 56) ^ idx;
    return (double)(splitmix64(key) >> 11) * 0x1.0p-53;
}

__global__ void k_generate(double* A, double* b, double* c, int64_t m, int64_t n, int64_t L,
                           uint64_t seed) {
    const int64_t ns = n - m;
    const int64_t total = L * n;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = t / L, i = t - j * L;
        double v = 0.0;
        if (i < m) v = (j < ns) ? uniform01(seed, 1, (uint64_t)(i + j * m)) : ((i == j - ns) ? 1.0 : 0.0);
        A[t] = v;
        if (j == 0) b[i] = (i < m) ? ((double)ns / 4.0) * (1.0 + uniform01(seed, 2, (uint64_t)i)) : 0.0;
        if (i == 0) c[j] = (j < ns) ? uniform01(seed, 3, (uint64_t)j) : 0.0;
    }
}

// slack basis (v4:268-277 with the intended semantics); vectors zeroed by the host
__global__ void k_reset(Params P) {
    const int64_t m = P.m, n = P.n, L = P.L, ns = P.ns;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t li = t0; li < P.mloc; li += stride) P.B0[li * L + P.r0 + li] = 1.0;  // init_I (v4:182-188)
    for (int64_t i = t0; i < m; i += stride) {
        P.c_B[i] = P.c[ns + i];
        P.x_b[i] = P.b[i];
        P.y0[i] = P.c[ns + i];
        P.b_ixs[i] = ns + i;
        if (P.xw) P.xw[i] = P.b[i];  // B_w = I
    }
    for (int64_t k = t0; k < ARR_GROUPS * ARR_LINES * ARR_STRIDE; k += stride) P.arrive[k] = 0u;
    if (P.trec && t0 == 0) P.trec->fresh = 0;
    if (P.upd_tag)
        for (int64_t k = t0; k < UPD_WORDS * P.upd_cap; k += stride) P.upd_tag[k] = 0ull;
    if (P.price_tag)
        for (int64_t k = t0; k < PRICE_WORDS * P.price_cap; k += stride) P.price_tag[k] = 0ull;
    for (int64_t j = t0; j < n; j += stride) {
        if (P.W) P.W[j] = 1.0;  // Devex reference framework
        int32_t pos = -1;
        if (j < ns && j >= P.s_lo && j < P.s_hi) {
            pos = (int32_t)(j - P.s_lo);
            P.nb_list[pos] = (int32_t)j;
        }
        P.nb_pos[j] = pos;
    }
    if (t0 == 0) {
        DevState* st = P.st;
        st->status = ST_RUNNING;
        st->nb_count = (int32_t)(P.s_hi - P.s_lo);
        st->iter = 0;
        st->limit = 0;
        st->p = -1;
        st->q = -1;
        st->min_e = 0.0;
        st->z = 0.0;
        st->aq = 1.0;
        st->s_y = 0.0;
        st->y_applied = 0;
        st->xb_applied = 0;
        st->y_buf = 0;
        st->nw = 0;
        st->leave = -1;
        st->wp = 1.0;
        st->uncovered = 0u;
        st->mbox_epoch = st->mbox_epoch + 1u;  // (every rank resets alike)
    }
}

// ---------------------------------------------------------------------------
// MINLOC exchange through peer mailboxes (spx_mbox_attach): the replacement
// for the all-gather of the candidate records (v4:294-302 runs the argmin on
// one device; across ranks every rank needs every record).  One workgroup:
// this rank's record (price_out, written by k_price) is stored as tagged
// words into slot [seq & 1][rank] of every rank's mailbox, then the nin
// slots of this rank's own mailbox are polled until every word carries seq
// and unpacked into price_in, which k_update reads as it reads the RCCL
// all-gather's output.  Each 8-byte word is stored and loaded whole, so a
// record is complete when all its tags match, with no fence or flag.  Two
// parities suffice: a rank reaches exchange seq + 2 only after every rank's
// record of seq + 1, which each stored after consuming seq.  System-scope
// stores and loads (the mailboxes are fine-grained, mapped over xGMI on other
// devices).  A rank that polls for MBOX_TIMEOUT_TICKS without seeing a peer
// stops with ST_HANDOFF_TIMEOUT, and its later exchanges only send.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_exchange(Params P) {
    const int tid = threadIdx.x;
    const int G = P.nin;
    const int nh = P.pr_stride * (int)(sizeof(ArgMinEntry) / 4);  // 32-bit halves per record
    const uint32_t seq = ld_agent(P.mbox_seq) + 1u;
    const int64_t par = seq & 1u;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(P.price_out);
    for (int k = tid; k < G * nh; k += 256) {
        const int g = k / nh, h = k - g * nh;
        const uint64_t w = ((uint64_t)seq << 32) | src[h];
        __hip_atomic_store(&P.mbox_peer[g][(par * G + P.mbox_rank) * nh + h], w, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const bool dead = ld_agent(&P.st->status) == ST_HANDOFF_TIMEOUT;
    __shared__ int s_to;
    if (tid == 0) s_to = 0;
    __syncthreads();
    uint32_t* dst = reinterpret_cast<uint32_t*>(const_cast<ArgMinEntry*>(P.price_in));
    const unsigned long long t0 = rtime();
    for (int k = tid; k < G * nh; k += 256) {
        const uint64_t* p = &P.mbox[par * G * nh + k];
        uint64_t w = 0;
        bool ok = false;
        while (!dead) {
            w = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if ((uint32_t)(w >> 32) == seq) {
                ok = true;
                break;
            }
            if (rtime() - t0 > MBOX_TIMEOUT_TICKS) break;
            __builtin_amdgcn_s_sleep(2);
        }
        if (!ok) s_to = 1;  // (a benign race: every writer stores 1)
        dst[k] = (uint32_t)w;
    }
    __syncthreads();
    if (tid == 0) {
        st_agent(P.mbox_seq, seq);
        if (s_to) P.st->status = ST_HANDOFF_TIMEOUT;
    }
}

hipError_t launch_exchange(const Params& P, hipStream_t s) {
    hipLaunchKernelGGL(k_exchange, dim3(1), dim3(256), 0, s, P);
    return hipGetLastError();
}

static int grid_for(int64_t work, int block) {
    int64_t g = (work + block - 1) / block;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (int)g;
}

hipError_t launch_generate(double* A, double* b, double* c, int64_t m, int64_t n, int64_t L, uint64_t seed,
                           hipStream_t s) {
    hipLaunchKernelGGL(k_generate, dim3(grid_for(L * n, 256) * 4), dim3(256), 0, s, A, b, c, m, n, L, seed);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Steepest-edge pricing (SPX_PRICING_STEEPEST; oracle se_choose).  Weights
// gamma_j = 1 + ||B^-1 A_j||^2: exact at the slack basis (k_se_init), then
// kept by the Goldfarb-Reid recurrence inside k_price, which needs for the
// pending pivot (alpha = its FTRAN column, a_prev of the coming pass; B^-1
// before it = B_w + sum_{s<tau} eta_s r_s^T):
//   A_j . B^-T alpha = (B_w^T alpha) . A_j + sum_{s<tau} (U[:, s] . alpha) Wt[j][s]
// and gamma_p = 1 + ||alpha||^2.  k_se_part / k_se_fin form those before each
// pricing pass (after any fold): the column sums of M^T alpha for M = [B_w's
// columns (the compact list, or all of B_w) | U | alpha], per row block in
// ascending row order, then over the blocks in ascending order.
// ---------------------------------------------------------------------------
// Round 5: both kernels latency-bound no more (C3 steepest pass: the two took
// about 28 us): k_se_part's threads request a 16-row block of their column at
// once, and k_se_fin sums the row-block partials in slices of threads
// (coalesced, several loads in flight per thread), then the slices in
// ascending order.  Round 6: k_ftran_bc forms k_se_part's sums itself on
// every pass but a window's first (Params::se_fused, 8-row partials).
constexpr int SE_RB = 16;     // rows per k_se_part workgroup

// The pending pivot (its alpha parity and the window position): from the
// state, or -- when the FTRAN pass deferred its tail (TailRec) -- from the
// record, as the next k_price derives it
__device__ __forceinline__ bool se_pending(const Params& P, int& nw, const double*& al) {
    const DevState* st = P.st;
    int64_t iter = st->iter;
    int32_t nwv = st->nw;
    if (P.trec) {
        const TailRec R = *P.trec;
        if (R.fresh) {
            iter = R.it + 1;
            nwv = R.nw + 1;
        }
    }
    if (st->status != ST_RUNNING || iter >= st->limit) return false;
    nw = nwv;
    al = (iter & 1) ? P.alpha1 : P.alpha0;  // alpha of the pending pivot
    return nw > 0;
}

__global__ __launch_bounds__(256) void k_se_part(Params P) {
    int nw;
    const double* al;
    if (!se_pending(P, nw, al)) return;
    const int64_t m = P.m, L = P.L;
    const int KW = P.win, tau = nw - 1;
    const int S = P.bc ? P.bc_n[0] : (int)m;
    const int ncols = S + KW + 1;
    const int64_t i0 = (int64_t)blockIdx.x * SE_RB;
    const int nr = (int)(m - i0 < SE_RB ? m - i0 : SE_RB);
    __shared__ double sa[SE_RB];
    if (threadIdx.x < SE_RB) sa[threadIdx.x] = threadIdx.x < nr ? al[i0 + threadIdx.x] : 0.0;
    __syncthreads();
    const double* Mw = P.bc ? bc_buf(P, P.bc_n[2]) : P.B0;
    const int64_t ldm = P.bc ? (int64_t)P.bc_n[1] : L;  // row pitch (compact: bc_pitch)
    double* out = P.se_part + (int64_t)blockIdx.x * (L + KW + 1);
    for (int c = threadIdx.x; c < ncols; c += blockDim.x) {
        // the block's rows of column c, requested together (rows clamped;
        // the sum takes rows < nr in ascending order)
        const double* src;
        int64_t ld;
        if (c < S) {
            src = Mw + c;
            ld = ldm;
        } else if (c < S + KW) {
            const int sc = c - S;
            src = P.U + (sc < tau ? sc : 0);
            ld = KW;
        } else {
            src = al;
            ld = 1;
        }
        double v[SE_RB];
#pragma unroll
        for (int r = 0; r < SE_RB; ++r) v[r] = src[(i0 + (r < nr ? r : nr - 1)) * ld];
        double acc = 0.0;
        const bool live = c < S || c >= S + KW || c - S < tau;
#pragma unroll
        for (int r = 0; r < SE_RB; ++r)
            if (r < nr && live) acc = fma(c < S + KW ? v[r] : sa[r], sa[r], acc);
        out[c] = acc;
    }
}

// (Round 6: SE_FC columns per workgroup and SE_FS slices of partials each --
// 16 x 64 instead of 64 x 16 -- so the sums of a C3 pass's ~520 columns
// spread over ~33 workgroups instead of 9: with the fused path's 512
// partials the 9 were bound by their CUs' load rate)
constexpr int SE_FC = 16;
constexpr int SE_FS = 1024 / SE_FC;
constexpr int SE_FB = 8;  // partials per slice per round trip

__global__ __launch_bounds__(1024) void k_se_fin(Params P) {
    int nw;
    const double* al;
    if (!se_pending(P, nw, al)) return;
    const int64_t m = P.m, L = P.L;
    const int KW = P.win;
    const int S = P.bc ? P.bc_n[0] : (int)m;
    const int ncols = S + KW + 1;
    const int64_t stride = L + KW + 1;
    const int tid = threadIdx.x, cl = tid % SE_FC, sl = tid / SE_FC;  // column in the group, slice
    const int64_t c = (int64_t)blockIdx.x * SE_FC + cl;
    __shared__ double red[SE_FS][SE_FC];
    // slice sl sums the partials g = sl, sl + SE_FS, ... (ascending), SE_FB at a time
    double v = 0.0;
    const int64_t cc = c < ncols ? c : 0;
    const int gend = (int64_t)blockIdx.x * SE_FC < ncols ? P.se_parts : 0;  // (groups past the columns: nothing)
    for (int g0 = sl; g0 < gend; g0 += SE_FS * SE_FB) {
        double t[SE_FB];
#pragma unroll
        for (int k = 0; k < SE_FB; ++k) {
            const int g = g0 + k * SE_FS;
            t[k] = P.se_part[(int64_t)(g < P.se_parts ? g : 0) * stride + cc];
        }
#pragma unroll
        for (int k = 0; k < SE_FB; ++k)
            if (g0 + k * SE_FS < P.se_parts) v += t[k];
    }
    red[sl][cl] = v;
    __syncthreads();
    if (sl == 0 && c < ncols) {
        double w = red[0][cl];
#pragma unroll 16
        for (int k = 1; k < SE_FS; ++k) w += red[k][cl];
        if (c < S) P.se_v[P.bc ? (int64_t)P.rlist[c] : c] = w;
        else if (c < S + KW) P.se_cg[c - S] = w;
        else P.se_cg[KW] = 1.0 + w;
    }
    if (P.bc) {  // the unit columns of B_w: (B_w^T alpha)_k = alpha_k
        const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + tid, nt = (int64_t)gridDim.x * blockDim.x;
        for (int64_t k = t0; k < m; k += nt)
            if (P.rmap[k] < 0) P.se_v[k] = al[k];
    }
}

// gamma_j = 1 + ||A_j||^2 for every column (the slack basis B = I), one wave
// per column, lane-strided then a butterfly
__global__ __launch_bounds__(256) void k_se_init(Params P) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwv = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t j = w0; j < P.n; j += nwv) {
        const double* col = P.A + j * P.L;
        double a = 0.0;
        for (int64_t k = lane; k < P.m; k += 64) a = fma(col[k], col[k], a);
        a = wave_sum(a);
        if (lane == 0) P.W[j] = 1.0 + a;
    }
}

hipError_t launch_se_init(const Params& P, hipStream_t s) {
    if (!P.steep) return hipSuccess;
    hipLaunchKernelGGL(k_se_init, dim3(grid_for(P.n * 64, 256)), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_se_prep(const Params& P, hipStream_t s, int fused_parts) {
    if (!P.steep) return hipSuccess;
    Params Q = P;
    if (fused_parts > 0) {
        Q.se_parts = fused_parts;  // the previous k_ftran_bc's workgroup partials (Params::se_fused)
    } else {
        hipLaunchKernelGGL(k_se_part, dim3((unsigned)P.se_parts), dim3(256), 0, s, P);
    }
    // SE_FC columns per workgroup (the columns in use, S + KW + 1, are at most L + KW + 1)
    hipLaunchKernelGGL(k_se_fin, dim3((unsigned)((P.L + P.win + 1 + SE_FC - 1) / SE_FC)), dim3(1024), 0, s, Q);
    return hipGetLastError();
}

int se_parts_for(int64_t m) { return (int)((m + SE_RB - 1) / SE_RB); }

hipError_t launch_reset(const Params& P, hipStream_t s) {
    const int64_t w = P.m > P.n ? P.m : P.n;
    hipLaunchKernelGGL(k_reset, dim3(grid_for(w, 256)), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_flush(const Params& P, hipStream_t s) {
    hipLaunchKernelGGL(k_flush, dim3(1), dim3(1024), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_materialize(const Params& P, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_materialize, dim3(grid_for((P.row_shard ? P.mloc : P.m) * P.L, 256)), dim3(256), 0, s, P,
                       out);
    return hipGetLastError();
}

hipError_t launch_reduced_costs(const Params& P, double* e, hipStream_t s) {
    hipLaunchKernelGGL(k_reduced_costs, dim3(grid_for(P.n * 64, 256)), dim3(256), 0, s, P, e);
    return hipGetLastError();
}

hipError_t launch_objective(const Params& P, hipStream_t s) {
    hipLaunchKernelGGL(k_objective, dim3(1), dim3(256), 0, s, P);
    return hipGetLastError();
}


}  // namespace spx
