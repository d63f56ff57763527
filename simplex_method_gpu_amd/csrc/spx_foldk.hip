// spx_foldk.hip — the eta window's fold kernels (between loop passes, every KW
// pivots): k_fold (dense B_w), the compact FTRAN operand's list and gather,
// k_cfold (the fold over the listed columns only), and launch_fold, which
// picks among them and the tableau's fold.  Tile and rebuild helpers shared
// with the reinversion and the tableau are in spx_fold.h.
#include <hip/hip_runtime.h>
#include <math.h>

#include "spx_device.h"
#include "spx_common.h"
#include "spx_fold.h"
#include "spx_kernels.h"
#include "spx_tableau.h"

namespace spx {

// ---------------------------------------------------------------------------
// Eta-window fold (spx_device.h): B_w += U[:, 0..nf) R, y_w += SY[0..nf) R for
// the nf = nw - 1 complete pivots of the window; the pending pivot stays
// pending as tau = 0.  A workgroup owns a 64-column stripe of B and a range of
// rows (spx_fold.h): its first tiles go in flight, wave 0 rebuilds R for the
// stripe (one column per lane: r_tau = Qrows[tau] + sum_{s<tau} Urows[tau][s]
// r_s) into LDS; then each wave updates 16-row x 64-column tiles with
// v_mfma_f64_16x16x4_f64 (K = the window, 4 pivots per step): the tile of B is
// the accumulator, U the A operand, R the B operand.  B is read and written
// once.  min_nw: fold only when nw >= min_nw (the loop asks for KW, a readback
// for 2).
// ---------------------------------------------------------------------------
template <int KW>
__global__ __launch_bounds__(FOLD_THREADS) void k_fold(Params P, int min_nw) {
    DevState* st = P.st;
    const int nw = st->nw;
    if (nw < min_nw || nw < 2) return;
    const int nf = nw - 1;
    __shared__ double Rl[KW][FOLD_RP];
    __shared__ double NT[KW][FOLD_NP<KW>];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t L = P.L;
    const int64_t c0 = (int64_t)blockIdx.x * 64;
    int64_t i0, i1;
    fold_rows(P.m, i0, i1);
    // spx_fold.h: first tiles in flight, R rebuilt by all four waves, tiles
    // (the rebuild's operands are requested ahead of the first tiles and the
    // barriers wait for LDS only: the rebuild does not wait for the tiles)
    FoldRPre<KW> rpre;
    fold_r_load<KW>(P.Urows, P.Qrows, L, c0, rpre);
    FoldTilePre<KW> pre;
    fold_tile_first<KW>(P.B0, P.U, nf, L, c0, i0, i1, pre);
    fold_stage_N_pre<KW>(rpre, nf, NT);
    lds_barrier();
    if (tid < 256) fold_rebuild_R4<KW, FOLD_RP>(P.Qrows, NT, nf, L, c0, Rl, &rpre);
    lds_barrier();
    fold_tiles<KW, FOLD_RP>(P.B0, P.U, nf, L, c0, i0, i1, Rl, pre, true);
    if (wave == 0 && blockIdx.y == 0) {
        // y_w += SY R for this stripe (t ascending, the rebuild's R)
        double* y = st->y_buf ? P.y1 : P.y0;
        const int sl = fold_slot(lane);
        double d = 0.0;
#pragma unroll
        for (int t = 0; t < KW; ++t)
            if (t < nf) d = fma(P.SY[t], Rl[t][sl], d);
        y[c0 + lane] += d;
    } else if (wave == 1) {
        // xw = B_w b follows B_w: xw += U (R b), R b = Wt[n][0..nf); the rows
        // spread over every workgroup, one lane per row, t ascending
        const double* wb = P.Wt + P.n * KW;
        const int64_t nwg = (int64_t)gridDim.x * gridDim.y;
        const int64_t rpw = (P.m + nwg - 1) / nwg;
        const int64_t r0 = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * rpw;
        const int64_t r1 = (r0 + rpw < P.m) ? r0 + rpw : P.m;
        for (int64_t i = r0 + lane; i < r1; i += 64) {
            double d = 0.0;
#pragma unroll
            for (int t = 0; t < KW; ++t)
                if (t < nf) d = fma(P.U[i * KW + t], wb[t], d);
            P.xw[i] += d;
        }
    }
    __syncthreads();
    if (tid == 0) {
        s_last = arrive_last(arrive_group(P.arrive, ARR_FOLD), gridDim.x * gridDim.y,
                             blockIdx.y * gridDim.x + blockIdx.x);
    }
    __syncthreads();
    if (s_last && tid == 0) {
        P.SY[0] = P.SY[nf];
        st->nw = 1;
    }
}

// ---------------------------------------------------------------------------
// Compact FTRAN operand (Params::bc): after every fold (and reset or
// reinversion) the rows that have left join the column list in ascending
// order (k_bc_list, one workgroup), then every row of B_w is gathered onto
// those columns (k_bc_gather).  The dense B_w stays the master copy.
// ---------------------------------------------------------------------------
// min_nw > 0 (the compact fold): only when that fold runs (k_fold's test),
// recording S and the pitch before the append in bc_n[3] / bc_n[4]
// carry (compact pricing, a loop fold): dw is carried across this fold, so a
// dw that belongs to the y_w being folded away is marked 2 for k_as_rows
__global__ __launch_bounds__(1024) void k_bc_list(Params P, int min_nw, int carry) {
    __shared__ int s_w[16];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (min_nw > 0) {
        const int nw = P.st->nw;
        if (nw < min_nw || nw < 2) return;
    }
    if (tid == 0) {
        s_base = P.bc_n[0];
        P.bc_n[3] = P.bc_n[0];
        P.bc_n[4] = P.bc_n[1];
        // compact pricing: y_w is about to change (or B_w was rebuilt): dw is
        // stale, unless this fold carries one that was valid (2, turned back
        // into 1 by k_as_order once k_as_rows has carried every column)
        P.bc_n[5] = (carry && min_nw > 0 && P.bc_n[5] == 1) ? 2 : 0;
    }
    __syncthreads();
    for (int64_t k0 = 0; k0 < P.m; k0 += 1024) {
        const int64_t k = k0 + tid;
        const bool nu = k < P.m && P.rleft[k] != 0 && P.rmap[k] < 0;
        const uint64_t bal = __ballot(nu);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int off = s_base, tot = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) off += s_w[w];
            tot += s_w[w];
        }
        if (nu) {
            P.rmap[k] = off + pre;
            P.rlist[off + pre] = (int32_t)k;
        }
        __syncthreads();
        if (tid == 0) s_base += tot;
        __syncthreads();
    }
    if (tid == 0) {
        P.bc_n[0] = s_base;
        // row pitch of bc: S rounded up to 64 doubles (512 B).  Rows then lie
        // back to back (m x pitch, contiguous), so a wave's rows spread over
        // the HBM channels; at the full pitch L every row started a multiple
        // of L * 8 bytes apart
        P.bc_n[1] = s_base > 0 ? ((s_base + 63) / 64) * 64 : 64;
    }
}
// Compact pricing (Params::AS): the rows of A the list gained, AS[j][c] =
// A[rlist[c], j] for c in [bc_n[3], S), right after k_bc_list (same min_nw
// test, before k_cfold resets the window count).  A rebuild starts from
// bc_n[0] = 0, so it copies every row.  One thread per (column, new row):
// the threads of a column read its scattered elements and store one run.
// Rows past as_cap are not copied (a compact pass stops before reading them).
// The dw carry (carry != 0 and k_bc_list found dw valid: bc_n[5] == 2): the
// fold about to run makes y_w += sum_{t<nf} SY[t] r_t, and Wt[j][t] = r_t . A_j
// is stored for every column (the non-basic ones by the pricing pass after
// pivot t, the basic ones by its FTRAN pass), so
//   dw[j] += sum_{t<nf} SY[t] Wt[j][t]
// is y_w . A_j - c_j for the new y_w without a stream of A.  The column's wave
// has lane t take the product of pivot t (rounded on its own), then the
// butterfly: an order no grid, dispatch or chunking enters.  Before k_cfold,
// whose last workgroup rewrites SY[0] and the window count.
__global__ __launch_bounds__(256) void k_as_rows(Params P, int min_nw, int carry) {
    int nw = 0;
    if (min_nw > 0) {
        nw = P.st->nw;
        if (nw < min_nw || nw < 2) return;
    }
    const int S0 = P.bc_n[3];
    const int S = P.bc_n[0] < P.as_cap ? P.bc_n[0] : P.as_cap;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= P.n) return;
    if (carry && min_nw > 0 && P.bc_n[5] == 2) {  // (uniform: the whole wave sums)
        const int lane = (int)(threadIdx.x & 63);
        const int KW = P.win, nf = nw - 1;
        double v = 0.0;
        if (lane < nf && lane < KW) v = mul_nc(P.SY[lane], P.Wt[j * KW + lane]);
        v = wave_sum(v);
        if (lane == 0) P.dw[j] += v;
    }
    for (int c = S0 + (int)(threadIdx.x & 63); c < S; c += 64)
        P.AS[j * P.as_ld + c] = P.A[j * P.L + P.rlist[c]];
}
// ... and the order its sum runs in (spx_device.h): rank of every list
// position under the key (lane of the dense stream, row), by counting (one
// workgroup; S^2 / 1024 compares per thread, S <= as_cap <= 4096)
// (the kernel after k_as_rows: marks a carried dw valid for the new y_w)
__global__ __launch_bounds__(1024) void k_as_order(Params P, int min_nw, int carry) {
    __shared__ int s_row[4096];
    if (min_nw > 0) {
        const int nw = P.st->nw;
        if (nw < min_nw || nw < 2) return;
    }
    const int S = P.bc_n[0] < P.as_cap ? P.bc_n[0] : P.as_cap;
    const int tid = threadIdx.x;
    for (int c = tid; c < S; c += 1024) s_row[c] = P.rlist[c];
    __syncthreads();
    auto key = [](int r) { return (int64_t)((r >> 1) & 63) << 32 | (int64_t)r; };
    for (int c = tid; c < S; c += 1024) {
        const int64_t kc = key(s_row[c]);
        int rank = 0;
        for (int d = 0; d < S; ++d) rank += key(s_row[d]) < kc ? 1 : 0;
        P.as_ord[rank] = c;  // (rows are distinct: the ranks are a permutation)
    }
    if (tid < 65) {
        int off = 0;
        for (int d = 0; d < S; ++d) off += ((s_row[d] >> 1) & 63) < tid ? 1 : 0;
        P.as_off[tid] = off;
    }
    if (carry && min_nw > 0 && tid == 0 && P.bc_n[5] == 2) P.bc_n[5] = 1;
}
static void launch_as_rows(const Params& P, int min_nw, int carry, hipStream_t s) {
    if (!P.AS) return;
    hipLaunchKernelGGL(k_as_rows, dim3((unsigned)((P.n + 3) / 4)), dim3(256), 0, s, P, min_nw, carry);
    hipLaunchKernelGGL(k_as_order, dim3(1), dim3(1024), 0, s, P, min_nw, carry);
}

constexpr int BC_ROWS = 4;  // rows per k_bc_gather workgroup
__global__ __launch_bounds__(256) void k_bc_gather(Params P) {
    const int S = P.bc_n[0];
    const int64_t L = P.L, ldc = P.bc_n[1];
    double* const bc = bc_buf(P, P.bc_n[2]);
    for (int r = 0; r < BC_ROWS; ++r) {
        const int64_t i = (int64_t)blockIdx.x * BC_ROWS + r;
        if (i >= P.m) break;
        for (int c = threadIdx.x; c < S; c += 256) bc[i * ldc + c] = P.B0[i * L + P.rlist[c]];
    }
}
// the whole operand from the dense B_w (reset, reinversion, warm start; and
// after a dense fold, SPX_DENSE_FOLD=1)
hipError_t launch_compact(const Params& P, hipStream_t s) {
    if (!P.bc) return hipSuccess;
    hipLaunchKernelGGL(k_bc_list, dim3(1), dim3(1024), 0, s, P, 0, 0);
    launch_as_rows(P, 0, 0, s);
    hipLaunchKernelGGL(k_bc_gather, dim3((unsigned)((P.m + BC_ROWS - 1) / BC_ROWS)), dim3(256), 0, s, P);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Compact fold (Params::bc): the eta-window fold of k_fold
// restricted to B_w's non-unit columns.  A column of B_w outside the list is
// e_k and stays e_k (every r_t has an exact 0 there: B_w[q_t, k] = 0 for the
// unit column k != q_t, and the window's leaving rows q_t join the list
// first, k_bc_list), so only the m x S' listed entries change -- the dense
// fold rewrites all m x L of them.  Per 64-column group of the new list:
//   R: r_t = Qrows[t][k_c] + sum_{s<t} Urows[t][s] r_s (Qrows: the base rows
//      k_price staged), by one wave, one lane per column, the s terms of each
//      r_t in ascending order with the fold's zero coefficients -- the fma
//      sequence of fold_rebuild_R4, so the bits of k_fold's R;
//   tiles: the fold's MFMA tiles (fold_tile_take, v_mfma_f64_16x16x4f64, the
//      same K order), rows read from the active buffer at the old pitch
//      (columns the window added read as e_k), written to the other buffer
//      at the new pitch, and the same values scattered into the dense B_w at
//      (i, rlist[c]) -- so the dense B_w is k_fold's, entry for entry, and
//      the operand is what k_bc_gather would gather from it;
//   y_w += SY R over the group's columns, xw += U (R b) as k_fold.
// The last workgroup resets the window and flips the active buffer.  The
// grid is fixed (host-side, captured in graphs): workgroup b takes group
// b % ng and row range b / ng of the floor(grid / ng) ranges; the rest only
// count in.
// ---------------------------------------------------------------------------
template <int KW>
__device__ __forceinline__ void cfold_tile_issue(const double* Bo, int64_t ldo, int S0, const double* U, int64_t c0,
                                                 int64_t r0, int64_t i1, FoldTilePre<KW>& t) {
    const int lane = threadIdx.x & 63;
    const int kr = lane >> 4, cl = lane & 15;
    const int64_t ilast = i1 > 0 ? i1 - 1 : 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i0r = r0 + kr + 4 * r;
        const int64_t i = i0r < ilast ? i0r : ilast;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t c = c0 + 32 * h + 2 * cl;  // even; the pair lies inside the old pitch when c < S0
            t.b[r][h] = *reinterpret_cast<const fdbl2*>(&Bo[i * ldo + (c < S0 ? c : 0)]);
        }
    }
#pragma unroll
    for (int j = 0; j < KW / 8; ++j) {
        const int e = 128 * j + 2 * lane;
        const int64_t ia0 = r0 + e / KW;
        const int64_t ia = ia0 < ilast ? ia0 : ilast;
        t.u[j] = *reinterpret_cast<const fdbl2*>(&U[ia * KW + e % KW]);
    }
}
// the old entries of the tile's columns, or e_k for the columns past S0
// (rlv: rlist of this lane's four columns, -1 past S)
__device__ __forceinline__ double cfold_old(double v, int64_t i, int64_t c, int S0, int k) {
    return c < S0 ? v : (k == i ? 1.0 : 0.0);
}

template <int KW>
__global__ __launch_bounds__(FOLD_THREADS) void k_cfold(Params P, int min_nw) {
    static_assert(SPX_FOLD_ULDS, "the compact fold stages U through LDS");
    DevState* st = P.st;
    // (the list's shape read beside the window count: one round trip)
    const int nw = st->nw;
    const int S = P.bc_n[0], sel = P.bc_n[2], S0 = P.bc_n[3];
    const int64_t ldn = P.bc_n[1], ldo = P.bc_n[4] > 0 ? P.bc_n[4] : 64;
    asm volatile("" ::"s"(S), "s"(sel), "s"(S0), "s"(ldn), "s"(ldo));  // (kept ahead of the branch)
    if (nw < min_nw || nw < 2) return;
    const int nf = nw - 1;
    constexpr int KS = KW / 4;
    __shared__ double Rl[KW][FOLD_RP];
    __shared__ double NT[KW][FOLD_NP<KW>];
    __shared__ double Ush[FOLD_THREADS / 64][16][FOLD_UP<KW>];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kr = lane >> 4, cl = lane & 15;
    const int64_t L = P.L, m = P.m;
    const double* const Bo = bc_buf(P, sel);
    double* const Bn = bc_buf(P, sel ^ 1);
    const int ng = (int)(ldn / 64);
    const int nper = (int)gridDim.x / ng;  // row ranges per group
    const int g = (int)blockIdx.x % ng, yr = (int)blockIdx.x / ng;
    const bool work = yr < nper;
    unsigned long long* const fst =
        (P.stamps && tid == 0 && blockIdx.x < 1024) ? P.stamps + STAMP_FOLD + STAMP_FOLD_PER * (int64_t)blockIdx.x
                                                    : nullptr;
    // (lane 0 of every wave: the y / xw waves' own end stamps, slots 7 / 6)
    unsigned long long* const fsx =
        (P.stamps && lane == 0 && blockIdx.x < 1024) ? P.stamps + STAMP_FOLD + STAMP_FOLD_PER * (int64_t)blockIdx.x
                                                     : nullptr;
    if (fst) fst[0] = rtime();
    const int64_t c0 = (int64_t)g * 64;
    const int64_t per = ((m + nper - 1) / nper + 15) / 16 * 16;
    const int64_t i0 = work ? (int64_t)yr * per : m;
    const int64_t i1 = (i0 + per < m) ? i0 + per : m;
    if (work && i0 < m) {
        const int64_t cc = c0 + lane;
        // (the list entry of this lane's column, for y_w: read unconditionally
        // and pinned below, so the compiler cannot turn it into a guarded
        // load waited for on the spot)
        int kcl = P.rlist[cc < L ? cc : L - 1];
        // R, one lane per row t and eight columns per wave (columns
        // c0 + 8 wave + j): lane t holds N[t][s] = Urows[t][s] (0 unless
        // s < t < nf) and r_t of each column; step s hands r_s (final after
        // step s - 1) from lane s to the lanes t > s, which take
        // fma(N[t][s], r_s, r_t) -- every r_t its s terms in ascending s,
        // fold_rebuild_R4's fma sequence, so its bits
        constexpr int CPW = 64 / (FOLD_THREADS / 64);
        const int64_t cw0 = c0 + CPW * wave;
        const bool rows = cw0 < S;  // (wave-uniform) any listed column
        const int tl = lane < KW ? lane : KW - 1;
        double rt[CPW];
        // every operand read unconditionally (clamped): the coefficients
        // (staged transposed into LDS, NT[s][t] = N[t][s], as k_fold), the
        // list entries, then the base-row entries, which wait only for the
        // first two (vmcnt retires in issue order)
        FoldRPre<KW> rpre;
#pragma unroll
        for (int j = 0; j < FoldRPre<KW>::NPT; ++j) {
            const int k = tid + j * FOLD_THREADS;
            rpre.n[j] = P.Urows[k < KW * KW ? k : KW * KW - 1];
        }
        int kl[CPW];
#pragma unroll
        for (int j = 0; j < CPW; ++j) kl[j] = P.rlist[cw0 + j < L ? cw0 + j : L - 1];
#pragma unroll
        for (int j = 0; j < CPW; ++j) {
            const int k = (unsigned)kl[j] < (unsigned)L ? kl[j] : 0;
            rt[j] = P.Qrows[(int64_t)tl * L + k];
        }
        // the list entries of this lane's tile columns (unit entries past S0)
        int rk[4];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                const int64_t c = c0 + 32 * h + 2 * cl + x;
                rk[2 * h + x] = c < S ? P.rlist[c] : -1;
            }
        // the wave's first tile in flight during the rebuild
        const int64_t step = 16 * (int64_t)(FOLD_THREADS / 64);
        int64_t r0 = i0 + 16 * wave;
        FoldTilePre<KW> cur;
        // (unconditional: rows clamped into the range, a branch here made
        // the compiler wait for everything before the rebuild)
        cfold_tile_issue<KW>(Bo, ldo, S0, P.U, c0, r0, i1, cur);
        fold_stage_N_pre<KW>(rpre, nf, NT);
        lds_barrier();
        // (the pins: every read above is issued before anything waits)
#pragma unroll
        for (int j = 0; j < CPW; ++j) {
            asm volatile("" : "+v"(rt[j]));
            rt[j] = (lane < nf && cw0 + j < S) ? rt[j] : 0.0;
        }
        asm volatile("" : "+v"(kcl));
        if (fst) fst[1] = rtime();
        if (rows) {
#pragma unroll
            for (int s = 0; s < KW - 1; ++s) {
                const double co = NT[s][tl];
                // one exec mask per step for the wave's columns
                double rs[CPW];
#pragma unroll
                for (int j = 0; j < CPW; ++j) rs[j] = readlane_d(rt[j], s);
                if (lane > s) {
#pragma unroll
                    for (int j = 0; j < CPW; ++j) rt[j] = fma(co, rs[j], rt[j]);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < CPW; ++j) rt[j] = 0.0;
        }
        if (lane < KW) {
#pragma unroll
            for (int j = 0; j < CPW; ++j) Rl[lane][fold_slot(CPW * wave + j)] = rt[j];
        }
        lds_barrier();
        if (fst) fst[2] = rtime();
        // tiles (fold_tiles' k-step order), the first one already in flight
        double (*Us)[FOLD_UP<KW>] = Ush[wave];
        for (; r0 < i1; r0 += step) {
            dbl4 acc[4];
            double af[KS];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = r0 + kr + 4 * r;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int64_t c = c0 + 32 * h + 2 * cl;
                    cur.b[r][h].x = cfold_old(cur.b[r][h].x, i, c, S0, rk[2 * h]);
                    cur.b[r][h].y = cfold_old(cur.b[r][h].y, i, c + 1, S0, rk[2 * h + 1]);
                }
            }
            fold_tile_take<KW>(cur, r0, i1, nf, acc, af, Us);
            if (r0 + step < i1) cfold_tile_issue<KW>(Bo, ldo, S0, P.U, c0, r0 + step, i1, cur);
            double rf[2][4];
            double uf[2];
            uf[0] = Us[cl][kr];
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) rf[0][jb] = Rl[kr][16 * jb + cl];
#pragma unroll
            for (int s2 = 0; s2 < KS; ++s2) {
                if (s2 + 1 < KS) {
                    uf[(s2 + 1) & 1] = Us[cl][4 * (s2 + 1) + kr];
#pragma unroll
                    for (int jb = 0; jb < 4; ++jb) rf[(s2 + 1) & 1][jb] = Rl[4 * (s2 + 1) + kr][16 * jb + cl];
                }
                const double a = uf[s2 & 1];
#pragma unroll
                for (int jb = 0; jb < 4; ++jb)
                    acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, rf[s2 & 1][jb], acc[jb], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            // the new operand rows (whole pitch: zeros past S) and the dense B_w
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = r0 + kr + 4 * r;
                if (i < i1) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        fdbl2 v;
                        v.x = acc[2 * h][r];
                        v.y = acc[2 * h + 1][r];
                        *reinterpret_cast<fdbl2*>(&Bn[i * ldn + c0 + 32 * h + 2 * cl]) = v;
                        if (rk[2 * h] >= 0) P.B0[i * L + rk[2 * h]] = v.x;
                        if (rk[2 * h + 1] >= 0) P.B0[i * L + rk[2 * h + 1]] = v.y;
                    }
                }
            }
        }
        if (fst) fst[3] = rtime();
        if (wave == 0 && yr == 0) {
            // y_w += SY R for the group's columns (k_fold's sum, t ascending;
            // the terms past nf dropped by a select). SY[t] is read once by
            // lane t and handed on by readlane, so it is read before the
            // column guard: every lane must hold its entry.
            double syl = P.SY[lane < KW ? lane : KW - 1];
            asm volatile("" : "+v"(syl));  // (so the read cannot sink under the guard)
            if (cc < S) {
                double* y = st->y_buf ? P.y1 : P.y0;
                const int sl = fold_slot(lane);
                double d = 0.0;
#pragma unroll
                for (int t = 0; t < KW; ++t) {
                    const double v = fma(readlane_d(syl, t), Rl[t][sl], d);
                    d = t < nf ? v : d;
                }
                y[kcl] += d;
                if (fsx) fsx[7] = rtime();
            }
        }
    }
    if (wave == FOLD_THREADS / 64 - 1) {
        // xw += U (R b), R b = Wt[n][0..nf): the rows spread over every
        // workgroup, one lane per row, t ascending (k_fold's); the last
        // wave, which has tiles only when a range passes 112 rows
        // (R b: lane t holds entry t, handed to every row by readlane)
        double wbl = P.Wt[P.n * KW + (lane < KW ? lane : KW - 1)];
        asm volatile("" : "+v"(wbl));  // (read by every lane, not sunk into the row loop)
        const int64_t nwg = (int64_t)gridDim.x;
        const int64_t rpw = (m + nwg - 1) / nwg;
        const int64_t r0 = (int64_t)blockIdx.x * rpw;
        const int64_t r1 = (r0 + rpw < m) ? r0 + rpw : m;
        for (int64_t i = r0 + lane; i < r1; i += 64) {
            double u[KW];
#pragma unroll
            for (int t2 = 0; t2 < KW / 2; ++t2) {
                const fdbl2 v = *reinterpret_cast<const fdbl2*>(&P.U[i * KW + 2 * t2]);
                u[2 * t2] = v.x;
                u[2 * t2 + 1] = v.y;
            }
            double d = 0.0;
#pragma unroll
            for (int t = 0; t < KW; ++t) {
                const double v = fma(u[t], readlane_d(wbl, t), d);
                d = t < nf ? v : d;
            }
            P.xw[i] += d;
        }
        if (fsx) fsx[6] = rtime();
    }
    __syncthreads();
    if (fst) fst[4] = rtime();
    if (tid == 0) s_last = arrive_last(arrive_group(P.arrive, ARR_FOLD), gridDim.x, blockIdx.x);
    __syncthreads();
    if (fst) fst[5] = rtime();
    if (s_last && tid == 0) {
        P.SY[0] = P.SY[nf];
        P.bc_n[2] = sel ^ 1;
        st->nw = 1;
    }
}

// compact fold: k_bc_list (the window's leaving rows join the list) then
// k_cfold over the listed columns only (P.bc, one workgroup per CU); carry:
// dw follows y_w across the fold (k_as_rows)
hipError_t launch_cfold(const Params& P, int min_nw, int cus, hipStream_t s, bool carry) {
    const int cy = (carry && P.AS) ? 1 : 0;
    hipLaunchKernelGGL(k_bc_list, dim3(1), dim3(1024), 0, s, P, min_nw, cy);
    launch_as_rows(P, min_nw, cy, s);
    // every column group of the list needs a workgroup (m > 16,384: more
    // groups than CUs)
    const int64_t ngmax = P.L / 64;
    const int64_t nc = cus > 0 ? cus : 256;
    const dim3 grid((unsigned)(nc > ngmax ? nc : ngmax));
    switch (P.win) {
        case 8: hipLaunchKernelGGL(k_cfold<8>, grid, dim3(FOLD_THREADS), 0, s, P, min_nw); break;
        case 16: hipLaunchKernelGGL(k_cfold<16>, grid, dim3(FOLD_THREADS), 0, s, P, min_nw); break;
        case 32: hipLaunchKernelGGL(k_cfold<32>, grid, dim3(FOLD_THREADS), 0, s, P, min_nw); break;
        case 64: hipLaunchKernelGGL(k_cfold<64>, grid, dim3(FOLD_THREADS), 0, s, P, min_nw); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_fold(const Params& P, int min_nw, int cus, hipStream_t s, bool carry) {
    if (P.bc && P.cfold) return launch_cfold(P, min_nw, cus, s, carry);  // the listed columns only
    if (P.tab) {  // T_w and dw first: k_fold resets the window
        const hipError_t e = launch_tab_fold(P, min_nw, cus, s);
        if (e != hipSuccess) return e;
        // A[:, n-m:] = I: B_w is T_w's slack block and the tableau fold has
        // updated y_w and xw too (and reset the window); B_w itself is rebuilt
        // from T_w only for readbacks (launch_tab_binv)
        if (P.tab_slack) return hipSuccess;
    }
    const int nx = (int)(P.L / 64);
    const dim3 grid((unsigned)nx, (unsigned)fold_grid_y(P.m, nx, cus));
    switch (P.win) {
        case 8: hipLaunchKernelGGL(k_fold<8>, grid, dim3(FOLD_THREADS), 0, s, P, min_nw); break;
        case 16: hipLaunchKernelGGL(k_fold<16>, grid, dim3(FOLD_THREADS), 0, s, P, min_nw); break;
        case 32: hipLaunchKernelGGL(k_fold<32>, grid, dim3(FOLD_THREADS), 0, s, P, min_nw); break;
        case 64: hipLaunchKernelGGL(k_fold<64>, grid, dim3(FOLD_THREADS), 0, s, P, min_nw); break;
        default: return hipErrorInvalidValue;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_compact(P, s);  // the compact FTRAN operand follows B_w
}

}  // namespace spx
