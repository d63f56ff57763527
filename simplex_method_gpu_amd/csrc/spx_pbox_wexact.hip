// spx_pbox_wexact.hip — gfx950 kernels that form the exact steepest-edge weights
// of a warm basis for the bounded primal simplex loop (spx_pbox.h).
// Not on the per-iteration loop: they run where the weights restart for a warm
// basis under SPX_PRIMAL_WEIGHTS_EXACT, and on spx_refresh_primal_weights.
// Deterministic: fixed tiling from m and n alone, fixed summation orders, no
// floating-point atomics.
#include "spx_pbox.h"

#include "spx_common.h"

namespace spx {

namespace {

typedef double dbl4 __attribute__((ext_vector_type(4)));

constexpr int WX_OPER = PBOX_WX_TILE * PBOX_WX_LD;  // doubles of one staged operand (128 rows x 16 k, padded)
constexpr int WX_STAGE = 2 * WX_OPER;               // S rows, then A columns
constexpr size_t WX_LDS = 2 * WX_STAGE * sizeof(double);
constexpr int WX_LOADS = PBOX_WX_TILE * PBOX_WX_KC / 2 / PBOX_WX_BLOCK;  // dbl2 per thread, operand and chunk
// Workgroups per CU the product kernel is compiled for (compile-time, for A/B builds).  2: at most 256
// registers, accumulators in VGPRs, two waves per SIMD and two workgroups' LDS (2 x 74 KB) per CU; 1: 219
// VGPRs + 128 AGPRs, one wave per SIMD.  Measured at 4096 x 16384: 9.3 ms against 16.1 ms.
#ifndef SPX_WX_WGS_PER_CU
#define SPX_WX_WGS_PER_CU 2
#endif
static_assert(WX_LOADS == 4 && PBOX_WX_BLOCK == 256 && PBOX_WX_KC == 16, "the load map below is written for these");

// the dbl2 at k, k + 1 of a row (nullptr: zeros), entries at k >= m as zeros
__device__ __forceinline__ dbl2 wx_load(const double* row, int64_t k, int64_t m) {
    if (!row || k >= m) return dbl2{0.0, 0.0};
    dbl2 v = *reinterpret_cast<const dbl2*>(row + k);
    if (k + 1 >= m) v.y = 0.0;
    return v;
}

}  // namespace

__global__ __launch_bounds__(PBOX_WX_BLOCK, SPX_WX_WGS_PER_CU) void k_pbox_wexact(Params P, PboxWexactArgs W) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wx_dsm[];
    __shared__ double s_half[2][PBOX_WX_TILE];
    double* lds = reinterpret_cast<double*>(wx_dsm);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cl = lane & 15, kr = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;  // the wave's 64 x 64 quadrant
    const int64_t m = P.m, L = P.L;
    int64_t cnt = P.st->nb_count;
    if (cnt > W.cap) cnt = W.cap;
    const int64_t row0 = (int64_t)blockIdx.x * PBOX_WX_TILE;
    const int64_t slot0 = (int64_t)blockIdx.y * PBOX_WX_TILE;

    // load map: thread t stages the dbl2 at k = 2 (t & 7) of rows (t >> 3) + 32 u of either operand
    const int lk = 2 * (tid & 7), lr = tid >> 3;
    const double* srow[WX_LOADS];
    const double* acol[WX_LOADS];
#pragma unroll
    for (int u = 0; u < WX_LOADS; ++u) {
        const int64_t i = row0 + lr + 32 * u;
        srow[u] = i < m ? W.S + i * L : nullptr;
        const int64_t s = slot0 + lr + 32 * u;
        acol[u] = nullptr;
        if (s < cnt) {
            const int64_t j = P.nb_list[s];
            if (!(P.slack_unit && j >= P.ns)) acol[u] = P.A + j * L;  // (a unit slack: k_pbox_wexact_slack)
        }
    }

    dbl4 acc[4][4];
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) acc[it][jt] = dbl4{0.0, 0.0, 0.0, 0.0};

    dbl2 sv[WX_LOADS], av[WX_LOADS];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int u = 0; u < WX_LOADS; ++u) {
            sv[u] = wx_load(srow[u], k0 + lk, m);
            av[u] = wx_load(acol[u], k0 + lk, m);
        }
    };
    auto stage = [&](int buf) {
        double* d = lds + buf * WX_STAGE;
#pragma unroll
        for (int u = 0; u < WX_LOADS; ++u) {
            *reinterpret_cast<dbl2*>(d + (lr + 32 * u) * PBOX_WX_LD + lk) = sv[u];
            *reinterpret_cast<dbl2*>(d + WX_OPER + (lr + 32 * u) * PBOX_WX_LD + lk) = av[u];
        }
    };

    const int nchunk = (int)((m + PBOX_WX_KC - 1) / PBOX_WX_KC);
    fetch(0);
    stage(0);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        if (c + 1 < nchunk) fetch((int64_t)(c + 1) * PBOX_WX_KC);  // in flight during this chunk's MFMAs
        const double* ds = lds + (c & 1) * WX_STAGE + (wr * 64 + cl) * PBOX_WX_LD + kr;
        const double* da = lds + (c & 1) * WX_STAGE + WX_OPER + (wc * 64 + cl) * PBOX_WX_LD + kr;
#pragma unroll
        for (int s = 0; s < PBOX_WX_KC / 4; ++s) {
            double a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                a[t] = ds[16 * t * PBOX_WX_LD + 4 * s];
                b[t] = da[16 * t * PBOX_WX_LD + 4 * s];
            }
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int jt = 0; jt < 4; ++jt)
                    acc[it][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[it], b[jt], acc[it][jt], 0, 0, 0);
        }
        if (c + 1 < nchunk) stage((c + 1) & 1);
        __syncthreads();
    }

    // column norms over the wave's 64 rows: tile, register, then the four row groups (lane >> 4)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        double q = 0.0;
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int r = 0; r < 4; ++r) q = fma(acc[it][jt][r], acc[it][jt][r], q);
        q += __shfl_xor(q, 16, 64);
        q += __shfl_xor(q, 32, 64);
        if (kr == 0) s_half[wr][wc * 64 + 16 * jt + cl] = q;
    }
    __syncthreads();
    if (tid < PBOX_WX_TILE && slot0 + tid < cnt)
        W.parts[(int64_t)blockIdx.x * W.cap + slot0 + tid] = s_half[0][tid] + s_half[1][tid];
}

// column k of S squared and summed over the rows of row block blockIdx.y, rows ascending
__global__ __launch_bounds__(PBOX_WX_BLOCK) void k_pbox_wexact_slack(Params P, PboxWexactArgs W) {
    const int64_t m = P.m, L = P.L;
    const int64_t k = (int64_t)blockIdx.x * PBOX_WX_BLOCK + threadIdx.x;
    if (k >= m) return;
    const int64_t i0 = (int64_t)blockIdx.y * PBOX_WX_TILE;
    const int64_t i1 = i0 + PBOX_WX_TILE < m ? i0 + PBOX_WX_TILE : m;
    const double* p = W.S + i0 * L + k;
    double q = 0.0;
    int64_t i = i0;
    for (; i + 4 <= i1; i += 4, p += 4 * L) {
        const double v0 = p[0], v1 = p[L], v2 = p[2 * L], v3 = p[3 * L];
        q = fma(v0, v0, q);
        q = fma(v1, v1, q);
        q = fma(v2, v2, q);
        q = fma(v3, v3, q);
    }
    for (; i < i1; ++i, p += L) q = fma(p[0], p[0], q);
    W.sparts[(int64_t)blockIdx.y * L + k] = q;
}

// gamma_j = 1 + the row blocks' partials, ascending
__global__ __launch_bounds__(PBOX_WX_BLOCK) void k_pbox_wexact_sum(Params P, PboxWexactArgs W) {
    int64_t cnt = P.st->nb_count;
    if (cnt > W.cap) cnt = W.cap;
    const int64_t s = (int64_t)blockIdx.x * PBOX_WX_BLOCK + threadIdx.x;
    if (s >= cnt) return;
    const int64_t j = P.nb_list[s];
    const bool unit = P.slack_unit && j >= P.ns;
    const double* src = unit ? W.sparts + (j - P.ns) : W.parts + s;
    const int64_t pitch = unit ? P.L : W.cap;
    double g = 0.0;
    for (int rb = 0; rb < W.row_blocks; ++rb) g += src[rb * pitch];
    W.gamma[j] = 1.0 + g;
}

hipError_t pbox_wexact_prepare() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_pbox_wexact), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)WX_LDS);
}

hipError_t launch_pbox_wexact(const Params& P, const PboxWexactArgs& W, const PboxWexactCfg& c, hipStream_t s) {
    if (c.col_tiles > 65535 || c.row_blocks > 65535) return hipErrorInvalidValue;  // (the grid's y extent)
    if (c.col_tiles > 0 && c.row_blocks > 0)
        hipLaunchKernelGGL(k_pbox_wexact, dim3(c.row_blocks, c.col_tiles), dim3(PBOX_WX_BLOCK), WX_LDS, s, P, W);
    if (P.slack_unit && c.slack_grid > 0)
        hipLaunchKernelGGL(k_pbox_wexact_slack, dim3(c.slack_grid, c.row_blocks), dim3(PBOX_WX_BLOCK), 0, s, P, W);
    if (c.sum_grid > 0) hipLaunchKernelGGL(k_pbox_wexact_sum, dim3(c.sum_grid), dim3(PBOX_WX_BLOCK), 0, s, P, W);
    return hipGetLastError();
}

}  // namespace spx
