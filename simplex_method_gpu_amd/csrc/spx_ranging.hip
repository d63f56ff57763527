// spx_ranging.hip — gfx950 kernels of sensitivity ranging at the optimum
// (spx_ranging.h).  Off every loop: they run when the caller asks
// for cost or right-hand-side ranges.  Deterministic: fixed tiling from m and n
// alone, every reduction a minimum under (value, index), no atomics.
#include "spx_ranging.h"

#include "spx_common.h"

namespace spx {

namespace {

typedef double dbl4 __attribute__((ext_vector_type(4)));

constexpr int RG_OPER = RNG_TILE * RNG_LD;  // doubles of one staged operand (128 rows x 16 k, padded)
constexpr int RG_STAGE = 2 * RG_OPER;       // S rows, then A columns
constexpr size_t RG_LDS = 2 * RG_STAGE * sizeof(double);
constexpr int RG_LOADS = RNG_TILE * RNG_KC / 2 / RNG_BLOCK;  // dbl2 per thread, operand and chunk
// Workgroups per CU k_rng_cost is compiled for: 2 keeps the accumulators in VGPRs under the 256-register cap
// (k_pbox_wexact lost 1.77 x at one workgroup per CU)
#ifndef SPX_RNG_WGS_PER_CU
#define SPX_RNG_WGS_PER_CU 2
#endif
static_assert(RG_LOADS == 4 && RNG_BLOCK == 256 && RNG_KC == 16, "the load map below is written for these");
constexpr int RG_AHEAD = 8;  // rows of k_rng_rhs's walk whose loads are issued together
static_assert(RNG_ROWS % RG_AHEAD == 0, "k_rng_rhs indexes its staged rows by chunk");
constexpr int RG_NONE = 0x7fffffff;  // "no column" inside k_rng_cost (the partials carry INT64_MAX)

// the epilogue's per-row records of the two column halves, in the staging buffers once the K loop is done
struct alignas(8) RgHalf {
    double down, up;
    int32_t kdown, kup;
};
static_assert(2 * RNG_TILE * sizeof(RgHalf) <= RG_LDS, "the half records reuse the staging buffers");

// the dbl2 at k, k + 1 of a row (nullptr: zeros), entries at k >= m as zeros
__device__ __forceinline__ dbl2 rg_load(const double* row, int64_t k, int64_t m) {
    if (!row || k >= m) return dbl2{0.0, 0.0};
    dbl2 v = *reinterpret_cast<const dbl2*>(row + k);
    if (k + 1 >= m) v.y = 0.0;
    return v;
}

// (v, j) replaces (bv, bj) when smaller, the smaller index on equal values
__device__ __forceinline__ void rg_min(double v, int32_t j, double& bv, int32_t& bj) {
    if (v < bv || (v == bv && j < bj)) {
        bv = v;
        bj = j;
    }
}

__device__ __forceinline__ void rg_min64(double v, int64_t j, double& bv, int64_t& bj) {
    if (v < bv || (v == bv && j < bj)) {
        bv = v;
        bj = j;
    }
}

}  // namespace

// per list slot: sigma, s and the column; the non-basic column's own cost range
__global__ __launch_bounds__(RNG_BLOCK) void k_rng_gather(Params P, RngArgs R) {
    int64_t cnt = P.st->nb_count;
    if (cnt > R.cap) cnt = R.cap;
    const int64_t s = (int64_t)blockIdx.x * RNG_BLOCK + threadIdx.x;
    if (s >= cnt) return;
    const int32_t j = P.nb_list[s];
    const bool fr = R.is_free && R.is_free[j];
    const bool up = !fr && R.at_upper && R.at_upper[j];
    const double sg = fr ? 0.0 : (up ? -1.0 : 1.0);
    const double sd = sg * R.d[j];
    const double sk = sd > 0.0 ? sd : 0.0;  // (free: 0)
    R.sk[s] = sk;
    R.sig[s] = sg;
    R.col[s] = j;
    R.c_down[j] = fr ? 0.0 : (up ? sk : INFINITY);
    R.c_up[j] = fr ? 0.0 : (up ? INFINITY : sk);
    R.c_kdown[j] = (fr || up) ? j : -1;
    R.c_kup[j] = (fr || !up) ? j : -1;
}

__global__ __launch_bounds__(RNG_BLOCK, SPX_RNG_WGS_PER_CU) void k_rng_cost(Params P, RngArgs R) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rg_dsm[];
    double* lds = reinterpret_cast<double*>(rg_dsm);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cl = lane & 15, kr = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;  // the wave's 64 x 64 quadrant
    const int64_t m = P.m, L = P.L;
    int64_t cnt = P.st->nb_count;
    if (cnt > R.cap) cnt = R.cap;
    const int64_t row0 = (int64_t)blockIdx.x * RNG_TILE;
    const int64_t slot0 = (int64_t)blockIdx.y * RNG_TILE;

    // load map: thread t stages the dbl2 at k = 2 (t & 7) of rows (t >> 3) + 32 u of either operand
    const int lk = 2 * (tid & 7), lr = tid >> 3;
    const double* srow[RG_LOADS];
    const double* acol[RG_LOADS];
#pragma unroll
    for (int u = 0; u < RG_LOADS; ++u) {
        const int64_t i = row0 + lr + 32 * u;
        srow[u] = i < m ? R.S + i * L : nullptr;
        const int64_t s = slot0 + lr + 32 * u;
        acol[u] = s < cnt ? P.A + (int64_t)P.nb_list[s] * L : nullptr;  // (a slack's unit column too)
    }

    dbl4 acc[4][4];
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) acc[it][jt] = dbl4{0.0, 0.0, 0.0, 0.0};

    dbl2 sv[RG_LOADS], av[RG_LOADS];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int u = 0; u < RG_LOADS; ++u) {
            sv[u] = rg_load(srow[u], k0 + lk, m);
            av[u] = rg_load(acol[u], k0 + lk, m);
        }
    };
    auto stage = [&](int buf) {
        double* d = lds + buf * RG_STAGE;
#pragma unroll
        for (int u = 0; u < RG_LOADS; ++u) {
            *reinterpret_cast<dbl2*>(d + (lr + 32 * u) * RNG_LD + lk) = sv[u];
            *reinterpret_cast<dbl2*>(d + RG_OPER + (lr + 32 * u) * RNG_LD + lk) = av[u];
        }
    };

    const int nchunk = (int)((m + RNG_KC - 1) / RNG_KC);
    fetch(0);
    stage(0);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        if (c + 1 < nchunk) fetch((int64_t)(c + 1) * RNG_KC);  // in flight during this chunk's MFMAs
        const double* ds = lds + (c & 1) * RG_STAGE + (wr * 64 + cl) * RNG_LD + kr;
        const double* da = lds + (c & 1) * RG_STAGE + RG_OPER + (wc * 64 + cl) * RNG_LD + kr;
#pragma unroll
        for (int s = 0; s < RNG_KC / 4; ++s) {
            double a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                a[t] = ds[16 * t * RNG_LD + 4 * s];
                b[t] = da[16 * t * RNG_LD + 4 * s];
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

    // Epilogue.  acc[it][jt][r] is T at row wr 64 + 16 it + 4 r + kr and slot wc 64 + 16 jt + cl of the tile
    // (the f64 accumulator layout: column = lane & 15, row = (lane >> 4) + 4 r).  The slots' s, sigma, column:
    double ssk[4], ssg[4];
    int32_t scol[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        const int64_t s = slot0 + wc * 64 + 16 * jt + cl;
        const bool live = s < cnt;  // (a slot past the list has T = 0: never a candidate)
        ssk[jt] = live ? R.sk[s] : 0.0;
        ssg[jt] = live ? R.sig[s] : 1.0;
        scol[jt] = live ? R.col[s] : RG_NONE;
    }
    const double tol = R.tol;
    RgHalf* half = reinterpret_cast<RgHalf*>(rg_dsm);  // [2][RNG_TILE]; every wave is past the K loop's last barrier
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double dn = INFINITY, up = INFINITY;
            int32_t kdn = RG_NONE, kup = RG_NONE;
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {  // the lane's four columns, ascending tiles
                const double t = acc[it][jt][r];
                const bool fr = ssg[jt] == 0.0;
                const double g = fr ? t : ssg[jt] * t;
                const double a = fabs(g);
                if (a > tol) {
                    const double q = ssk[jt] / a;
                    if (fr || g < 0.0) rg_min(q, scol[jt], up, kup);
                    if (fr || g > 0.0) rg_min(q, scol[jt], dn, kdn);
                }
            }
#pragma unroll
            for (int x = 1; x < 16; x <<= 1) {  // the 16 lanes that hold the row: xor 1, 2, 4, 8
                const double odn = __shfl_xor(dn, x, 64), oup = __shfl_xor(up, x, 64);
                const int32_t okdn = __shfl_xor(kdn, x, 64), okup = __shfl_xor(kup, x, 64);
                rg_min(odn, okdn, dn, kdn);
                rg_min(oup, okup, up, kup);
            }
            if (cl == 0) half[wc * RNG_TILE + wr * 64 + 16 * it + 4 * r + kr] = RgHalf{dn, up, kdn, kup};
        }
    __syncthreads();
    if (tid < RNG_TILE && row0 + tid < m) {  // the two column halves, then one partial per (column tile, row)
        RgHalf h = half[tid];
        const RgHalf o = half[RNG_TILE + tid];
        rg_min(o.down, o.kdown, h.down, h.kdown);
        rg_min(o.up, o.kup, h.up, h.kup);
        RngPart p;
        p.down = h.down;
        p.up = h.up;
        p.kdown = h.kdown == RG_NONE ? INT64_MAX : (int64_t)h.kdown;
        p.kup = h.kup == RG_NONE ? INT64_MAX : (int64_t)h.kup;
        R.cparts[(int64_t)blockIdx.y * m + row0 + tid] = p;
    }
}

// row i's partials over the column tiles merged by key; scattered to the row's basic column
__global__ __launch_bounds__(RNG_BLOCK) void k_rng_cost_min(Params P, RngArgs R) {
    const int64_t m = P.m;
    const int64_t i = (int64_t)blockIdx.x * RNG_BLOCK + threadIdx.x;
    if (i >= m) return;
    double dn = INFINITY, up = INFINITY;
    int64_t kdn = INT64_MAX, kup = INT64_MAX;
    for (int ct = 0; ct < R.col_tiles; ++ct) {
        const RngPart p = R.cparts[(int64_t)ct * m + i];
        rg_min64(p.down, p.kdown, dn, kdn);
        rg_min64(p.up, p.kup, up, kup);
    }
    const int64_t j = P.b_ixs[i];
    R.c_down[j] = dn;
    R.c_up[j] = up;
    R.c_kdown[j] = kdn == INT64_MAX ? -1 : kdn;
    R.c_kup[j] = kup == INT64_MAX ? -1 : kup;
}

// column r of S against x_b and ub_B over the rows of row block blockIdx.y, rows ascending
__global__ __launch_bounds__(RNG_BLOCK) void k_rng_rhs(Params P, RngArgs R) {
    __shared__ double s_x[RNG_ROWS], s_u[RNG_ROWS];
    __shared__ int32_t s_fr[RNG_ROWS];
    const int64_t m = P.m, L = P.L;
    const int64_t i0 = (int64_t)blockIdx.y * RNG_ROWS;
    const int rows = (int)(i0 + RNG_ROWS < m ? RNG_ROWS : m - i0);
    if (threadIdx.x < RNG_ROWS) {
        const int64_t i = i0 + threadIdx.x;
        double xv = 0.0, uv = INFINITY;
        int32_t fr = 1;
        if (i < m) {
            uv = R.ub_B ? R.ub_B[i] : INFINITY;
            xv = P.x_b[i];
            xv = xv > 0.0 ? xv : 0.0;  // clamped into [0, ub_B]
            xv = xv < uv ? xv : uv;
            fr = R.is_free ? (int32_t)R.is_free[P.b_ixs[i]] : 0;
        }
        s_x[threadIdx.x] = xv;
        s_u[threadIdx.x] = uv;
        s_fr[threadIdx.x] = fr;
    }
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * RNG_BLOCK + threadIdx.x;
    if (r >= m) return;
    const double tol = R.tol;
    const double* p = R.S + i0 * L + r;
    double dn = INFINITY, up = INFINITY;
    int64_t kdn = INT64_MAX, kup = INT64_MAX;
    // RG_AHEAD rows' loads in flight before the first is used: with one load per trip the walk was a chain of 64
    // load latencies (35 us at m = 1024 against k_pbox_wexact_slack's 12.5).  A row past the block
    // reads as 0 without a load, and 0 is never a candidate.
    for (int i8 = 0; i8 < rows; i8 += RG_AHEAD) {
        double v[RG_AHEAD];
#pragma unroll
        for (int u = 0; u < RG_AHEAD; ++u) v[u] = i8 + u < rows ? p[(int64_t)(i8 + u) * L] : 0.0;
#pragma unroll
        for (int u = 0; u < RG_AHEAD; ++u) {
            const int ii = i8 + u;  // (< RNG_ROWS: rows <= RNG_ROWS, a multiple of RG_AHEAD)
            const double beta = v[u];
            const double a = fabs(beta);
            if (s_fr[ii] || !(a > tol)) continue;
            const double xv = s_x[ii], uv = s_u[ii];
            const int64_t key = 2 * (i0 + ii);
            const double lo = xv / a;  // to the lower bound (side 0)
            if (beta > 0.0) rg_min64(lo, key, dn, kdn);
            else rg_min64(lo, key, up, kup);
            if (uv < INFINITY) {  // to the upper bound (side 1)
                const double hi = (uv - xv) / a;
                if (beta > 0.0) rg_min64(hi, key + 1, up, kup);
                else rg_min64(hi, key + 1, dn, kdn);
            }
        }
    }
    R.rparts[(int64_t)blockIdx.y * m + r] = RngPart{dn, up, kdn, kup};
}

// right-hand side r: the row blocks' partials merged by key
__global__ __launch_bounds__(RNG_BLOCK) void k_rng_rhs_min(Params P, RngArgs R) {
    const int64_t m = P.m;
    const int64_t r = (int64_t)blockIdx.x * RNG_BLOCK + threadIdx.x;
    if (r >= m) return;
    double dn = INFINITY, up = INFINITY;
    int64_t kdn = INT64_MAX, kup = INT64_MAX;
    for (int rb = 0; rb < R.rhs_blocks; ++rb) {
        const RngPart p = R.rparts[(int64_t)rb * m + r];
        rg_min64(p.down, p.kdown, dn, kdn);
        rg_min64(p.up, p.kup, up, kup);
    }
    R.r_down[r] = dn;
    R.r_up[r] = up;
    R.r_kdown[r] = kdn == INT64_MAX ? -1 : kdn;
    R.r_kup[r] = kup == INT64_MAX ? -1 : kup;
}

hipError_t rng_prepare() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_rng_cost), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)RG_LDS);
}

hipError_t launch_rng_cost(const Params& P, const RngArgs& R, const RngCfg& c, hipStream_t s) {
    if (c.col_tiles > 65535 || c.row_blocks > 65535) return hipErrorInvalidValue;  // (the grid's y extent)
    if (c.gather_grid > 0) hipLaunchKernelGGL(k_rng_gather, dim3(c.gather_grid), dim3(RNG_BLOCK), 0, s, P, R);
    if (c.col_tiles > 0 && c.row_blocks > 0)
        hipLaunchKernelGGL(k_rng_cost, dim3(c.row_blocks, c.col_tiles), dim3(RNG_BLOCK), RG_LDS, s, P, R);
    if (c.min_grid > 0) hipLaunchKernelGGL(k_rng_cost_min, dim3(c.min_grid), dim3(RNG_BLOCK), 0, s, P, R);
    return hipGetLastError();
}

hipError_t launch_rng_rhs(const Params& P, const RngArgs& R, const RngCfg& c, hipStream_t s) {
    if (c.rhs_blocks > 65535) return hipErrorInvalidValue;
    if (c.rhs_grid_x > 0 && c.rhs_blocks > 0) {
        hipLaunchKernelGGL(k_rng_rhs, dim3(c.rhs_grid_x, c.rhs_blocks), dim3(RNG_BLOCK), 0, s, P, R);
        hipLaunchKernelGGL(k_rng_rhs_min, dim3(c.min_grid), dim3(RNG_BLOCK), 0, s, P, R);
    }
    return hipGetLastError();
}

}  // namespace spx
