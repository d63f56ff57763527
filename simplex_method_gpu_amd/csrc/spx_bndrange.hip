// spx_bndrange.hip — gfx950 kernels of bound ranging at the optimum
// (spx_bndrange.h).  Off every loop: they run when the caller asks
// for bound ranges.  Deterministic: fixed tiling from m and n alone, every
// reduction a minimum under (value, 2 row + side), no atomics.
#include "spx_bndrange.h"

#include "spx_common.h"

namespace spx {

namespace {

typedef double dbl4 __attribute__((ext_vector_type(4)));

constexpr int BD_OPER = RNG_TILE * RNG_LD;  // doubles of one staged operand (128 rows x 16 k, padded)
constexpr int BD_STAGE = 2 * BD_OPER;       // S rows, then A columns
constexpr size_t BD_LDS = 2 * BD_STAGE * sizeof(double);
constexpr int BD_LOADS = RNG_TILE * RNG_KC / 2 / RNG_BLOCK;  // dbl2 per thread, operand and chunk
// Workgroups per CU k_rng_bound is compiled for: 2, as k_rng_cost (spx_ranging.hip)
#ifndef SPX_BND_WGS_PER_CU
#define SPX_BND_WGS_PER_CU 2
#endif
static_assert(BD_LOADS == 4 && RNG_BLOCK == 256 && RNG_KC == 16, "the load map below is written for these");
constexpr int BD_NONE = 0x7fffffff;  // "no row" inside k_rng_bound (the partials carry INT64_MAX)

// the epilogue's per-slot records of the two row halves, in the staging buffers once the K loop is done, behind
// the staged rows: x (RNG_TILE doubles), ub_B (RNG_TILE doubles), free (RNG_TILE int32 in RNG_TILE doubles' room)
struct alignas(8) BdHalf {
    double down, up;
    int32_t kdown, kup;
};
constexpr int BD_ROWS_DBL = 3 * RNG_TILE;  // doubles the staged rows take, rounded up
static_assert(BD_ROWS_DBL * sizeof(double) + 2 * RNG_TILE * sizeof(BdHalf) <= BD_LDS,
              "the staged rows and the half records reuse the staging buffers");

// the dbl2 at k, k + 1 of a row (nullptr: zeros), entries at k >= m as zeros
__device__ __forceinline__ dbl2 bd_load(const double* row, int64_t k, int64_t m) {
    if (!row || k >= m) return dbl2{0.0, 0.0};
    dbl2 v = *reinterpret_cast<const dbl2*>(row + k);
    if (k + 1 >= m) v.y = 0.0;
    return v;
}

// (v, j) replaces (bv, bj) when smaller, the smaller key on equal values
__device__ __forceinline__ void bd_min(double v, int32_t j, double& bv, int32_t& bj) {
    if (v < bv || (v == bv && j < bj)) {
        bv = v;
        bj = j;
    }
}

__device__ __forceinline__ void bd_min64(double v, int64_t j, double& bv, int64_t& bj) {
    if (v < bv || (v == bv && j < bj)) {
        bv = v;
        bj = j;
    }
}

}  // namespace

// per list slot: the column, where it sits, its range
__global__ __launch_bounds__(RNG_BLOCK) void k_rng_bound_gather(Params P, BndArgs B) {
    int64_t cnt = P.st->nb_count;
    if (cnt > B.cap) cnt = B.cap;
    const int64_t s = (int64_t)blockIdx.x * RNG_BLOCK + threadIdx.x;
    if (s >= cnt) return;
    const int32_t j = P.nb_list[s];
    const bool fr = B.is_free && B.is_free[j];
    const bool up = !fr && B.at_upper && B.at_upper[j];
    B.col[s] = j;
    B.kind[s] = fr ? 2 : (up ? 1 : 0);
    B.ubj[s] = B.ub ? B.ub[j] : INFINITY;
}

__global__ __launch_bounds__(RNG_BLOCK, SPX_BND_WGS_PER_CU) void k_rng_bound(Params P, BndArgs B) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bd_dsm[];
    double* lds = reinterpret_cast<double*>(bd_dsm);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cl = lane & 15, kr = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;  // the wave's 64 x 64 quadrant
    const int64_t m = P.m, L = P.L;
    int64_t cnt = P.st->nb_count;
    if (cnt > B.cap) cnt = B.cap;
    const int64_t row0 = (int64_t)blockIdx.x * RNG_TILE;
    const int64_t slot0 = (int64_t)blockIdx.y * RNG_TILE;

    // load map: thread t stages the dbl2 at k = 2 (t & 7) of rows (t >> 3) + 32 u of either operand
    const int lk = 2 * (tid & 7), lr = tid >> 3;
    const double* srow[BD_LOADS];
    const double* acol[BD_LOADS];
#pragma unroll
    for (int u = 0; u < BD_LOADS; ++u) {
        const int64_t i = row0 + lr + 32 * u;
        srow[u] = i < m ? B.S + i * L : nullptr;
        const int64_t s = slot0 + lr + 32 * u;
        acol[u] = s < cnt ? P.A + (int64_t)P.nb_list[s] * L : nullptr;  // (a slack's unit column too)
    }

    dbl4 acc[4][4];
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) acc[it][jt] = dbl4{0.0, 0.0, 0.0, 0.0};

    dbl2 sv[BD_LOADS], av[BD_LOADS];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int u = 0; u < BD_LOADS; ++u) {
            sv[u] = bd_load(srow[u], k0 + lk, m);
            av[u] = bd_load(acol[u], k0 + lk, m);
        }
    };
    auto stage = [&](int buf) {
        double* d = lds + buf * BD_STAGE;
#pragma unroll
        for (int u = 0; u < BD_LOADS; ++u) {
            *reinterpret_cast<dbl2*>(d + (lr + 32 * u) * RNG_LD + lk) = sv[u];
            *reinterpret_cast<dbl2*>(d + BD_OPER + (lr + 32 * u) * RNG_LD + lk) = av[u];
        }
    };

    const int nchunk = (int)((m + RNG_KC - 1) / RNG_KC);
    fetch(0);
    stage(0);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        if (c + 1 < nchunk) fetch((int64_t)(c + 1) * RNG_KC);  // in flight during this chunk's MFMAs
        const double* ds = lds + (c & 1) * BD_STAGE + (wr * 64 + cl) * RNG_LD + kr;
        const double* da = lds + (c & 1) * BD_STAGE + BD_OPER + (wc * 64 + cl) * RNG_LD + kr;
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

    // Every wave is past the K loop's last barrier: the staging buffers now take the workgroup's rows (x_b clamped
    // into [0, ub_B], ub_B, "basic column is free"; a row past m as free: T is 0 there anyway) and, behind them,
    // the half records.
    double* s_x = lds;
    double* s_u = lds + RNG_TILE;
    int32_t* s_fr = reinterpret_cast<int32_t*>(lds + 2 * RNG_TILE);
    BdHalf* half = reinterpret_cast<BdHalf*>(lds + BD_ROWS_DBL);  // [2][RNG_TILE]
    if (tid < RNG_TILE) {
        const int64_t i = row0 + tid;
        double xv = 0.0, uv = INFINITY;
        int32_t fr = 1;
        if (i < m) {
            uv = B.ub_B ? B.ub_B[i] : INFINITY;
            xv = P.x_b[i];
            xv = xv > 0.0 ? xv : 0.0;
            xv = xv < uv ? xv : uv;
            fr = B.is_free ? (int32_t)B.is_free[P.b_ixs[i]] : 0;
        }
        s_x[tid] = xv;
        s_u[tid] = uv;
        s_fr[tid] = fr;
    }
    __syncthreads();

    // Epilogue.  acc[it][jt][r] is T at row wr 64 + 16 it + 4 r + kr and slot wc 64 + 16 jt + cl of the tile
    // (the f64 accumulator layout: column = lane & 15, row = (lane >> 4) + 4 r).  x_B(t) = x_B - t alpha.
    const double tol = B.tol;
    double dn[4], up[4];
    int32_t kdn[4], kup[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        dn[jt] = up[jt] = INFINITY;
        kdn[jt] = kup[jt] = BD_NONE;
    }
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // the lane's 16 rows
            const int li = wr * 64 + 16 * it + 4 * r + kr;
            if (s_fr[li]) continue;
            const double xv = s_x[li], uv = s_u[li];
            const int32_t key = (int32_t)(2 * (row0 + li));
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                const double t = acc[it][jt][r];
                const double a = fabs(t);
                if (!(a > tol)) continue;
                const double lo = xv / a;  // to the lower bound (side 0)
                if (t > 0.0) bd_min(lo, key, up[jt], kup[jt]);
                else bd_min(lo, key, dn[jt], kdn[jt]);
                if (uv < INFINITY) {  // to the upper bound (side 1)
                    const double hi = (uv - xv) / a;
                    if (t > 0.0) bd_min(hi, key + 1, dn[jt], kdn[jt]);
                    else bd_min(hi, key + 1, up[jt], kup[jt]);
                }
            }
        }
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
#pragma unroll
        for (int x = 16; x < 64; x <<= 1) {  // the 4 lanes that hold the slot: xor 16, 32
            const double odn = __shfl_xor(dn[jt], x, 64), oup = __shfl_xor(up[jt], x, 64);
            const int32_t okdn = __shfl_xor(kdn[jt], x, 64), okup = __shfl_xor(kup[jt], x, 64);
            bd_min(odn, okdn, dn[jt], kdn[jt]);
            bd_min(oup, okup, up[jt], kup[jt]);
        }
        if (kr == 0) half[wr * RNG_TILE + wc * 64 + 16 * jt + cl] = BdHalf{dn[jt], up[jt], kdn[jt], kup[jt]};
    }
    __syncthreads();
    if (tid < RNG_TILE && slot0 + tid < cnt) {  // the two row halves, then one partial per (row block, slot)
        BdHalf h = half[tid];
        const BdHalf o = half[RNG_TILE + tid];
        bd_min(o.down, o.kdown, h.down, h.kdown);
        bd_min(o.up, o.kup, h.up, h.kup);
        RngPart p;
        p.down = h.down;
        p.up = h.up;
        p.kdown = h.kdown == BD_NONE ? INT64_MAX : (int64_t)h.kdown;
        p.kup = h.kup == BD_NONE ? INT64_MAX : (int64_t)h.kup;
        B.parts[(int64_t)blockIdx.x * B.cap + slot0 + tid] = p;
    }
}

// slot s's partials over the row blocks merged by key; the own-bound cap; scattered to the slot's column
__global__ __launch_bounds__(RNG_BLOCK) void k_rng_bound_min(Params P, BndArgs B) {
    int64_t cnt = P.st->nb_count;
    if (cnt > B.cap) cnt = B.cap;
    const int64_t s = (int64_t)blockIdx.x * RNG_BLOCK + threadIdx.x;
    if (s >= cnt) return;
    double dn = INFINITY, up = INFINITY;
    int64_t kdn = INT64_MAX, kup = INT64_MAX;
    for (int rb = 0; rb < B.row_blocks; ++rb) {
        const RngPart p = B.parts[(int64_t)rb * B.cap + s];
        bd_min64(p.down, p.kdown, dn, kdn);
        bd_min64(p.up, p.kup, up, kup);
    }
    if (kdn == INT64_MAX) kdn = -1;
    if (kup == INT64_MAX) kup = -1;
    const int32_t kind = B.kind[s];
    const double u = B.ubj[s];
    if (kind == 2) {  // free: no bound to move
        dn = up = INFINITY;
        kdn = kup = -1;
    } else if (kind == 0) {  // at lower: the rising bound meets the upper one (strictly first, or the row is reported)
        if (u < up) {
            up = u;
            kup = BND_OWN;
        }
    } else if (u < dn) {  // at upper: the falling bound meets the lower one
        dn = u;
        kdn = BND_OWN;
    }
    const int32_t j = B.col[s];
    B.down[j] = dn;
    B.up[j] = up;
    B.kdown[j] = kdn;
    B.kup[j] = kup;
}

// row i's basic column: its own two slacks
__global__ __launch_bounds__(RNG_BLOCK) void k_rng_bound_basic(Params P, BndArgs B) {
    const int64_t m = P.m;
    const int64_t i = (int64_t)blockIdx.x * RNG_BLOCK + threadIdx.x;
    if (i >= m) return;
    const int64_t j = P.b_ixs[i];
    const double uv = B.ub_B ? B.ub_B[i] : INFINITY;
    double xv = P.x_b[i];
    xv = xv > 0.0 ? xv : 0.0;  // clamped into [0, ub_B]
    xv = xv < uv ? xv : uv;
    const bool fr = B.is_free && B.is_free[j];
    const bool fin = uv < INFINITY;
    B.up[j] = fr ? INFINITY : xv;
    B.kup[j] = fr ? -1 : 2 * i;
    B.down[j] = fin ? uv - xv : INFINITY;
    B.kdown[j] = fin ? 2 * i + 1 : -1;
}

hipError_t bnd_prepare() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_rng_bound), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)BD_LDS);
}

hipError_t launch_rng_bound(const Params& P, const BndArgs& B, const BndCfg& c, hipStream_t s) {
    if (c.col_tiles > 65535 || c.row_blocks > 65535) return hipErrorInvalidValue;  // (the grid's y extent; keys in 31 bits)
    if (c.slot_grid > 0) hipLaunchKernelGGL(k_rng_bound_gather, dim3(c.slot_grid), dim3(RNG_BLOCK), 0, s, P, B);
    if (c.col_tiles > 0 && c.row_blocks > 0)
        hipLaunchKernelGGL(k_rng_bound, dim3(c.row_blocks, c.col_tiles), dim3(RNG_BLOCK), BD_LDS, s, P, B);
    if (c.slot_grid > 0) hipLaunchKernelGGL(k_rng_bound_min, dim3(c.slot_grid), dim3(RNG_BLOCK), 0, s, P, B);
    if (c.row_grid > 0)
        hipLaunchKernelGGL(k_rng_bound_basic, dim3(c.row_grid), dim3(RNG_BLOCK), 0, s, P, B);
    return hipGetLastError();
}

}  // namespace spx
