// spx_cprows.h — compact pricing: the row form of a column's operand fetch
// (k_price WM 6, DESIGN.md §4 "Compact pricing"; shared by the kernel and the
// host, no HIP needed: tools/cprows_check.cpp compiles it alone).
//
// A priced column's S listed entries of AS are one contiguous run.  The row
// form reads the run as NC = 2, 4 or 8 coalesced chunks of 64 doubles (lane l
// takes entries l + 64 t), stores them to the wave's private LDS slot and
// hands each lane its own terms from there; the gather form has every lane
// fetch its terms from global memory one by one.  Which form a pass takes is
// a function of the list's length S and the row limit alone (wave-uniform on
// the device), so no grid, block or dispatch enters it, and both forms put
// the same operands into the same fma chain: the same bits.
//   S <= 128: NC 2, four columns in flight;  S <= 256: NC 4, four columns;
//   S <= 512: NC 8, two columns;  S = 0, S > limit: the gather form.
// SPX_CPRICE_ROWS=N sets the limit (the longest list the row form serves):
// 512 by default, 0 = the gather form everywhere, clamped to the rows of AS,
// and lowered a tier at a time where the slots would cost occupancy.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#if defined(__HIPCC__)
#define SPX_CPROWS_HD __host__ __device__
#else
#define SPX_CPROWS_HD
#endif

namespace spx_cprows {

constexpr int ROWS_MAX = 512;  // NC <= 8
constexpr int ROWS_DEFAULT = 512;

// chunks of 64 entries a row of S listed entries is read in; 0 = gather form
SPX_CPROWS_HD constexpr int chunks(int S, int limit) {
    return (S <= 0 || S > limit || S > ROWS_MAX) ? 0 : (S <= 128 ? 2 : (S <= 256 ? 4 : 8));
}
// columns in flight per wave (the gather form keeps its two)
SPX_CPROWS_HD constexpr int depth(int nc) { return (nc == 2 || nc == 4) ? 4 : 2; }
// doubles of a wave's LDS slot: the widest row the limit admits, and behind
// it the unit entry A[q, j] (a pair, so that the slots stay 16-byte aligned)
SPX_CPROWS_HD constexpr int slot_doubles(int limit) { return limit > 0 ? 64 * chunks(limit, limit) + 2 : 0; }
// dynamic LDS the slots add to a workgroup of `waves` waves
SPX_CPROWS_HD constexpr size_t lds_bytes(int waves, int limit) {
    return (size_t)waves * (size_t)slot_doubles(limit) * sizeof(double);
}

// the longest list of the next smaller slot (cprice_setup steps the limit down
// while the slots would take a workgroup off a CU); 0: no row form
SPX_CPROWS_HD constexpr int tier_below(int limit) { return limit > 256 ? 256 : (limit > 128 ? 128 : 0); }

// SPX_CPRICE_ROWS's value (nullptr or unparsable: the default) within the
// rows of AS (cap)
inline int32_t limit_from(const char* env, int64_t cap) {
    long v = ROWS_DEFAULT;
    if (env && *env) {
        char* end = nullptr;
        const long t = std::strtol(env, &end, 10);
        if (end != env && t >= 0) v = t;
    }
    return (int32_t)std::max<int64_t>(0, std::min<int64_t>({(int64_t)v, cap, (int64_t)ROWS_MAX}));
}

}  // namespace spx_cprows
