// spx_dwcarry.h — compact pricing: which windows open with the dense pass
// that stores dw (an anchor) and which carry dw across their fold (host only,
// no HIP: tools/dw_carry_check.cpp compiles it alone).
//
// dw[j] = y_w . A_j - c_j is stored by the dense pass k_price<.., DW> plus
// k_dw_basic, and follows y_w across a fold by dw[j] += sum_t SY[t] Wt[j][t]
// (k_as_rows).  The carried sum takes at most KW - 1 roundings per window, so
// every P-th fold since the last anchor anchors again: P = 32 by default, a
// design constant that keeps the dense stream under 1/32 of one per window;
// SPX_DW_ANCHOR=N sets it, 1 = every fold (no carry), 0 = never again.
// The rule reads the fold count since the last anchor and whether dw is
// valid, nothing else: not the call's length, the dispatch or its chunking.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace spx_host {

struct DwCarry {
    int32_t period = 32;  // P
    int32_t since = 0;    // folds carried since the last anchor
    bool ok = false;      // dw belongs to the current y_w (the device's bc_n[5] == 1)
    int64_t anchors = 0;  // windows opened by an anchor pass (monotone)

    // would the next fold of a compact-priced window carry
    bool carry_next() const { return ok && (period == 0 || since + 1 < period); }
    // a loop fold: true = it carries (dw stays valid), false = dw is stale and
    // the window opens with an anchor
    bool fold() {
        const bool c = carry_next();
        if (c) ++since;
        else ok = false;
        return c;
    }
    void anchor() {
        ok = true;
        since = 0;
        ++anchors;
    }
    void invalidate() { ok = false; }

    // Batch graphs (nf folds each, the first one at the batch's start).  The
    // anchor batch is captured with dw stale, so its first fold anchors and
    // the others follow the rule from there; the carry batch carries at every
    // fold.  A batch fits when the rule would decide each of its folds the
    // same way; where neither fits, the window is enqueued pass by pass.
    bool fits_anchor_batch() const { return !carry_next(); }
    bool fits_carry_batch(int nf) const { return ok && (period == 0 || since + nf < period); }
    void replay(int nf) {  // the host's mirror of a replayed batch
        for (int i = 0; i < nf; ++i)
            if (!fold()) anchor();
    }
};

// SPX_DW_ANCHOR's value (nullptr: unset)
inline int32_t dw_period_from(const char* env, int32_t dflt = 32) {
    if (!env || !*env) return dflt;
    char* end = nullptr;
    const long v = std::strtol(env, &end, 10);
    if (end == env || v < 0) return dflt;
    return (int32_t)std::min<long>(v, 1 << 30);
}

// Mean bytes of a window's pricing launches under the anchor period: KW - 1
// launches, all compact in a carried window; an anchor window (one in P, or
// none when P == 0: the first window's share vanishes over a solve) has one
// dense stream among them.  dense / compact: the bytes of one such pass.
inline double dw_mean_price_bytes(double dense, double compact, int win, int32_t period) {
    const double passes = (double)(win - 1);
    const double share = period > 0 ? 1.0 / (double)period : 0.0;
    return ((passes - share) * compact + share * dense) / passes;
}
// the carry's bytes per window: dw read and written and the Wt rows read
inline double dw_carry_bytes(int64_t n, int win) { return 8.0 * (double)n * (double)(win + 2); }

}  // namespace spx_host
