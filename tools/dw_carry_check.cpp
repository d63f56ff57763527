// dw_carry_check.cpp — host check of the dw anchor rule (spx_dwcarry.h;
// DESIGN.md §4 "Carrying dw"): the anchor counter, the batch graph a replay
// picks, and the bytes_price / carry arithmetic of spx_info.  A loop that
// enqueues pass by pass is the reference; the batched loop (graphs of nf
// folds where one fits, passes elsewhere) must take the same decision at
// every fold and count the same anchors, for every period, batch shape,
// call chunking and invalidation pattern.  No device code.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/dw_carry_check.cpp -o tools/dw_carry_check
#include <cstdio>
#include <vector>

#include "../simplex_method_gpu_amd/csrc/spx_dwcarry.h"

using spx_host::DwCarry;

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                 \
        }                                                            \
    } while (0)

// one window opened pass by pass (enqueue_pass): the fold, then the anchor
// where dw is stale.  Returns 1 for a carry, 0 for an anchor
static int eager_window(DwCarry& d, bool fold) {
    bool carry = false;
    if (fold) carry = d.fold();
    if (!d.ok) d.anchor();
    return carry ? 1 : 0;
}

// `windows` windows after the first, in calls of `chunk` batches-or-windows,
// batches of nf folds; stale_at: dw goes stale before that window (a readback)
static void run(int period, int nf, int windows, int stale_at, std::vector<int>& trace_ref, int64_t& anchors_ref) {
    DwCarry ref;
    ref.period = period;
    trace_ref.clear();
    eager_window(ref, false);  // the first window: no fold, an anchor
    for (int w = 0; w < windows; ++w) {
        if (w == stale_at) ref.invalidate();
        trace_ref.push_back(eager_window(ref, true));
    }
    anchors_ref = ref.anchors;

    DwCarry d;
    d.period = period;
    std::vector<int> trace;
    eager_window(d, false);
    int w = 0;
    int graph_a = 0, graph_k = 0, eager = 0;
    while (w < windows) {
        const bool whole = w + nf <= windows && !(stale_at > w && stale_at < w + nf);
        if (w == stale_at) d.invalidate();
        if (whole && d.fits_carry_batch(nf)) {
            for (int i = 0; i < nf; ++i) trace.push_back(1);  // (the carry batch carries at every fold)
            d.replay(nf);
            w += nf;
            ++graph_k;
        } else if (whole && d.fits_anchor_batch()) {
            // the anchor batch was captured from a stale dw with this period
            DwCarry cap;
            cap.period = period;
            for (int i = 0; i < nf; ++i) trace.push_back(eager_window(cap, true));
            d.replay(nf);
            w += nf;
            ++graph_a;
        } else {
            trace.push_back(eager_window(d, true));
            ++w;
            ++eager;
        }
    }
    CHECK(trace == trace_ref);
    CHECK(d.anchors == ref.anchors);
    CHECK(d.ok == ref.ok && d.since == ref.since);
    if (nf == 1 && stale_at < 0) CHECK(eager == 0);  // one window per batch: always a graph
    (void)graph_a;
    (void)graph_k;
}

int main() {
    std::vector<int> tr;
    int64_t anchors = 0;
    for (int period : {0, 1, 2, 3, 5, 32})
        for (int nf : {1, 2, 3})
            for (int windows : {0, 1, 7, 64, 100})
                for (int stale_at : {-1, 0, 3, 40}) {
                    run(period, nf, windows, stale_at, tr, anchors);
                    if (stale_at < 0 || stale_at >= windows) {
                        // the documented rule: the first window, then every P-th fold
                        const int64_t want = 1 + (period > 0 ? windows / period : 0);
                        CHECK(anchors == want);
                        for (int w = 0; w < windows; ++w) CHECK(tr[(size_t)w] == ((period > 0 && (w + 1) % period == 0) ? 0 : 1));
                    }
                }
    // SPX_DW_ANCHOR parsing
    CHECK(spx_host::dw_period_from(nullptr) == 32 && spx_host::dw_period_from("") == 32);
    CHECK(spx_host::dw_period_from("0") == 0 && spx_host::dw_period_from("1") == 1 && spx_host::dw_period_from("3") == 3);
    CHECK(spx_host::dw_period_from("-4") == 32 && spx_host::dw_period_from("x") == 32);
    // bytes: period 1 is a dense opener in each of the window's KW - 1 launches' mean, period 0 none
    const double dense = 400e6, compact = 9e6;
    CHECK(spx_host::dw_mean_price_bytes(dense, compact, 64, 1) == (62.0 * compact + dense) / 63.0);
    CHECK(spx_host::dw_mean_price_bytes(dense, compact, 64, 0) == compact);
    const double m32 = spx_host::dw_mean_price_bytes(dense, compact, 64, 32);
    CHECK(m32 > compact && m32 < compact + (dense - compact) / (63.0 * 32.0) * 1.0000001);
    CHECK(spx_host::dw_carry_bytes(16384, 64) == 8.0 * 16384 * 66);
    if (fails) std::printf("%d checks failed\n", fails);
    else std::printf("ok\n");
    return fails ? 1 : 0;
}
