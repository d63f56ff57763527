// spx_ctx.h — what the host translation units behind include/simplex.h share
// (spx_api.cpp, spx_api_dual.cpp, spx_api_pbox.cpp, spx_api_ranging.cpp): the context, the error plumbing and the few
// helpers one unit calls in the other.  Internal: not installed, not part of
// the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/simplex.h"
#include "spx_device.h"
#include "spx_dual.h"
#include "spx_dwcarry.h"
#include "spx_kernels.h"
#include "spx_loop.h"
#include "spx_pbox.h"
#include "spx_ranging.h"
#include "spx_bndrange.h"
#include "spx_reinv.h"

namespace spx_host {

// records the message spx_last_error returns (thread-local) and returns `code`
int fail(int code, const char* fmt, ...);

}  // namespace spx_host

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return spx_host::fail(e_ == hipErrorOutOfMemory ? SPX_ERR_OOM : SPX_ERR_HIP, "%s: %s (%s:%d)", \
                                  #expr, hipGetErrorString(e_), __FILE__, __LINE__);          \
    } while (0)

#define NCCL_TRY(expr)                                                                                  \
    do {                                                                                                \
        ncclResult_t r_ = (expr);                                                                       \
        if (r_ != ncclSuccess)                                                                          \
            return spx_host::fail(SPX_ERR_RCCL, "%s: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

#define SPX_TRY(expr)          \
    do {                       \
        int rc_ = (expr);      \
        if (rc_ != SPX_OK) return rc_; \
    } while (0)

// The dual simplex loop's host state (spx_dual.h; everything that reads or
// writes it is in spx_api_dual.cpp, the rest of the runtime goes through the
// hooks at the end of this file).  Invariants, between any two API calls:
//  - args.rho != nullptr  <=>  dual_setup ran: every buffer of DualSeArgs, cfg
//    and e are allocated.  args.ub / ub_B / at_upper and b_user are allocated by
//    the first spx_set_bounds with a finite bound, and never freed.
//  - checked: the current basis passed the dual feasibility check (boxed: the
//    entry normalisation) since it was last set from outside the dual loop.
//    Cleared by reset, spx_set_basis, spx_set_algorithm and spx_set_bounds;
//    reinversion keeps the basis and so keeps it.
//  - the steepest-edge weights args.w are those of the current B^-1, or w_stale
//    is set (k_dual_norms runs before the next steepest pass or readback).
//    Only steepest-edge dual passes keep them: everything else that changes
//    B^-1 or the rule sets w_stale.
//  - boxed  <=>  some upper bound is finite.  Then the passes run the boxed
//    kernels, b_user holds the caller's right-hand side and Params::b (= ctx b)
//    is the effective one, b_user - sum_{j non-basic at upper} u_j A_j.  Not
//    boxed: Params::b is the caller's b and no column is at upper.
//  - ub is empty (never set: all +inf) or holds n bounds, the host copy of args.ub.
//  - ratio is the ratio test of the next boxed pass (spx_set_dual_ratio); it
//    invalidates nothing: x_b, Params::b and at_upper are consistent between any
//    two calls under either rule.  args.lrec != nullptr  <=>  the long-step
//    buffers (rkey .. lrec) are allocated: by the first boxed pass under
//    SPX_DUAL_RATIO_LONG_STEP, never freed.  The flip counters live in args.lrec
//    (all 0 while it is not allocated).
struct DualState {
    spx::DualLongArgs args{};
    spx::DualCfg cfg{};
    double* e = nullptr;  // n reduced costs (the feasibility check)
    int32_t rule = SPX_DUAL_PRICING_DANTZIG;  // leaving-row rule (spx_set_dual_pricing)
    int32_t ratio = SPX_DUAL_RATIO_TEXTBOOK;  // ratio test of the boxed passes (spx_set_dual_ratio)
    bool checked = false;
    bool w_stale = true;
    bool boxed = false;
    std::vector<double> ub;
    double* b_user = nullptr;  // L
    // general bounds (spx_set_bounds_lu).  lb is empty (no lower
    // bound but 0: everything above holds as it reads) or holds n lower bounds,
    // some non-zero (-inf: a free column); then ub_user holds the caller's n
    // upper bounds, ub (and args.ub) the ranges ub_user - lb (+inf for a free
    // column), boxed is set whatever the ranges are, and Params::b is b_user -
    // A lsh - the at-upper sum of the ranges (lsh = lb, 0 where -inf).  shifted
    // <=> some lsh[j] != 0: box_sync then runs k_box_rhs_lu with d_lsh, the device
    // copy of lsh (allocated by the first such call, never freed).  nfree counts
    // the free columns: > 0 only while the context does not run SPX_ALGO_DUAL.
    std::vector<double> lb, ub_user;
    bool shifted = false;
    int64_t nfree = 0;
    double* d_lsh = nullptr;  // n
};

// The bounded primal loop's host state (spx_pbox.h; everything that reads or
// writes it is in spx_api_pbox.cpp).  The bounds, placements and the caller's
// right-hand side are DualState's (args.ub / ub_B / at_upper, b_user, ub,
// boxed): PboxArgs points at the same buffers.  Invariants:
//  - args.rec != nullptr  <=>  pbox_setup ran: parts, rparts, rec and cfg are
//    set, and so are the dual loop's buffers (dual_setup) and the boxed ones
//    (box_buffers: with no finite bound ub and ub_B are all +inf, at_upper all 0).
//  - checked: since the basis, the bounds, b, c or the algorithm were last set
//    from outside, the entry check passed (x_b recomputed from the placements
//    and within its bounds) and rbuf holds the pending pivot's row.
//  - the counters live in args.rec (all 0 while it is not allocated).
//  - phase 1 (spx_set_primal_phase1): p1.ph != nullptr  <=>
//    pbox_setup ran (w, yp, vparts and the device phase word are allocated with
//    the rest, whatever `phase1` says).  ninf / y_stale: the device phase word as
//    of the last readback by this loop; passes are the four-step ones while
//    phase1 && (ninf > 0 || y_stale).  y_dirty: a four-step pass was enqueued
//    since y was last known current, so a readback of y (flush), a switch of the
//    algorithm or of phase1 first runs the refresh (pbox_fresh_y).  With phase1
//    off and y_dirty clear the loop is the three-launch loop and never reads p1.
//  - steepest edge (spx_set_primal_pricing): se.se != nullptr  <=>
//    pbox_se_setup ran (gamma, rho, tau, tparts and the pending record, allocated
//    by the first steepest-edge pass or weight readback; a Dantzig context never
//    allocates or launches any of it).  se.gamma holds the weights of the current
//    basis up to the recurrence the device record marks pending, or se_stale is
//    set: the next steepest-edge pass or readback restarts them at 1 + ||A_j||^2
//    and clears the record.  Only steepest-edge passes keep them: reset,
//    spx_set_basis, spx_set_algorithm and a change of rule set se_stale; a
//    reinversion keeps the basis and the record owns its operands, so it stays.
//    rule == STEEPEST and phase1 never hold together (both setters refuse).
//  - exact weights (spx_set_primal_weight_init, spx_refresh_primal_weights;
//    DESIGN.md §7i): wx.parts != nullptr  <=>  pbox_wexact_setup ran (the partial
//    buffers and wx_S, an m x L copy of the true B^-1, allocated by the first
//    exact recomputation; a context in REFERENCE mode that never refreshes
//    allocates and launches none of it).  wx_S is shared with ranging
//    (RangingState), whichever asks first allocates it (pbox_binv_copy); both
//    overwrite it whole before they read it.  winit says what a restart does for a
//    warm basis; warm: spx_set_basis was called since create / the last reset, so
//    the slack basis is `!warm && pivots == 0`, where a restart is
//    k_pbox_se_init's in both modes.
struct PboxState {
    spx::PboxArgs args{};
    spx::PboxCfg cfg{};
    bool checked = false;
    spx::Pbox1Args p1{};
    bool phase1 = false;
    bool y_dirty = false;
    int32_t ninf = 0;
    int32_t y_stale = 0;
    std::vector<hipEvent_t> ev_vtb;  // timing: pairs around k_pbox_vtb + k_pbox_vtb_sum, or k_pbox_tau + _sum (spx_pbox_vtb_times)
    size_t n_vtb = 0;
    int32_t rule = SPX_PRIMAL_PRICING_DANTZIG;  // entering rule (spx_set_primal_pricing)
    // phase 1's rule (spx_set_primal_phase_one_pricing), consulted only while phase1 && rule ==
    // STEEPEST: that state exists only with p1rule == STEEPEST (create and the three setters refuse it otherwise)
    int32_t p1rule = SPX_PRIMAL_PRICING_DANTZIG;
    bool se1_ready = false;  // pbox_se1_prepare ran
    // the rule with free columns (spx_set_primal_free_pricing), consulted only while DualState::nfree > 0
    // && rule == STEEPEST: that state exists only with frrule == STEEPEST (spx_set_bounds_lu and the two setters
    // refuse it otherwise).  Then every pass runs k_pbox_price_se_f / k_pbox_update_f / k_pbox_step_se_f.
    int32_t frrule = SPX_PRIMAL_PRICING_DANTZIG;
    bool sef_ready = false;  // pbox_se_f_prepare ran
    spx::PboxSeArgs se{};
    spx::PboxSeCfg secfg{};
    bool se_stale = true;
    int32_t winit = SPX_PRIMAL_WEIGHTS_REFERENCE;  // how the weights restart for a warm basis
    bool warm = false;
    spx::PboxWexactArgs wx{};
    spx::PboxWexactCfg wxcfg{};
    double* wx_S = nullptr;  // m x L
    std::vector<hipEvent_t> ev_wx;  // timing: pairs around an exact recomputation (spx_pbox_wexact_times)
    size_t n_wx = 0;
    // free columns: fr.lb_B != nullptr  <=>  pbox_free_setup ran
    // (is_free and lb_B, allocated by the first entry check of a context with
    // DualState::nfree > 0; any other context allocates and launches none of it).
    // The entry check uploads both from DualState::lb and the basis; between
    // entry checks k_pbox_step_f / k_pbox_step_se_f keeps lb_B.  While nfree > 0 every
    // pass runs the *_f kernels (the rule is Dantzig) or the *_se_f ones (steepest
    // edge with frrule == STEEPEST), and with phase1 off the device's ninf is 0.
    spx::PboxFreeArgs fr{};
    int8_t* fr_flags = nullptr;  // n (fr.is_free)
    // phase 1's ratio test (spx_set_primal_phase_one_ratio): consulted per pass, under the host
    // condition that launches k_pbox_vtb.  lg.lrec != nullptr  <=>  a pass ran under SPX_PRIMAL_RATIO_LONG_STEP (the
    // counters, allocated by the first such pass; a context that never sets the rule allocates and launches nothing)
    int32_t p1ratio = SPX_PRIMAL_RATIO_TEXTBOOK;
    spx::PboxLongArgs lg{};
};

// Sensitivity ranging (spx_ranging.h; everything that reads or writes it is in
// spx_api_ranging.cpp).  args.cparts != nullptr  <=>  ranging_setup
// ran: every buffer of RngArgs but S (PboxState::wx_S, shared) and cfg are set,
// by the first spx_ranging_cost / spx_ranging_rhs; a context that never asks
// allocates and launches none of it.  Nothing here outlives a call but the
// buffers: every call recomputes from the context's current state, and writes
// nothing the loops read.
struct RangingState {
    spx::RngArgs args{};
    spx::RngCfg cfg{};
    double* d = nullptr;         // n reduced costs
    int8_t* free_flags = nullptr;  // n (args.is_free while the context holds a free column)
    std::vector<hipEvent_t> ev[2];  // timing: pairs around a cost [0] / right-hand-side [1] ranging (spx_ranging_times)
    size_t n_ev[2] = {0, 0};
};

// Bound ranging (spx_bndrange.h; everything that reads or writes it is in
// spx_api_ranging.cpp).  args.parts != nullptr  <=>  bound_setup
// ran: every buffer of BndArgs but S (PboxState::wx_S, shared as above) and cfg
// are set, by the first spx_ranging_bound; a context that never asks allocates
// and launches none of it.  As RangingState, nothing outlives a call but the
// buffers.
struct BoundRangingState {
    spx::BndArgs args{};
    spx::BndCfg cfg{};
    int8_t* free_flags = nullptr;  // n (args.is_free while the context holds a free column)
    std::vector<hipEvent_t> ev;    // timing: pairs around a bound ranging (spx_ranging_bound_times)
    size_t n_ev = 0;
};

struct spx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int cus = 256;
    int64_t m = 0, n = 0, L = 0, ns = 0;
    spx_opts opts{};
    spx::Params P{};
    spx::PriceCfg pcfg{};
    spx::UpdateCfg ucfg{};
    int64_t max_local_cols = 0;

    // device allocations
    std::vector<void*> allocs;
    double* A = nullptr;
    double* b = nullptr;
    double* c = nullptr;
    spx::ArgMinEntry* send = nullptr;
    spx::ArgMinEntry* recv = nullptr;

    // pinned host mirrors
    spx::DevState* st_host = nullptr;
    int64_t* limit_host = nullptr;

    // multi-rank
    ncclComm_t comm = nullptr;
    bool comm_ready = false;
    bool use_comm = false;  // MINLOC through RCCL: nranks > 1, or SPX_FLAG_COMM1 (one-rank test of that path)
    bool graph_fallback = false;  // a capture with RCCL calls failed: eager passes
    // peer mailboxes (spx_mbox_export / spx_mbox_attach): MINLOC by k_exchange
    uint64_t* mbox = nullptr;
    uint32_t* mbox_seq = nullptr;
    uint64_t** mbox_peer = nullptr;  // device array of nranks mailbox pointers
    std::vector<void*> mbox_opened;  // IPC mappings of the other ranks' mailboxes
    bool mbox_ready = false;
    bool mbox_fused = false;  // loop passes exchange inside k_price / k_ftran_bc (Params::mbox_fused)
    bool bc_want = false;      // compact FTRAN operand wanted (allocated by set_slack_flags)
    bool slack_ident = false;  // A[:, n-m:] = I (checked before setup_common)
    bool defer_ok = false;        // loop passes defer the pricing tail into k_update (Params::defer_price)
    bool defer_tail = false;      // loop passes defer the ratio-test tail into k_price (Params::defer_tail)
    // steepest edge: k_ftran_bc stores k_se_part's sums (Params::se_fused) when
    // se_fuse is set; se_chain = the last pass enqueued did, and nothing since
    // changed B_w, U or alpha, so the next pass's k_se_fin reads them
    bool se_fuse = false;
    bool se_chain = false;
    int64_t se_rows = 0;

    // compact pricing (Params::AS).  cp_ok: allocated and applicable; cp_now:
    // the passes being enqueued price compactly (decided per chunk of an
    // iterate call from the list length, iterate_raw); dwc.ok: dw belongs to
    // the current y_w (false after a rebuild, a readback flush, a switch of
    // pricing mode and every fold that does not carry it: the next window
    // then opens with the dense pass that stores it, an anchor; dwc decides
    // which folds carry, spx_dwcarry.h).  ccfg / dcfg: the compact launch and
    // the dense launch that stores dw; s_list: bc_n[0] as of the last
    // readback (bcn_host: its pinned mirror)
    bool cp_ok = false, cp_now = false;
    spx_host::DwCarry dwc{};
    spx::PriceCfg ccfg{}, dcfg{};
    int32_t s_list = 0;
    int32_t* bcn_host = nullptr;

    // graph replay of `batch` passes (graph_c / graph_exec_c: the batch with
    // compact pricing whose first window opens with an anchor; graph_k /
    // graph_exec_k: the one whose folds all carry dw; all are captured by
    // spx_prepare)
    hipGraphExec_t graph_exec = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec_c = nullptr;
    hipGraph_t graph_c = nullptr;
    hipGraphExec_t graph_exec_k = nullptr;
    hipGraph_t graph_k = nullptr;
    int batch = 0;

    // in-process group exchange
    hipEvent_t ev_sent = nullptr, ev_recv = nullptr, ev_sent2 = nullptr, ev_recv2 = nullptr;
    // row-sharded B^-1
    int64_t mb = 0;
    unsigned char* rs_recv = nullptr;

    // per-kernel timing
    bool timing = false;
    std::vector<hipEvent_t> ev_price, ev_update;  // pairs (start, stop)
    std::vector<hipEvent_t> ev_xend;              // after the MINLOC exchange
    size_t n_price = 0, n_update = 0;

    int64_t pivots = 0;
    int32_t status = SPX_STATUS_MAX_ITER;
    bool stepped_price = false;
    int nw = 0;  // eta window: device st->nw as of the last readback, advanced per enqueued pass
    // what the loop actually enqueued (spx_dispatch_stats)
    int64_t n_eager = 0, n_graph_launch = 0, n_graph_pass = 0, n_persist_launch = 0, n_persist_pass = 0;
    int64_t n_persist_fallback = 0;  // persistent launches found not co-resident
    int64_t n_folds = 0;
    int64_t n_graph_builds = 0;  // batch graphs captured + instantiated + uploaded
    int graph_folds = 0;     // folds inside one captured batch
    bool capturing = false;  // build_graph: passes are recorded, not run

    // persistent loop kernel (spx_loop.h): window mode, one rank
    spx::LoopCfg lcfg{};
    spx::LoopArgs la{};
    bool persist = false;
    double loop_clock[3] = {0.0, 0.0, 0.0};  // timing: phase A / B / C microseconds (in-kernel clock)
    int64_t loop_clock_passes = 0;
    uint32_t loop_epoch = 0;  // persistent launches so far (LoopArgs::epoch)
    std::vector<hipEvent_t> ev_loop;
    std::vector<int32_t> ev_loop_passes;
    size_t n_loop = 0;
    std::vector<hipEvent_t> ev_fold;  // timing: the window folds between loop launches
    size_t n_fold = 0;

    // basis reinversion (spx_reinv.h): work buffers allocated on first use
    spx::RvParams rv{};
    double* rv_Pa = nullptr;
    double* rv_Pb = nullptr;
    double* rv_Ypart = nullptr;
    int64_t* rv_cols = nullptr;
    int64_t* rv_pos = nullptr;
    int64_t refactor_base = 0;  // pivots at the last reinversion (opts.refactor_every)
    bool broken = false;        // a failed spx_set_basis left no valid basis

    int32_t algo = SPX_ALGO_PRIMAL;  // the loop spx_iterate runs
    DualState dual;                  // the dual one's state (spx_api_dual.cpp)
    PboxState pbox;                  // the bounded primal one's (spx_api_pbox.cpp)
    RangingState rng;                // sensitivity ranging (spx_api_ranging.cpp)
    BoundRangingState brng;          // bound ranging (spx_api_ranging.cpp)

    template <typename T>
    int alloc(T** p, size_t count, unsigned ext_flags = ~0u) {
        void* d = nullptr;
        size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        hipError_t e = ext_flags == ~0u ? hipMalloc(&d, bytes) : hipExtMallocWithFlags(&d, bytes, ext_flags);
        if (e != hipSuccess)
            return spx_host::fail(SPX_ERR_OOM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        allocs.push_back(d);
        e = hipMemsetAsync(d, 0, bytes, stream);
        if (e != hipSuccess) return spx_host::fail(SPX_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
        *p = static_cast<T*>(d);
        return SPX_OK;
    }
};

namespace spx_host {

// spx_api.cpp, called by the dual loop
bool env_on(const char* name);   // the variable is set and starts with '1'
bool env_off(const char* name);  // ... with '0'
size_t env_bytes(const char* name);  // the variable's value where it is a count >= 1, else 0
int clear_tickets(spx_ctx* x);
int read_state(spx_ctx* x);  // the device state to the host: the one synchronisation of an iterate call
int flush(spx_ctx* x);
int set_limit(spx_ctx* x, int64_t limit);
int set_running(spx_ctx* x);  // the device and host status back to running (pivot count kept)
// timing: the next price / update event pairs of a pass; its exchange-end
// event is ev_xend[n_price - 1] afterwards
int pass_events(spx_ctx* x, hipEvent_t* p0, hipEvent_t* p1, hipEvent_t* u0, hipEvent_t* u1);

// spx_api_dual.cpp: all the rest of the runtime knows of the dual loop
// the combination of options the dual loop does not run with (for the error
// message), or nullptr.  win: the eta window in use (0 = explicit)
const char* dual_conflict(const spx_opts& o, int win);
void dual_on_create(spx_ctx* x);  // the leaving-row rule opts.flags asks for
int dual_setup(spx_ctx* x);       // buffers and launch geometry, on first use
int iterate_dual(spx_ctx* x, int64_t k);
// boxed: Params::b = the effective right-hand side of the current placements,
// before anything that recomputes x_b from it (not boxed: nothing)
int box_sync(spx_ctx* x);
// do_reset, before launch_reset: boxed, every column back at lower; no pass
// in flight, nothing checked, no weights
int dual_on_reset(spx_ctx* x);
void dual_on_reinvert(spx_ctx* x);   // B^-1 rebuilt for the same or a new basis: no weights
void dual_on_new_basis(spx_ctx* x);  // spx_set_basis: nothing checked
double* dual_rhs_target(spx_ctx* x);  // where spx_set_rhs writes the caller's b
// spx_set_algorithm's refusals and state changes around the switch to `algo`
int dual_switch_algorithm(spx_ctx* x, int32_t algo);
// boxed: zu = sum of c_j u_j over the non-basic columns at upper; else 0
int dual_objective_offset(spx_ctx* x, double* zu);
// the boxed buffers (ub, ub_B, at_upper, b_user), on first use: no bound, every
// column at lower, b_user = Params::b
int box_buffers(spx_ctx* x);
// boxed: a column at an upper bound that no longer exists goes to lower; then
// Params::b from the placements and x_b = B^-1 Params::b (B^-1 untouched)
int box_replace_xb(spx_ctx* x);
// general bounds: x_b[i] += the lower bound of row i's basic column (0 for a free
// one), on a host copy of x_b with its b_ixs; nothing without lower bounds
void box_unshift_xb(const spx_ctx* x, double* x_b, const int64_t* b_ixs);

// spx_api_pbox.cpp: all the rest of the runtime knows of the bounded primal loop
int pbox_setup(spx_ctx* x);  // buffers and launch geometry, on first use
int iterate_pbox(spx_ctx* x, int64_t k);
int pbox_on_reset(spx_ctx* x);     // do_reset: counters cleared, nothing checked
void pbox_on_change(spx_ctx* x);   // the basis, the bounds, b, c or the algorithm were set: nothing checked
int pbox_on_create(spx_ctx* x);    // phase 1 and the entering rule as opts.flags asks for
void pbox_weights_lost(spx_ctx* x);  // the basis was set from outside or another loop takes it: steepest-edge weights restart
void pbox_basis_set(spx_ctx* x);     // spx_set_basis: the basis is no longer known to be the slack basis
int pbox_on_reinvert(spx_ctx* x);  // B^-1, x_b and y rebuilt: y current, the rows classified again
int pbox_fresh_y(spx_ctx* x);      // before anything outside the loop reads y: y = c_B B^-1 if phase 1 left it stale
int pbox_binv_copy(spx_ctx* x);    // PboxState::wx_S, the m x L buffer a true B^-1 is materialised into, on first use

}  // namespace spx_host
