// spx_kernels.h — host-side launchers for the gfx950 kernels of the dense
// revised-simplex hot loop: the only interface of the kernel units below to
// the host code.
//
// One loop pass is two launches (SURVEY.md §7 design notes):
//   k_price   stages y in LDS (applying the last pivot's y update on the fly),
//             then e_j = y.A_j - c_j over this rank's non-basic columns fused
//             with the entering argmin (v4:288-302).  One wave per column, A
//             read with 16-byte non-temporal loads, wave shuffle + LDS argmin,
//             last-workgroup-done fan-in.
//   k_update  applies the pending rank-1 update B^-1 += E r^T (v4:331-333)
//             while streaming B^-1 once, and in the same pass computes FTRAN
//             alpha = B^-1_new A_p (v4:307-308), the last pivot's x_b update
//             (v4:347-348) for the rows it owns, compute_theta and the leaving
//             argmin (v4:199-208,324); the last workgroup then finds q, the
//             y-update scalar (v4:352-355) and does the basis bookkeeping
//             (v4:339-342).
// Host synchronisation per pass: none.  Termination (optimum / unbounded /
// iteration limit) is a device-side status word every kernel checks first.
// The deferred pivot state is described in spx_device.h.
//
// Cross-workgroup hand-offs inside a launch (partials, alpha) use agent-scope
// relaxed atomic stores/loads (global_* sc1: L1 bypass) drained with
// s_waitcnt vmcnt(0) before a workgroup barrier and one agent-scope ticket
// add per workgroup (MI355X_MICROARCH.md, Valid forms, first table row), on
// sharded counters (arrive_last, spx_common.h).
// Everything is deterministic: fixed reduction orders, no float atomics, so
// results are bit-identical for any grid / block size and any shard count.
//
// The kernel units, one family each with its launchers:
//   spx_price.hip    k_price and the pricing-only build switches
//   spx_update.hip   k_update, k_ftran_bc (compact operand), k_tab_update
//                    (window tableau) and the one-workgroup tail kernels
//   spx_foldk.hip    the eta window's folds (k_fold, k_cfold) and the compact
//                    operand's list and gather
//   spx_kernels.hip  off the two launches: flush and readbacks, setup, the
//                    mailbox exchange, steepest edge's preparation
//   spx_handoff.h    device helpers k_price and the FTRAN kernels share: the
//                    partials, the pivot tail, mailbox records, phase stamps
#pragma once
#include <hip/hip_runtime.h>

#include "spx_device.h"

namespace spx {

struct PriceCfg {
    int block;         // 256 / 512 / 1024 threads
    bool lds_y;        // stage y in LDS (L*8 bytes) or read it from global
    int wm;            // 0 explicit B^-1; eta window: 1 base row in LDS, 2 in global; 3 tableau;
                       // 4 / 5 = 1 / 2 with steepest edge (B_w^T alpha in LDS / global);
                       // 6 compact pricing (Params::AS: the listed rows of A, dw, the Wt rows)
    size_t lds_bytes;  // dynamic LDS per workgroup
    int grid;          // workgroups (persistent-style, grid-stride over columns)
    bool tk = false;   // wm 1: the instantiation with the ticketed tail (Params::price_dyn)
    bool dw = false;   // wm 1 / 2: the instantiation that also stores dw[j] (opens a compact-priced window)
};

struct UpdateCfg {
    int block;  // threads per workgroup (256 / 512 / 1024)
    int rows;   // B^-1 rows per wave (1/2/4/8)
    int grid;   // ceil(m / (block / 64 * rows))
    int bc_entry;  // compact FTRAN, 1 row per wave: k_ftran_bc (>= 1) or k_update<..., BC> (0);
                   // with the deferred tail, k_ftran_bc's rows per wave (1, 2, 4: SPX_FTRAN_RPW)
    int mark;      // diagnostic: k_mark before the launch (SPX_DIAG_MARK=1, stamps only)
};

hipError_t price_prepare(const PriceCfg& c, int* blocks_per_cu);
hipError_t launch_price(const Params& P, const PriceCfg& c, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
// compact pricing: dw for the basic columns, after the dense pass that stored the others
hipError_t launch_dw_basic(const Params& P, hipStream_t s);
hipError_t launch_update(const Params& P, const UpdateCfg& c, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
// a pending deferred ratio-test tail (Params::defer_tail), applied on its own
hipError_t launch_apply_tail(const Params& P, hipStream_t s);
hipError_t launch_generate(double* A, double* b, double* c, int64_t m, int64_t n, int64_t L, uint64_t seed,
                           hipStream_t s);
hipError_t launch_reset(const Params& P, hipStream_t s);
hipError_t launch_flush(const Params& P, hipStream_t s);
hipError_t launch_finalize_rs(const Params& P, hipStream_t s);
hipError_t launch_exchange(const Params& P, hipStream_t s);
hipError_t launch_compact(const Params& P, hipStream_t s);
hipError_t launch_tail(const Params& P, int nparts, hipStream_t s);
hipError_t launch_materialize(const Params& P, double* out, hipStream_t s);
hipError_t launch_reduced_costs(const Params& P, double* e, hipStream_t s);
hipError_t launch_objective(const Params& P, hipStream_t s);
// carry (compact pricing, the compact fold): dw[j] += sum_t SY[t] Wt[j][t]
// before the fold changes y_w, and stays valid (bc_n[5]) if it was
hipError_t launch_fold(const Params& P, int min_nw, int cus, hipStream_t s, bool carry = false);
// steepest edge (P.steep): weights at the slack basis; B_w^T alpha, U^T alpha
// and gamma_p of the pending pivot before a pricing pass
hipError_t launch_se_init(const Params& P, hipStream_t s);
hipError_t launch_se_prep(const Params& P, hipStream_t s, int fused_parts = 0);  // fused_parts: the FTRAN pass's partials
int se_parts_for(int64_t m);

}  // namespace spx
