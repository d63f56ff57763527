"""Bounded primal simplex loop (SPX_ALGO_PRIMAL_BOX) at C3's
shape against the dual and the primal explicit pass.

Every side runs in a child process of its own on device 0, in this order, so the
first and the last record show the drift of the box:
  primal        the headline LP (seeded generator), window=-1: k_price / k_update
  dual          the covering LP of tests/dual_ref.py, SPX_ALGO_DUAL (Dantzig):
                k_dual_price / k_dual_update
  pbox          the bounded LP of tests/primal_box_ref.py boxed_primal(m, n, seed),
                SPX_ALGO_PRIMAL_BOX: k_pbox_price / k_pbox_update
  primal_again
Per side: it/s over --k timed pivots of an untimed context after --warm pivots,
and from a timing context (SPX_FLAG_TIMING) the mean kernel times of the same
passes, the pricing kernel's algorithmic bandwidth 8 (m + 1) x streamed
non-basic columns / time against 8 TB/s, and rest_us = what a pass takes beyond
its two big kernels (the one-workgroup kernel and the launch gaps).  The pbox
record also carries the flip passes and to-upper pivots of the timed block.

--solve times whole bounded solves to the optimum at every --solve-shape
(pivots, seconds, flip counts), each checked by the CPU certificate recomputed
from the returned basis and placements (tests/dual_box_ref.py certificate).
--rows adds, per solve shape, the same LP with every finite bound written as a
row (x_j + s = u_j; a bounded slack u_k becomes the row a_k.x >= b_k - u_k,
negated) on the primal loop with its default eta window.

--phase1 measures the loop's phase 1 (SPX_FLAG_PRIMAL_PHASE1)
instead, again one child per side, the sides alternating:
  pbox          as above (flag off): the phase-2 pass rate the others compare with
  pbox_flag     the same LP with the flag on: a feasible entry, so the same three
                launches per pass
  p1_dense      tests/primal_phase1_ref.py boxed_general(m, n, seed) from the slack
                basis: the start of phase 1, about two thirds of the rows infeasible
  p1_sparse     boxed_primal's LP with every --sparse-every-th row turned into a
                violated >= row: few infeasible rows, phase 1 near its end; once
                they are gone the same context's phase-2 passes are timed after
                --warm more pivots (pivots and passes per second, flip passes, and
                under SPX_FLAG_TIMING the kernel times and the count of k_pbox_vtb
                launches, 0 once the loop is back on the three-launch pass)
  pbox_again, pbox_flag_again
Phase-1 records carry the rows out of bounds before and after the timed passes,
passes and pivots per second, the mean times of k_pbox_vtb (+ its reduction),
the pricing and the update kernel over the phase-1 passes, and k_pbox_vtb's
algorithmic bandwidth 8 L x (rows with w_i != 0, the mean of before and after)
/ time beside the update kernel's 16 m L / time, both against 8 TB/s.

--primal-pricing steepest measures exact steepest-edge pricing
against the Dantzig loop instead, one child per side, the sides alternating:
  pbox          as above (Dantzig): k_pbox_price
  pbox_se       the same LP under SPX_PRIMAL_PRICING_STEEPEST: k_pbox_price_se, and
                tau_us, the mean of k_pbox_tau + k_pbox_tau_sum over the pivot passes
  pbox_se_lds1 / pbox_se_lds0   the LDS layouts that are not the default (y alone in
                LDS with rho and tau from L2; nothing in LDS), through the
                SPX_PBOX_SE_LDS experiment switch
  pbox_again, pbox_se_again
and, with --solve, whole solves (the --solve mode above) at every --solve-shape
under both rules, Dantzig / steepest / Dantzig / steepest, with the ratios of
pivots and seconds.

--warm-resolve measures the exact weight start of a warm basis
instead, one child process per shape:
  resolve       at every --solve-shape the LP of tests/dual_box_ref.py boxed(m, n,
                seed): a boxed dual steepest-edge solve, spx_set_cost with
                primal_box_ref.cost_variant, spx_set_algorithm(SPX_ALGO_PRIMAL_BOX)
                under steepest edge and the re-solve; after one untimed sequence
                (first-launch costs) the two start modes alternate in that process,
                REFERENCE / EXACT / REFERENCE / EXACT: pivots, flip passes and wall
                seconds of the re-solve (the exact start inside them), and from one
                more EXACT sequence under SPX_FLAG_TIMING the exact start's device time
  kernel        at every --kernel-shape boxed_primal's LP under steepest edge after
                --warm pivots: five spx_refresh_primal_weights, their device times
                (spx_pbox_wexact_times), the fp64 rate 2 m^2 (n - m) / time of the
                fastest, and the mean wall time of a steepest-edge pass of the same
                context over --k pivots, so the start is also quoted in passes

--free measures the free-column kernels instead, in phase 1,
where the kernels they derive from run; one child per side, the sides
alternating:
  p1_parent     boxed_general(m, n, seed) from the slack basis on the library
                --parent-lib (a build of the parent commit): k_pbox_price1 /
                k_pbox_update1
  p1_free       the same LP with every fifth structural column free (j % 5 == 2:
                no bounds at all), on this build: k_pbox_price_f / k_pbox_update_f
  p1_nofree     the LP of p1_parent on this build (no free column: the parent's
                kernels)
  p1_parent_again, p1_free_again, p1_nofree_again
with the ratios of the kernel times and of the pass rates to p1_parent, and
p1_parent_again over p1_parent as the session's run-to-run spread.

--ranging measures sensitivity ranging instead, one child process
per --kernel-shape: boxed_primal's LP solved to the optimum under steepest edge,
then, after one untimed round, five rounds of spx_refresh_primal_weights,
spx_ranging_cost and spx_ranging_rhs, alternating, with their device times
(spx_pbox_wexact_times, spx_ranging_times), the ratio of the fastest cost ranging
to the fastest exact weight start, and the rates they amount to.  With --k >= 252
the bounded primal loop of a context that never ranges follows (role pbox, twice),
alternating with --parent-root (a built checkout of the parent commit: its package
and its libsimplex.so) when one is given.

--bound-ranging measures bound ranging against cost ranging, one
child process per --kernel-shape: the same LP, context and session as --ranging,
then, after one untimed round, five rounds of spx_ranging_cost and
spx_ranging_bound, alternating, with their device times (spx_ranging_times,
spx_ranging_bound_times) and the ratio of the fastest bound ranging to the
fastest cost ranging.  With --k >= 252 the loops of contexts that never range
follow (role pbox: the bounded primal loop; role dual_box: the boxed dual loop on
tests/dual_box_ref.py boxed), each twice, alternating with --parent-root when one
is given.

--phase1 --primal-pricing steepest --phase1-pricing steepest measures steepest
edge through phase 1 instead, one child per side, the sides
alternating:
  p1_dense      as above: the phase-1 Dantzig pass (k_pbox_vtb, k_pbox_price1, ...)
  p1_se         the same LP with the three flags: the phase-1 steepest-edge pass
                (k_pbox_vtb, k_pbox_price_se1, k_pbox_update1, k_pbox_step_se1,
                k_pbox_tau); price_us is k_pbox_price_se1's, vtb_us the mean of the
                k_pbox_vtb and the k_pbox_tau step (two event pairs per pass)
  pbox_se       as above: the phase-2 steepest-edge pass (k_pbox_price_se) of a
                context that never opted in; with --parent-lib also pbox_se_parent
                and pbox_parent, the same two sides on a build of the parent commit
  p1_dense_again, p1_se_again, pbox_se_again (, pbox_se_parent_again, pbox_parent_again)
The pricing kernels are compared by algorithmic bandwidth (bytes_price / time):
the sides stream different numbers of non-basic slack columns.  With --solve,
whole solves of boxed_general at every --solve-shape from the slack basis,
Dantzig phase 1 / steepest / Dantzig / steepest, each with the CPU certificate.

--free --primal-pricing steepest --phase1-pricing steepest --free-pricing steepest
measures steepest edge with free columns instead, in phase 1,
where the kernel it derives from runs; one child per side, the sides alternating:
  p1_se         boxed_general(m, n, seed) without free columns under steepest edge
                through phase 1: k_pbox_price_se1 / k_pbox_update1 / k_pbox_step_se1
  p1_se_free    the same LP with every fifth structural column free (p1_free's LP)
                and the three opt-ins: k_pbox_price_se_f / k_pbox_update_f /
                k_pbox_step_se_f
  p1_free       that LP under Dantzig: k_pbox_price_f / k_pbox_update_f
  with --parent-lib also p1_se_parent (p1_se on a build of the parent commit: its
  second run over its first is the session's parent-against-itself spread), and the
  loops of contexts that never opt in on both builds: pbox_se, pbox_se_parent,
  pbox, pbox_parent
  ..._again     every side once more
The pricing kernels are compared by time and by algorithmic bandwidth
(bytes_price / time: the sides stream different numbers of non-basic slack
columns).  With --solve, whole solves of tests/primal_lu_ref.py general_lu at
every --solve-shape from the slack basis, Dantzig / steepest / Dantzig /
steepest, each with the CPU certificate (certificate_lu).

--phase1-ratio long measures phase 1's long-step ratio test
instead, one child per side, the sides alternating, each twice:
  p1_dense_textbook / p1_dense_long   boxed_general(m, n, seed) from the slack basis
                under Dantzig, in timed chunks of --phase1-chunk pivots that end
                inside phase 1: the textbook pass, and the pass with k_pbox_long1
                between k_pbox_update1 and k_pbox_step1 (rows passed, passes that
                passed one, the most in one pass)
  p1_se_textbook / p1_se_long         the same under steepest edge through phase 1
  p1_never_parent / p1_never_this     with --parent-root: the textbook pass of a
                context that never opts in, on a build of the parent commit and on
                this build
With --solve, whole solves of boxed_general and general_lu at every --solve-shape
under both entering rules, textbook / long / textbook / long, with pivots,
phase-1 passes, rows passed, seconds and the CPU certificate.

    python tools/pbox_bench.py [--k 1000 --warm 200] [--solve --solve-shape 1024 4096 4 --rows]
                               [--out profiles/pbox_c3.json]
    python tools/pbox_bench.py --phase1 [--out profiles/pbox_phase1_c3.json]
    python tools/pbox_bench.py --primal-pricing steepest [--solve --solve-shape 1024 4096 4
                               --solve-shape 2048 8192 5] [--out profiles/pbox_se_c3.json]
    python tools/pbox_bench.py --warm-resolve --solve-shape 1024 4096 4 --solve-shape 2048 8192 5
                               --kernel-shape 1024 4096 4 --kernel-shape 2048 8192 5 --kernel-shape 4096 16384 5
                               [--out profiles/pbox_wexact.json]
    python tools/pbox_bench.py --free --parent-lib PATH [--out profiles/pbox_lu_c3.json]
    python tools/pbox_bench.py --phase1 --primal-pricing steepest --phase1-pricing steepest [--parent-lib PATH]
                               [--solve --solve-shape 1024 4096 4] [--out profiles/pbox_p1se_c3.json]
    python tools/pbox_bench.py --free --primal-pricing steepest --phase1-pricing steepest --free-pricing steepest
                               [--parent-lib PATH] [--solve --solve-shape 512 2048 4 --solve-shape 1024 4096 4]
                               [--out profiles/pbox_free_se_c3.json]
    python tools/pbox_bench.py --ranging --kernel-shape 1024 4096 4 --kernel-shape 2048 8192 5
                               --kernel-shape 4096 16384 5 [--parent-root DIR] [--out profiles/ranging_c3.json]
    python tools/pbox_bench.py --bound-ranging --kernel-shape 1024 4096 4 --kernel-shape 2048 8192 5
                               --kernel-shape 4096 16384 5 [--parent-root DIR] [--out profiles/bound_ranging_c3.json]
    python tools/pbox_bench.py --phase1-ratio long --warm 20 --k 400 --phase1-chunk 50 [--parent-root DIR]
                               [--solve --solve-shape 512 2048 4 --solve-shape 1024 4096 4]
                               [--out profiles/pbox_p1long_c3.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.environ.get("SPX_BENCH_ROOT") or ROOT)  # (a child of --parent-root: that checkout's package)
sys.path.insert(1, os.path.join(ROOT, "tests"))

PEAK = 8.0e12  # MI355X HBM bytes/s the fractions are quoted against


def measure(make_ctx, k, warm, flips=False):
    """it/s from an untimed context, kernel means from a timing one."""
    with make_ctx(False) as ctx:
        ctx.iterate(warm)
        _, p0 = ctx.iterate(0)
        t0 = time.perf_counter()
        st, p1 = ctx.iterate(k)
        dt = time.perf_counter() - t0
    with make_ctx(True) as ctx:
        ctx.iterate(warm)
        ctx.kernel_times()
        b0 = ctx.info()
        f0 = ctx.primal_flips() if flips else None
        ctx.iterate(k)
        kt = ctx.kernel_times()
        b1 = ctx.info()
        f1 = ctx.primal_flips() if flips else None
    price_us = 1e3 * kt["price_ms"] / max(kt["price_launches"], 1)
    update_us = 1e3 * kt["update_ms"] / max(kt["update_launches"], 1)
    bytes_price = 0.5 * (b0["bytes_price"] + b1["bytes_price"])
    res = {"pivots": p1 - p0, "status": int(st), "it_per_s": round((p1 - p0) / dt, 1),
           "price_us": round(price_us, 2), "update_us": round(update_us, 2),
           "rest_us": round(1e6 * dt / max(p1 - p0, 1) - price_us - update_us, 2),
           "timed_passes": kt["price_launches"], "bytes_price": bytes_price, "bytes_update": b1["bytes_update"],
           "price_TBps": round(bytes_price / (price_us * 1e-6) / 1e12, 3),
           "price_frac_of_8TBps": round(bytes_price / (price_us * 1e-6) / PEAK, 3),
           "update_TBps": round(b1["bytes_update"] / (update_us * 1e-6) / 1e12, 3)}
    if flips:
        res["flip_passes"], res["to_upper"] = f1[0] - f0[0], f1[1] - f0[1]
    return res


def run_primal(a):
    import simplex_method_gpu_amd as spx

    return measure(lambda timing: spx.Context(m=a.m, n=a.n, seed=0, device=0, window=-1, timing=timing), a.k, a.warm)


def run_dual(a):
    import numpy as np

    import dual_ref
    import simplex_method_gpu_amd as spx

    A, b, c = dual_ref.covering(a.m, a.n, a.seed)
    A_cols = np.ascontiguousarray(A.T)
    del A
    return measure(lambda timing: spx.Context(A_cols, b, c, device=0, window=-1, algorithm=spx.ALGO_DUAL,
                                              timing=timing), a.k, a.warm)


def run_pbox(a):
    import numpy as np

    import primal_box_ref
    import simplex_method_gpu_amd as spx

    A, b, c, u = primal_box_ref.boxed_primal(a.m, a.n, a.seed)
    A_cols = np.ascontiguousarray(A.T)
    del A
    return measure(lambda timing: spx.Context(A_cols, b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, upper=u,
                                              timing=timing), a.k, a.warm, flips=True)


def run_pbox_se(a):
    """The Dantzig side's LP under steepest edge; the tau step's mean time from the timing context."""
    import numpy as np

    import primal_box_ref
    import simplex_method_gpu_amd as spx

    A, b, c, u = primal_box_ref.boxed_primal(a.m, a.n, a.seed)
    A_cols = np.ascontiguousarray(A.T)
    del A
    tau = {}

    class Timed:  # (measure() reads kernel_times() itself: the tau events are read around it)
        def __init__(self, timing):
            self.ctx = spx.Context(A_cols, b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, timing=timing,
                                   primal_pricing=spx.PRIMAL_PRICING_STEEPEST)
            self.timing = timing

        def __enter__(self):
            self.ctx.__enter__()
            return self

        def __exit__(self, *exc):
            if self.timing:
                ms, launches = self.last
                tau.update({"tau_us": round(1e3 * ms / max(launches, 1), 2), "tau_launches": launches})
            return self.ctx.__exit__(*exc)

        def kernel_times(self):
            self.last = self.ctx.vtb_times()  # (read and reset with the kernel times: the last read is the timed block)
            return self.ctx.kernel_times()

        def __getattr__(self, name):
            return getattr(self.ctx, name)

    res = measure(Timed, a.k, a.warm, flips=True)
    res.update(tau)
    res["se_lds"] = os.environ.get("SPX_PBOX_SE_LDS", "default")
    return res


def run_pbox_flag(a):
    import numpy as np

    import primal_box_ref
    import simplex_method_gpu_amd as spx

    A, b, c, u = primal_box_ref.boxed_primal(a.m, a.n, a.seed)
    A_cols = np.ascontiguousarray(A.T)
    del A
    res = measure(lambda timing: spx.Context(A_cols, b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, upper=u,
                                             primal_phase1=True, timing=timing), a.k, a.warm, flips=True)
    return res


def with_ratio(ctx, a):
    """--phase1-ratio long: the context under SPX_PRIMAL_RATIO_LONG_STEP.  Under textbook the
    setter is not called: the context never opts in (and a parent build has no such setter)."""
    if a.phase1_ratio == "long":
        import simplex_method_gpu_amd as spx

        ctx.set_primal_phase1_ratio(spx.PRIMAL_RATIO_LONG_STEP)
    return ctx


def long_record(ctx, a):
    rec = {"phase1_ratio": a.phase1_ratio}
    if hasattr(ctx, "primal_long_steps"):
        ls = ctx.primal_long_steps()
        rec.update({"rows_passed": ls[0], "long_passes": ls[1], "most_in_one_pass": ls[2]})
    return rec


def measure_phase1(make_ctx, k, warm, chunk, want_phase2, warm2=0):
    """Phase-1 passes in chunks of `chunk` pivots, at most k pivots: only chunks
    that end with rows still out of bounds count (all their passes are phase-1
    passes).  want_phase2: then on to ninf == 0 and k timed phase-2 pivots."""
    res = {}
    with make_ctx(False) as ctx:
        ctx.iterate(warm)
        ph0 = ctx.primal_phase1()
        res["ninf_entry"], res["ninf_before"] = ph0[2], ph0[3]
        dt = 0.0
        piv = passes = st = 0
        ph = ph0
        while piv < k and ph[3] > 0:
            _, p0 = ctx.iterate(0)
            t0 = time.perf_counter()
            st, p1 = ctx.iterate(chunk)
            d = time.perf_counter() - t0
            nph = ctx.primal_phase1()
            if nph[3] == 0 or int(st) != 0:
                ph = nph
                break
            dt += d
            piv += p1 - p0
            passes += nph[0] - ph[0]
            ph = nph
        res.update({"ninf_after": ph[3], "pivots": piv, "passes": passes, "status": int(st),
                    "it_per_s": round(piv / dt, 1) if dt else None, "passes_per_s": round(passes / dt, 1) if dt else None})
        if hasattr(ctx, "primal_long_steps"):
            ls = ctx.primal_long_steps()
            res.update({"rows_passed": ls[0], "long_passes": ls[1], "most_in_one_pass": ls[2], "phase1_ratio_rule": ls[3]})
        if want_phase2:
            guard = 0
            while ctx.primal_phase1()[3] > 0 and guard < 400:
                st, _ = ctx.iterate(chunk)
                guard += 1
                if int(st) != 0:
                    break
            ph = ctx.primal_phase1()
            rec = {"ninf": ph[3], "phase1_passes_total": ph[0], "phase1_pivots_total": ph[1]}
            if ph[3] == 0 and int(st) == 0:
                ctx.iterate(warm2)
                _, p0 = ctx.iterate(0)
                f0 = ctx.primal_flips()
                t0 = time.perf_counter()
                st, p1 = ctx.iterate(k)
                d = time.perf_counter() - t0
                f1 = ctx.primal_flips()
                rec.update({"warm": warm2, "pivots": p1 - p0, "status": int(st), "it_per_s": round((p1 - p0) / d, 1),
                            "flip_passes": f1[0] - f0[0], "to_upper": f1[1] - f0[1],
                            "passes_per_s": round((p1 - p0 + f1[0] - f0[0]) / d, 1),
                            "phase1_passes_in_block": ctx.primal_phase1()[0] - ph[0]})
            res["phase2_same_context"] = rec
    with make_ctx(True) as ctx:
        ctx.iterate(warm)
        ctx.kernel_times()
        ctx.vtb_times()
        info = ctx.info()
        ph = ctx.primal_phase1()
        n0 = ph[3]
        tp = tu = tv = 0.0
        npass = nv = piv = st = 0
        while piv < k and ph[3] > 0:
            st, _ = ctx.iterate(chunk)
            nph = ctx.primal_phase1()
            kt = ctx.kernel_times()
            vt = ctx.vtb_times()
            if nph[3] == 0 or int(st) != 0:
                break
            tp += kt["price_ms"]
            tu += kt["update_ms"]
            tv += vt[0]
            npass += kt["price_launches"]
            nv += vt[1]
            piv += chunk
            ph = nph
        if npass:
            L, m = info["ld"], info["m"]
            vtb_us, price_us, update_us = 1e3 * tv / nv, 1e3 * tp / npass, 1e3 * tu / npass
            bytes_price = 0.5 * (info["bytes_price"] + ctx.info()["bytes_price"])
            res.update({"bytes_price": bytes_price, "price_TBps": round(bytes_price / (price_us * 1e-6) / 1e12, 3),
                        "vtb_pairs_per_pass": round(nv / npass, 3)})
            rows = 0.5 * (n0 + ph[3])
            bytes_vtb = 8.0 * L * rows
            bytes_dense = 8.0 * L * m
            res.update({"timed_passes": npass, "vtb_us": round(vtb_us, 2), "price_us": round(price_us, 2),
                        "update_us": round(update_us, 2), "w_rows_mean": rows, "w_density": round(rows / m, 4),
                        "bytes_vtb": bytes_vtb, "vtb_TBps": round(bytes_vtb / (vtb_us * 1e-6) / 1e12, 3),
                        "vtb_frac_of_8TBps": round(bytes_vtb / (vtb_us * 1e-6) / PEAK, 3),
                        "vtb_dense_equiv_TBps": round(bytes_dense / (vtb_us * 1e-6) / 1e12, 3),
                        "bytes_update": info["bytes_update"],
                        "update_TBps": round(info["bytes_update"] / (update_us * 1e-6) / 1e12, 3),
                        "update_frac_of_8TBps": round(info["bytes_update"] / (update_us * 1e-6) / PEAK, 3)})
        if want_phase2 and "pivots" in res.get("phase2_same_context", {}):
            # the same phase-2 block under SPX_FLAG_TIMING: which launches its passes are
            guard = 0
            while ctx.primal_phase1()[3] > 0 and guard < 400:
                ctx.iterate(chunk)
                guard += 1
            ctx.iterate(warm2)
            ctx.kernel_times()
            ctx.vtb_times()
            ctx.iterate(k)
            kt = ctx.kernel_times()
            vt = ctx.vtb_times()
            res["phase2_same_context"].update(
                {"timed_passes": kt["price_launches"], "vtb_launches": vt[1],
                 "price_us": round(1e3 * kt["price_ms"] / max(kt["price_launches"], 1), 2),
                 "update_us": round(1e3 * kt["update_ms"] / max(kt["update_launches"], 1), 2)})
    return res


def run_p1_dense(a):
    import numpy as np

    import primal_phase1_ref
    import simplex_method_gpu_amd as spx

    A, b, c, u = primal_phase1_ref.boxed_general(a.m, a.n, a.seed)
    A_cols = np.ascontiguousarray(A.T)
    del A
    return measure_phase1(lambda timing: with_ratio(spx.Context(A_cols, b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, upper=u,
                                                                primal_phase1=True, timing=timing), a),
                          a.k, a.warm, a.phase1_chunk or a.k, False)


def run_p1_se(a):
    """p1_dense's LP with steepest edge through phase 1."""
    import numpy as np

    import primal_phase1_ref
    import simplex_method_gpu_amd as spx

    A, b, c, u = primal_phase1_ref.boxed_general(a.m, a.n, a.seed)
    A_cols = np.ascontiguousarray(A.T)
    del A
    S = spx.PRIMAL_PRICING_STEEPEST
    return measure_phase1(lambda timing: with_ratio(spx.Context(A_cols, b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, upper=u,
                                                                primal_phase1=True, primal_pricing=S, primal_phase1_pricing=S,
                                                                timing=timing), a),
                          a.k, a.warm, a.phase1_chunk or a.k, False)


def _parent_bindings():
    """A build of the parent commit (SPX_LIB) lacks the entry point this package binds since."""
    from simplex_method_gpu_amd import _lib

    _lib.SIGNATURES.pop("spx_set_primal_free_pricing")


def _free_fifth(a):
    """p1_dense's LP with every fifth structural column free: (A_cols, b, c, l, u, free count)."""
    import numpy as np

    import primal_phase1_ref

    A, b, c, u = primal_phase1_ref.boxed_general(a.m, a.n, a.seed)
    ns = a.n - a.m
    fr = np.arange(ns) % 5 == 2
    l = np.zeros(a.n)
    l[:ns][fr] = -np.inf
    u[:ns][fr] = np.inf
    return np.ascontiguousarray(A.T), b, c, l, u, int(fr.sum())


def run_p1_se_free(a):
    """p1_free's LP under steepest edge in both phases, free columns included."""
    import simplex_method_gpu_amd as spx

    A_cols, b, c, l, u, nfree = _free_fifth(a)
    S = spx.PRIMAL_PRICING_STEEPEST
    res = measure_phase1(lambda timing: spx.Context(A_cols, b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, lower=l,
                                                    upper=u, primal_phase1=True, primal_pricing=S,
                                                    primal_phase1_pricing=S, primal_free_pricing=S, timing=timing),
                         a.k, a.warm, a.k, False)
    res["free_columns"] = nfree
    return res


def run_p1_se_parent(a):
    _parent_bindings()
    return run_p1_se(a)


def run_solve_lu(a):
    """Whole solves of general_lu (a fifth of the structural columns free) from the
    slack basis through phase 1, under Dantzig or under steepest edge throughout."""
    import numpy as np

    import primal_lu_ref
    import simplex_method_gpu_amd as spx

    out = []
    steep = a.primal_pricing == "steepest"
    rule = spx.PRIMAL_PRICING_STEEPEST if steep else spx.PRIMAL_PRICING_DANTZIG
    for (m, n, seed) in [tuple(s) for s in a.solve_shape]:
        A, b, c, l, u = primal_lu_ref.general_lu(m, n, seed)
        with spx.Context(np.ascontiguousarray(A.T), b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, lower=l, upper=u,
                         refactor_every=a.refactor, primal_phase1=True, primal_pricing=rule,
                         primal_phase1_pricing=rule, primal_free_pricing=rule) as ctx:
            with_ratio(ctx, a)
            ctx.iterate(20)  # (first-launch costs)
            ctx.reset()
            t0 = time.perf_counter()
            r = ctx.solve()
            dt = time.perf_counter() - t0
            x, up = ctx.primal()
            fl = ctx.primal_flips()
            ph = ctx.primal_phase1()
            lrec = long_record(ctx, a)
        rec = {"m": m, "n": n, "seed": seed, "refactor_every": a.refactor, "primal_pricing": a.primal_pricing,
               "free_columns": int(np.isneginf(l).sum()), "free_basic": int(np.isneginf(l)[r.b_ixs].sum()), **lrec,
               "status": int(r.status), "pivots": r.pivots, "z": r.z, "seconds": round(dt, 4),
               "it_per_s": round(r.pivots / dt, 1), "flip_passes": fl[0], "to_upper": fl[1],
               "phase1_passes": ph[0], "phase1_pivots": ph[1], "phase1_rows": ph[2]}
        if int(r.status) == 1:
            viol, dviol, zc = primal_lu_ref.certificate_lu(A, b, c, l, u, r.b_ixs, up)
            rec.update({"cert_bound_violation": viol, "cert_dual_violation": dviol,
                        "cert_z_rel": abs(zc - r.z) / abs(zc), "cert_ok": bool(viol <= 1e-9 and dviol <= 1e-7)})
        out.append(rec)
    return out


def run_pbox_se_parent(a):
    _parent_bindings()
    return run_pbox_se(a)


def run_pbox_parent(a):
    _parent_bindings()
    return run_pbox(a)


def run_solve_p1(a):
    """Whole solves of boxed_general from the slack basis through phase 1, under
    Dantzig or under steepest edge in both phases."""
    import numpy as np

    import primal_phase1_ref
    import simplex_method_gpu_amd as spx

    out = []
    steep = a.primal_pricing == "steepest"
    rule = spx.PRIMAL_PRICING_STEEPEST if steep else spx.PRIMAL_PRICING_DANTZIG
    for (m, n, seed) in [tuple(s) for s in a.solve_shape]:
        A, b, c, u = primal_phase1_ref.boxed_general(m, n, seed)
        with spx.Context(np.ascontiguousarray(A.T), b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, upper=u,
                         refactor_every=a.refactor, primal_phase1=True, primal_pricing=rule,
                         primal_phase1_pricing=rule) as ctx:
            with_ratio(ctx, a)
            ctx.iterate(20)  # (first-launch costs)
            ctx.reset()
            t0 = time.perf_counter()
            r = ctx.solve()
            dt = time.perf_counter() - t0
            x, up = ctx.primal()
            fl = ctx.primal_flips()
            ph = ctx.primal_phase1()
            lrec = long_record(ctx, a)
        rec = {"m": m, "n": n, "seed": seed, "refactor_every": a.refactor, "primal_pricing": a.primal_pricing, **lrec,
               "phase1_pricing": a.primal_pricing, "status": int(r.status), "pivots": r.pivots, "z": r.z,
               "seconds": round(dt, 4), "it_per_s": round(r.pivots / dt, 1), "flip_passes": fl[0], "to_upper": fl[1],
               "phase1_passes": ph[0], "phase1_pivots": ph[1], "phase1_rows": ph[2]}
        if int(r.status) == 1:
            viol, dviol, zc = primal_phase1_ref.certificate(A, b, c, u, r.b_ixs, up)
            rec.update({"cert_bound_violation": viol, "cert_dual_violation": dviol,
                        "cert_z_rel": abs(zc - r.z) / abs(zc), "cert_ok": bool(viol <= 1e-9 and dviol <= 1e-7)})
        out.append(rec)
    return out


def run_p1_free(a):
    """p1_dense's LP with every fifth structural column free."""
    import simplex_method_gpu_amd as spx

    A_cols, b, c, l, u, nfree = _free_fifth(a)
    res = measure_phase1(lambda timing: spx.Context(A_cols, b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, lower=l,
                                                    upper=u, primal_phase1=True, timing=timing), a.k, a.warm, a.k, False)
    res["free_columns"] = nfree
    return res


def run_p1_parent(a):
    """p1_dense on a build of the parent commit (SPX_LIB)."""
    _parent_bindings()
    return run_p1_dense(a)


def run_p1_sparse(a):
    import numpy as np

    import primal_box_ref
    import simplex_method_gpu_amd as spx

    A, b, c, u = primal_box_ref.boxed_primal(a.m, a.n, a.seed)
    ns = a.n - a.m
    ge = np.arange(a.m) % a.sparse_every == 1  # a.x <= b_i becomes a.x >= 0.1 b_i: violated at the slack basis
    A[ge, :ns] *= -1.0
    b[ge] *= -0.1
    u[ns:][ge] = np.inf
    A_cols = np.ascontiguousarray(A.T)
    del A
    return measure_phase1(lambda timing: spx.Context(A_cols, b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, upper=u,
                                                     primal_phase1=True, timing=timing), a.k, 1, a.sparse_chunk, True, a.warm)  # (warm 1: the entry check)


def bounds_as_rows(A, b, c, u):
    """The bounded LP with every finite bound as a row of its own (b stays >= 0
    where the slack basis is feasible for the bounded LP)."""
    import numpy as np

    m, n = A.shape
    ns = n - m
    rows, rhs = [], []
    for j in np.flatnonzero(np.isfinite(u[:ns])):  # x_j <= u_j
        r = np.zeros(ns)
        r[j] = 1.0
        rows.append(r)
        rhs.append(u[j])
    for k in np.flatnonzero(np.isfinite(u[ns:])):  # s_k <= u_k: -a_k.x <= u_k - b_k
        rows.append(-A[k, :ns])
        rhs.append(u[ns + k] - b[k])
    G = np.vstack([A[:, :ns]] + [np.asarray(rows)]) if rows else A[:, :ns]
    h = np.concatenate([b, np.asarray(rhs)])
    m2 = G.shape[0]
    A2 = np.hstack([G, np.eye(m2)])
    return A2, h, np.concatenate([c[:ns], np.zeros(m2)])


def run_solve(a):
    """Whole solves to the optimum: the first after a warm-up of the same context."""
    import numpy as np

    import primal_box_ref
    import simplex_method_gpu_amd as spx

    out = []
    rule = spx.PRIMAL_PRICING_STEEPEST if a.primal_pricing == "steepest" else spx.PRIMAL_PRICING_DANTZIG
    for (m, n, seed) in [tuple(s) for s in a.solve_shape]:
        A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
        with spx.Context(np.ascontiguousarray(A.T), b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, upper=u,
                         refactor_every=a.refactor, primal_pricing=rule) as ctx:
            ctx.iterate(20)  # (first-launch costs)
            ctx.reset()
            t0 = time.perf_counter()
            r = ctx.solve()
            dt = time.perf_counter() - t0
            x, up = ctx.primal()
            fl = ctx.primal_flips()
        rec = {"m": m, "n": n, "seed": seed, "refactor_every": a.refactor, "primal_pricing": a.primal_pricing,
               "status": int(r.status),
               "pivots": r.pivots, "z": r.z, "seconds": round(dt, 4), "it_per_s": round(r.pivots / dt, 1),
               "flip_passes": fl[0], "to_upper": fl[1], "at_upper": int(up.sum())}
        if int(r.status) == 1:
            viol, dviol, zc = primal_box_ref.certificate(A, b, c, u, r.b_ixs, up)
            rec.update({"cert_bound_violation": viol, "cert_dual_violation": dviol,
                        "cert_z_rel": abs(zc - r.z) / abs(zc), "cert_ok": bool(viol <= 1e-9 and dviol <= 1e-7)})
        if a.rows:
            A2, b2, c2 = bounds_as_rows(A, b, c, u)
            m2, n2 = A2.shape
            with spx.Context(np.ascontiguousarray(A2.T), b2, c2, device=0, ratio_test=spx.RATIO_GUARDED,
                             refactor_every=a.refactor) as ctx:
                ctx.iterate(20)
                ctx.reset()
                t0 = time.perf_counter()
                r2 = ctx.solve()
                dt2 = time.perf_counter() - t0
            rec["rows"] = {"m": m2, "n": n2, "status": int(r2.status), "pivots": r2.pivots, "z": r2.z,
                           "seconds": round(dt2, 4), "z_rel_to_bounded": abs(r2.z - r.z) / abs(r.z)}
        out.append(rec)
    return out


def run_warm_resolve(a):
    """One shape (the first --solve-shape): the re-solve under both start modes, alternating."""
    import numpy as np

    import dual_box_ref
    import primal_box_ref
    import simplex_method_gpu_amd as spx

    m, n, seed = a.solve_shape[0]
    A, b, c, u = dual_box_ref.boxed(m, n, seed, False)
    c2 = primal_box_ref.cost_variant(c, n - m, seed)
    A_cols = np.ascontiguousarray(A.T)

    def sequence(mode, timing=False):
        with spx.Context(A_cols, b, c, device=0, window=-1, algorithm=spx.ALGO_DUAL,
                         dual_pricing=spx.DUAL_PRICING_STEEPEST, upper=u, primal_pricing=spx.PRIMAL_PRICING_STEEPEST,
                         primal_weights=mode, timing=timing) as ctx:
            t0 = time.perf_counter()
            r0 = ctx.solve()
            t1 = time.perf_counter()
            ctx.set_cost(c2)
            ctx.set_algorithm(spx.ALGO_PRIMAL_BOX)
            t2 = time.perf_counter()
            r1 = ctx.solve()
            t3 = time.perf_counter()
            up = ctx.primal()[1]
            fl = ctx.primal_flips()
            rec = {"mode": "exact" if mode == spx.PRIMAL_WEIGHTS_EXACT else "reference", "dual_status": int(r0.status),
                   "dual_pivots": r0.pivots, "dual_seconds": round(t1 - t0, 4), "status": int(r1.status),
                   "pivots": r1.pivots - r0.pivots, "flip_passes": fl[0], "to_upper": fl[1], "z": r1.z,
                   "seconds": round(t3 - t2, 5)}
            if timing:
                ms, k = ctx.wexact_times()
                rec.update({"wexact_ms": round(ms, 4), "wexact_launches": k})
        if int(r1.status) == 1:
            viol, dviol, _ = primal_box_ref.certificate(A, b, c2, u, r1.b_ixs, up)
            rec["cert_ok"] = bool(viol <= 1e-9 and dviol <= 1e-7)
        return rec

    sequence(spx.PRIMAL_WEIGHTS_EXACT)  # first-launch costs
    runs = [sequence(mode) for mode in (spx.PRIMAL_WEIGHTS_REFERENCE, spx.PRIMAL_WEIGHTS_EXACT,
                                        spx.PRIMAL_WEIGHTS_REFERENCE, spx.PRIMAL_WEIGHTS_EXACT)]
    timed = sequence(spx.PRIMAL_WEIGHTS_EXACT, timing=True)
    ref_s = min(runs[0]["seconds"], runs[2]["seconds"])
    ex_s = min(runs[1]["seconds"], runs[3]["seconds"])
    return {"m": m, "n": n, "seed": seed, "runs": runs, "exact_timed": timed,
            "pivot_ratio": round(runs[0]["pivots"] / max(runs[1]["pivots"], 1), 2),
            "time_ratio": round(ref_s / ex_s, 2),
            "accepted": bool(all(runs[i + 1]["pivots"] < runs[i]["pivots"] and runs[i + 1]["seconds"] < runs[i]["seconds"]
                                 for i in (0, 2)))}


def run_wexact_kernel(a):
    """One shape (the first --kernel-shape): the exact recomputation's device time."""
    import numpy as np

    import primal_box_ref
    import simplex_method_gpu_amd as spx

    m, n, seed = a.kernel_shape[0]
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    A_cols = np.ascontiguousarray(A.T)
    del A
    with spx.Context(A_cols, b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, timing=True,
                     primal_pricing=spx.PRIMAL_PRICING_STEEPEST) as ctx:
        ctx.iterate(a.warm)
        ctx.wexact_times()
        times = []
        for _ in range(5):
            ctx.refresh_primal_weights()
            times.append(round(ctx.wexact_times()[0], 4))
        nb_slack = int(np.sum(~np.isin(np.arange(n - m, n), ctx.state()["b_ixs"])))
    with spx.Context(A_cols, b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, upper=u,
                     primal_pricing=spx.PRIMAL_PRICING_STEEPEST) as ctx:
        ctx.iterate(a.warm)
        f0 = ctx.primal_flips()
        _, p0 = ctx.iterate(0)
        t0 = time.perf_counter()
        _, p1 = ctx.iterate(a.k)
        dt = time.perf_counter() - t0
        f1 = ctx.primal_flips()
    passes = p1 - p0 + f1[0] - f0[0]
    pass_us = 1e6 * dt / max(passes, 1)
    best = min(times)
    flops = 2.0 * m * m * (n - m)
    return {"m": m, "n": n, "seed": seed, "warm": a.warm, "wexact_ms": times, "wexact_ms_best": best,
            "nonbasic_slacks": nb_slack, "flops_all_listed": flops,
            "fp64_TFLOPs": round(flops / (best * 1e-3) / 1e12, 2), "se_pass_us": round(pass_us, 2),
            "se_passes_timed": passes, "start_in_se_passes": round(best * 1e3 / pass_us, 1)}


def run_ranging_kernel(a):
    """One shape (the first --kernel-shape): boxed_primal's LP solved to the optimum
    under steepest edge, then five rounds of spx_refresh_primal_weights,
    spx_ranging_cost and spx_ranging_rhs, alternating, with their device times."""
    import numpy as np

    import primal_box_ref
    import simplex_method_gpu_amd as spx

    m, n, seed = a.kernel_shape[0]
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    A_cols = np.ascontiguousarray(A.T)
    del A
    with spx.Context(A_cols, b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, timing=True,
                     primal_pricing=spx.PRIMAL_PRICING_STEEPEST) as ctx:
        t0 = time.perf_counter()
        r = ctx.solve()
        solve_s = time.perf_counter() - t0
        if r.status != spx.SolveStatus.OptimumFound:
            raise SystemExit(f"{m}x{n}: the solve ended with {r.status!r}")
        ctx.refresh_primal_weights()  # first launches: untimed
        ctx.cost_ranging()
        ctx.rhs_ranging()
        ctx.wexact_times()
        ctx.ranging_times()
        wx, cost, rhs = [], [], []
        for _ in range(5):
            ctx.refresh_primal_weights()
            wx.append(round(ctx.wexact_times()[0], 4))
            g = ctx.cost_ranging()
            h = ctx.rhs_ranging()
            (tc, tr), _ = ctx.ranging_times()
            cost.append(round(tc, 4))
            rhs.append(round(tr, 4))
        nb_slack = int(np.sum(~np.isin(np.arange(n - m, n), r.b_ixs)))
    flops = 2.0 * m * m * (n - m)
    return {"m": m, "n": n, "seed": seed, "pivots": r.pivots, "solve_s": round(solve_s, 3), "nonbasic_slacks": nb_slack,
            "wexact_ms": wx, "cost_ms": cost, "rhs_ms": rhs, "wexact_ms_best": min(wx), "cost_ms_best": min(cost),
            "rhs_ms_best": min(rhs), "cost_over_wexact": round(min(cost) / min(wx), 3),
            "cost_fp64_TFLOPs": round(flops / (min(cost) * 1e-3) / 1e12, 2),
            "rhs_binv_TBps": round(2.0 * 8.0 * m * m / (min(rhs) * 1e-3) / 1e12, 3),  # materialise + one stream
            "finite_cost_limits": int(np.isfinite(g.down).sum() + np.isfinite(g.up).sum()),
            "finite_rhs_limits": int(np.isfinite(h.down).sum() + np.isfinite(h.up).sum())}


def run_bound_ranging_kernel(a):
    """One shape (the first --kernel-shape): run_ranging_kernel's LP and context, then
    five rounds of spx_ranging_cost and spx_ranging_bound, alternating, with their
    device times."""
    import numpy as np

    import primal_box_ref
    import simplex_method_gpu_amd as spx

    m, n, seed = a.kernel_shape[0]
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    A_cols = np.ascontiguousarray(A.T)
    del A
    with spx.Context(A_cols, b, c, device=0, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, timing=True,
                     primal_pricing=spx.PRIMAL_PRICING_STEEPEST) as ctx:
        t0 = time.perf_counter()
        r = ctx.solve()
        solve_s = time.perf_counter() - t0
        if r.status != spx.SolveStatus.OptimumFound:
            raise SystemExit(f"{m}x{n}: the solve ended with {r.status!r}")
        ctx.cost_ranging()  # first launches: untimed
        ctx.bound_ranging()
        ctx.ranging_times()
        ctx.bound_ranging_times()
        cost, bound = [], []
        for _ in range(5):
            ctx.cost_ranging()
            cost.append(round(ctx.ranging_times()[0][0], 4))
            g = ctx.bound_ranging()
            bound.append(round(ctx.bound_ranging_times()[0], 4))
        nb = ~np.isin(np.arange(n), r.b_ixs)
    flops = 2.0 * m * m * (n - m)
    return {"m": m, "n": n, "seed": seed, "pivots": r.pivots, "solve_s": round(solve_s, 3),
            "cost_ms": cost, "bound_ms": bound, "cost_ms_best": min(cost), "bound_ms_best": min(bound),
            "bound_over_cost": round(min(bound) / min(cost), 3),
            "bound_fp64_TFLOPs": round(flops / (min(bound) * 1e-3) / 1e12, 2),
            "finite_bound_limits": int(np.isfinite(g.down[nb]).sum() + np.isfinite(g.up[nb]).sum()),
            "side1_blockers": sum(int(np.sum((k[nb] >= 0) & (k[nb] % 2 == 1))) for k in (g.leave_down, g.leave_up)),
            "own_bound_winners": sum(int(np.sum(k[nb] == -2)) for k in (g.leave_down, g.leave_up))}


def run_dual_box(a):
    """The boxed dual loop (tests/dual_box_ref.py boxed) of a context that never ranges."""
    import numpy as np

    import dual_box_ref
    import simplex_method_gpu_amd as spx

    A, b, c, u = dual_box_ref.boxed(a.m, a.n, a.seed)
    A_cols = np.ascontiguousarray(A.T)
    del A
    return measure(lambda timing: spx.Context(A_cols, b, c, device=0, window=-1, algorithm=spx.ALGO_DUAL, upper=u,
                                              timing=timing), a.k, a.warm)


def child(a, role, pricing="dantzig", se_lds=None, lib=None, root=None, ratio="textbook"):
    env = dict(os.environ)
    if root is not None:
        env["SPX_BENCH_ROOT"] = os.path.abspath(root)
    if se_lds is not None:
        env["SPX_PBOX_SE_LDS"] = str(se_lds)
    if lib is not None:
        env["SPX_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--role", role, "--primal-pricing", pricing, "--m", str(a.m), "--n", str(a.n),
           "--seed", str(a.seed), "--k", str(a.k), "--warm", str(a.warm), "--refactor", str(a.refactor),
           "--sparse-every", str(a.sparse_every), "--sparse-chunk", str(a.sparse_chunk),
           "--phase1-ratio", ratio, "--phase1-chunk", str(a.phase1_chunk)]
    if a.rows:
        cmd.append("--rows")
    for shape in a.solve_shape:
        cmd += ["--solve-shape"] + [str(v) for v in shape]
    for shape in a.kernel_shape:
        cmd += ["--kernel-shape"] + [str(v) for v in shape]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    if out.returncode != 0:
        sys.stderr.write(out.stdout + out.stderr)
        raise SystemExit(f"{role} run failed ({out.returncode})")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--solve-shape", type=int, nargs=3, action="append", default=[], metavar=("M", "N", "SEED"))
    ap.add_argument("--rows", action="store_true", help="with --solve: the bounds as rows on the windowed primal loop too")
    ap.add_argument("--refactor", type=int, default=500)
    ap.add_argument("--phase1", action="store_true", help="the phase-1 sides instead (DESIGN.md 7f)")
    ap.add_argument("--sparse-every", type=int, default=100, help="p1_sparse: every this many rows one starts violated")
    ap.add_argument("--sparse-chunk", type=int, default=10, help="p1_sparse: pivots per timed chunk")
    ap.add_argument("--primal-pricing", default="dantzig", choices=["dantzig", "steepest"],
                    help="steepest: the steepest-edge sides against the Dantzig loop instead (DESIGN.md 7h)")
    ap.add_argument("--phase1-pricing", default="dantzig", choices=["dantzig", "steepest"],
                    help="with --phase1 --primal-pricing steepest: steepest edge through phase 1 (DESIGN.md 7l)")
    ap.add_argument("--warm-resolve", action="store_true",
                    help="the exact weight start of a warm basis instead (DESIGN.md 7i)")
    ap.add_argument("--kernel-shape", type=int, nargs=3, action="append", default=[], metavar=("M", "N", "SEED"),
                    help="with --warm-resolve: shapes at which the exact recomputation alone is timed")
    ap.add_argument("--free", action="store_true", help="the free-column kernels against the parent build instead (DESIGN.md 7j)")
    ap.add_argument("--parent-lib", default=None, help="with --free: libsimplex.so built from the parent commit")
    ap.add_argument("--role", default=None,
                    choices=[None, "primal", "dual", "pbox", "solve", "pbox_flag", "p1_dense", "p1_sparse", "pbox_se",
                             "warm_resolve", "wexact_kernel", "p1_free", "p1_parent", "ranging_kernel", "p1_se",
                             "pbox_se_parent", "pbox_parent", "solve_p1", "p1_se_free", "p1_se_parent", "solve_lu",
                             "bound_ranging_kernel", "dual_box"])
    ap.add_argument("--free-pricing", default="dantzig", choices=["dantzig", "steepest"],
                    help="with --free --primal-pricing steepest: steepest edge with free columns (DESIGN.md 7m)")
    ap.add_argument("--parent-root", default=None,
                    help="with --ranging: a built checkout of the parent commit (its package and its libsimplex.so)")
    ap.add_argument("--ranging", action="store_true",
                    help="sensitivity ranging against the exact weight start instead (DESIGN.md 7k)")
    ap.add_argument("--bound-ranging", action="store_true",
                    help="bound ranging against cost ranging instead (DESIGN.md 7n); --parent-root as with --ranging")
    ap.add_argument("--phase1-ratio", default="textbook", choices=["textbook", "long"],
                    help="long: phase 1's long-step ratio test against the textbook one instead (DESIGN.md 7o); "
                         "--parent-root as with --ranging")
    ap.add_argument("--phase1-chunk", type=int, default=0,
                    help="p1_dense / p1_se: pivots per timed chunk (0: --k, one chunk)")
    a = ap.parse_args()
    if a.role:  # a child: one side, one JSON line
        run = {"primal": run_primal, "dual": run_dual, "pbox": run_pbox, "solve": run_solve,
               "pbox_flag": run_pbox_flag, "p1_dense": run_p1_dense, "p1_sparse": run_p1_sparse,
               "pbox_se": run_pbox_se, "warm_resolve": run_warm_resolve, "wexact_kernel": run_wexact_kernel,
               "p1_free": run_p1_free, "p1_parent": run_p1_parent, "ranging_kernel": run_ranging_kernel,
               "p1_se": run_p1_se, "pbox_se_parent": run_pbox_se_parent, "pbox_parent": run_pbox_parent,
               "solve_p1": run_solve_p1, "p1_se_free": run_p1_se_free, "p1_se_parent": run_p1_se_parent,
               "solve_lu": run_solve_lu, "bound_ranging_kernel": run_bound_ranging_kernel,
               "dual_box": run_dual_box}[a.role]
        print(json.dumps(run(a)), flush=True)
        return
    if a.phase1_ratio == "long":
        res = {"m": a.m, "n": a.n, "k": a.k, "warm": a.warm, "seed": a.seed, "phase1_chunk": a.phase1_chunk}

        def side(key, role, pricing, **kw):
            res[key] = child(a, role, pricing, **kw)
            sys.stderr.write(f"{key}: {json.dumps(res[key])}\n")
            sys.stderr.flush()

        # the phase-1 pass under both ratio tests and both entering rules, alternating
        for again in ("", "_again"):
            for role, pricing in (("p1_dense", "dantzig"), ("p1_se", "steepest")):
                for ratio in ("textbook", "long"):
                    side(f"{role}_{ratio}{again}", role, pricing, ratio=ratio)
        res["long_over_textbook_passes_per_s"] = {
            f"{role}{ag}": round(res[f"{role}_long{ag}"]["passes_per_s"] / res[f"{role}_textbook{ag}"]["passes_per_s"], 4)
            for role in ("p1_dense", "p1_se") for ag in ("", "_again")
            if res[f"{role}_long{ag}"]["passes_per_s"] and res[f"{role}_textbook{ag}"]["passes_per_s"]}
        if a.parent_root:  # a context that never opts in, against a build of the parent commit
            for again in ("", "_again"):
                for name, root in (("parent", a.parent_root), ("this", None)):
                    side(f"p1_never_{name}{again}", "p1_dense", "dantzig", root=root)
            base = res["p1_never_parent"]["passes_per_s"]
            res["never_passes_per_s_over_parent"] = {k: round(res[k]["passes_per_s"] / base, 4)
                                                     for k in ("p1_never_this", "p1_never_parent_again", "p1_never_this_again")}
        if a.solve and a.solve_shape:
            res["solve"] = []
            for family, role in (("boxed_general", "solve_p1"), ("general_lu", "solve_lu")):
                for pricing in ("dantzig", "steepest"):
                    runs = [child(a, role, pricing, ratio=r) for r in ("textbook", "long", "textbook", "long")]
                    for i in range(len(a.solve_shape)):
                        tb, lg = runs[0][i], runs[1][i]
                        rec = {"family": family, "primal_pricing": pricing, "textbook": tb, "long": lg,
                               "textbook_again": runs[2][i], "long_again": runs[3][i],
                               "pivot_ratio": round(tb["pivots"] / lg["pivots"], 2),
                               "phase1_pass_ratio": round(tb["phase1_passes"] / max(lg["phase1_passes"], 1), 2),
                               "time_ratio": round(tb["seconds"] / lg["seconds"], 2),
                               "time_ratio_again": round(runs[2][i]["seconds"] / runs[3][i]["seconds"], 2),
                               "certificates_ok": bool(all(r[i].get("cert_ok") for r in runs))}
                        res["solve"].append(rec)
                        sys.stderr.write(f"solve: {json.dumps(rec)}\n")
                        sys.stderr.flush()
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    if a.bound_ranging:
        import copy

        res = {"k": a.k, "warm": a.warm, "kernel": []}
        for shape in a.kernel_shape:
            one = copy.copy(a)
            one.solve_shape, one.kernel_shape = [], [shape]
            res["kernel"].append(child(one, "bound_ranging_kernel", "steepest"))
            sys.stderr.write(f"bound ranging {shape}: {json.dumps(res['kernel'][-1])}\n")
            sys.stderr.flush()
        if a.k >= 252:  # the loops of contexts that never range, against the parent build when one is given
            roots = (("parent", a.parent_root), ("this", None)) if a.parent_root else (("this", None),)
            for role in ("pbox", "dual_box"):
                for again in ("", "_again"):
                    for name, root in roots:
                        key = f"{role}_{name}{again}"
                        res[key] = child(a, role, root=root)
                        sys.stderr.write(f"{key}: {json.dumps(res[key])}\n")
                        sys.stderr.flush()
                if a.parent_root:
                    base = res[f"{role}_parent"]["it_per_s"]
                    res[f"{role}_it_per_s_over_parent"] = {
                        k: round(res[k]["it_per_s"] / base, 4)
                        for k in (f"{role}_this", f"{role}_parent_again", f"{role}_this_again")}
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    if a.ranging:
        import copy

        res = {"k": a.k, "warm": a.warm, "kernel": []}
        for shape in a.kernel_shape:
            one = copy.copy(a)
            one.solve_shape, one.kernel_shape = [], [shape]
            res["kernel"].append(child(one, "ranging_kernel", "steepest"))
            sys.stderr.write(f"ranging {shape}: {json.dumps(res['kernel'][-1])}\n")
            sys.stderr.flush()
        if a.k >= 252:  # the loop of a context that never ranges, against the parent build when one is given
            roots = (("parent", a.parent_root), ("this", None)) if a.parent_root else (("this", None),)
            for again in ("", "_again"):
                for name, root in roots:
                    key = f"pbox_{name}{again}"
                    res[key] = child(a, "pbox", root=root)
                    sys.stderr.write(f"{key}: {json.dumps(res[key])}\n")
                    sys.stderr.flush()
            if a.parent_root:
                base = res["pbox_parent"]["it_per_s"]
                res["it_per_s_over_parent"] = {k: round(res[k]["it_per_s"] / base, 4)
                                               for k in ("pbox_this", "pbox_parent_again", "pbox_this_again")}
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    if a.warm_resolve:
        import copy

        res = {"k": a.k, "warm": a.warm, "resolve": [], "kernel": []}
        for key, role, shapes in (("kernel", "wexact_kernel", a.kernel_shape), ("resolve", "warm_resolve", a.solve_shape)):
            for shape in shapes:
                one = copy.copy(a)
                one.solve_shape, one.kernel_shape = ([shape], []) if key == "resolve" else ([], [shape])
                res[key].append(child(one, role, "steepest"))
                sys.stderr.write(f"{key} {shape}: {json.dumps(res[key][-1])}\n")
                sys.stderr.flush()
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    if a.k < 252:
        ap.error("--k: at least 252 timed pivots")
    res = {"m": a.m, "n": a.n, "k": a.k, "warm": a.warm, "seed": a.seed}
    if a.free and a.primal_pricing == "steepest":
        if a.phase1_pricing != "steepest" or a.free_pricing != "steepest":
            ap.error("--free --primal-pricing steepest needs --phase1-pricing steepest and --free-pricing steepest (the "
                     "library refuses it otherwise)")
        if a.parent_lib and not os.path.exists(a.parent_lib):
            ap.error("--parent-lib: no such file")
        sides = [("p1_se", "p1_se"), ("p1_se_free", "p1_se_free"), ("p1_free", "p1_free")]
        if a.parent_lib:
            sides += [("p1_se_parent", "p1_se_parent"), ("pbox_se", "pbox_se"), ("pbox_se_parent", "pbox_se_parent"),
                      ("pbox", "pbox"), ("pbox_parent", "pbox_parent")]
        for again in ("", "_again"):
            for key, role in sides:
                res[key + again] = child(a, role, "steepest" if "se" in role else "dantzig",
                                         lib=a.parent_lib if role.endswith("_parent") else None)
                sys.stderr.write(f"{key + again}: {json.dumps(res[key + again])}\n")
                sys.stderr.flush()
        keys = ("price_us", "price_TBps", "update_us", "vtb_us", "passes_per_s")
        for ag in ("", "_again"):
            q = res["p1_se_free" + ag]
            res["p1_se_free_over_p1_se" + ag] = {k: round(q[k] / res["p1_se" + ag][k], 4) for k in keys}
            res["p1_se_free_over_p1_free" + ag] = {k: round(q[k] / res["p1_free" + ag][k], 4) for k in keys}
        res["again_over_first"] = {k: {f: round(res[k + "_again"][f] / res[k][f], 4) for f in keys}
                                   for k in ("p1_se", "p1_se_free", "p1_free")}
        if a.parent_lib:
            res["p1_se_parent_again_over_p1_se_parent"] = {k: round(res["p1_se_parent_again"][k] / res["p1_se_parent"][k], 4)
                                                           for k in keys}
            res["p1_se_over_p1_se_parent"] = {ag or "first": {k: round(res["p1_se" + ag][k] / res["p1_se_parent" + ag][k], 4)
                                                              for k in keys} for ag in ("", "_again")}
            res["this_over_parent_it_per_s"] = {f"{k}{ag}": round(res[k + ag]["it_per_s"] / res[k + "_parent" + ag]["it_per_s"], 4)
                                                for k in ("pbox_se", "pbox") for ag in ("", "_again")}
            res["parent_again_over_parent_it_per_s"] = {k: round(res[k + "_parent_again"]["it_per_s"]
                                                                 / res[k + "_parent"]["it_per_s"], 4) for k in ("pbox_se", "pbox")}
        if a.solve and a.solve_shape:
            runs = [child(a, "solve_lu", rule) for rule in ("dantzig", "steepest", "dantzig", "steepest")]
            res["solve"] = []
            for i in range(len(a.solve_shape)):
                dz, se = runs[0][i], runs[1][i]
                res["solve"].append({"dantzig": dz, "steepest": se, "dantzig_again": runs[2][i],
                                     "steepest_again": runs[3][i],
                                     "pivot_ratio": round(dz["pivots"] / se["pivots"], 2),
                                     "time_ratio": round(dz["seconds"] / se["seconds"], 2),
                                     "certificates_ok": bool(all(r[i].get("cert_ok") for r in runs))})
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    if a.phase1 and a.primal_pricing == "steepest":
        if a.phase1_pricing != "steepest":
            ap.error("--phase1 --primal-pricing steepest needs --phase1-pricing steepest (the library refuses it otherwise)")
        if a.parent_lib and not os.path.exists(a.parent_lib):
            ap.error("--parent-lib: no such file")
        sides = [("p1_dense", "p1_dense"), ("p1_se", "p1_se"), ("pbox_se", "pbox_se")]
        if a.parent_lib:
            sides += [("pbox_se_parent", "pbox_se_parent"), ("pbox", "pbox"), ("pbox_parent", "pbox_parent")]
        for again in ("", "_again"):
            for key, role in sides:
                res[key + again] = child(a, role, "steepest" if "se" in role else "dantzig",
                                         lib=a.parent_lib if role.endswith("_parent") else None)
                sys.stderr.write(f"{key + again}: {json.dumps(res[key + again])}\n")
                sys.stderr.flush()
        d, q, w = res["p1_dense"], res["p1_se"], res["pbox_se"]
        res["p1_se_over_p1_dense"] = {k: round(q[k] / d[k], 3) for k in ("passes_per_s", "price_us", "update_us")}
        res["p1_se_over_pbox_se"] = {"pass_rate": round(q["passes_per_s"] / w["it_per_s"], 3),
                                     "price_TBps": round(q["price_TBps"] / w["price_TBps"], 4),
                                     "price_TBps_again": round(res["p1_se_again"]["price_TBps"]
                                                               / res["pbox_se_again"]["price_TBps"], 4)}
        res["again_over_first"] = {k: round(res[k + "_again"][f] / res[k][f], 4)
                                   for k, f in (("p1_dense", "passes_per_s"), ("p1_se", "passes_per_s"),
                                                ("pbox_se", "it_per_s"))}
        if a.parent_lib:
            res["this_over_parent_it_per_s"] = {f"{k}{ag}": round(res[k + ag]["it_per_s"] / res[k + "_parent" + ag]["it_per_s"], 4)
                                                for k in ("pbox_se", "pbox") for ag in ("", "_again")}
            res["parent_again_over_parent_it_per_s"] = {k: round(res[k + "_parent_again"]["it_per_s"]
                                                                 / res[k + "_parent"]["it_per_s"], 4) for k in ("pbox_se", "pbox")}
        if a.solve and a.solve_shape:
            runs = [child(a, "solve_p1", rule) for rule in ("dantzig", "steepest", "dantzig", "steepest")]
            res["solve"] = []
            for i in range(len(a.solve_shape)):
                dz, se = runs[0][i], runs[1][i]
                res["solve"].append({"dantzig": dz, "steepest": se, "dantzig_again": runs[2][i],
                                     "steepest_again": runs[3][i],
                                     "pivot_ratio": round(dz["pivots"] / se["pivots"], 2),
                                     "time_ratio": round(dz["seconds"] / se["seconds"], 2),
                                     "accepted": bool(all(runs[j + 1][i]["pivots"] < runs[j][i]["pivots"]
                                                          and runs[j + 1][i]["seconds"] < runs[j][i]["seconds"]
                                                          for j in (0, 2))
                                                      and all(r[i].get("cert_ok") for r in runs))})
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    if a.primal_pricing == "steepest":
        for key, role, lds in (("pbox", "pbox", None), ("pbox_se", "pbox_se", None), ("pbox_se_lds1", "pbox_se", 1),
                               ("pbox_se_lds0", "pbox_se", 0), ("pbox_again", "pbox", None),
                               ("pbox_se_again", "pbox_se", None)):
            res[key] = child(a, role, "steepest" if role == "pbox_se" else "dantzig", lds)
            sys.stderr.write(f"{key}: {json.dumps(res[key])}\n")
            sys.stderr.flush()
        d, q = res["pbox"], res["pbox_se"]
        res["se_over_dantzig"] = {k: round(q[k] / d[k], 3) for k in ("price_us", "update_us", "it_per_s")}
        if a.solve and a.solve_shape:
            runs = [child(a, "solve", rule) for rule in ("dantzig", "steepest", "dantzig", "steepest")]
            res["solve"] = []
            for i in range(len(a.solve_shape)):
                dz, se = runs[0][i], runs[1][i]
                res["solve"].append({"dantzig": dz, "steepest": se, "dantzig_again": runs[2][i],
                                     "steepest_again": runs[3][i],
                                     "pivot_ratio": round(dz["pivots"] / se["pivots"], 2),
                                     "time_ratio": round(dz["seconds"] / se["seconds"], 2)})
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    if a.free:
        if not a.parent_lib or not os.path.exists(a.parent_lib):
            ap.error("--free needs --parent-lib: a libsimplex.so built from the parent commit")
        for key, role in (("p1_parent", "p1_parent"), ("p1_free", "p1_free"), ("p1_nofree", "p1_dense"),
                          ("p1_parent_again", "p1_parent"), ("p1_free_again", "p1_free"), ("p1_nofree_again", "p1_dense")):
            res[key] = child(a, role, lib=a.parent_lib if role == "p1_parent" else None)
            sys.stderr.write(f"{key}: {json.dumps(res[key])}\n")
            sys.stderr.flush()
        keys = ("vtb_us", "price_us", "update_us", "passes_per_s")
        base = res["p1_parent"]
        for key in ("p1_free", "p1_nofree", "p1_parent_again", "p1_free_again", "p1_nofree_again"):
            res[f"{key}_over_p1_parent"] = {k: round(res[key][k] / base[k], 4) for k in keys}
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    if a.phase1:
        res.update({"sparse_every": a.sparse_every, "sparse_chunk": a.sparse_chunk})
        for key, role in (("pbox", "pbox"), ("pbox_flag", "pbox_flag"), ("p1_dense", "p1_dense"),
                          ("p1_sparse", "p1_sparse"), ("p1_dense_again", "p1_dense"), ("pbox_again", "pbox"),
                          ("pbox_flag_again", "pbox_flag")):
            res[key] = child(a, role)
            sys.stderr.write(f"{key}: {json.dumps(res[key])}\n")
            sys.stderr.flush()
        d, q = res["p1_dense"], res["pbox"]
        res["p1_dense_over_pbox"] = {"pass_rate": round(d["passes_per_s"] / q["it_per_s"], 3),
                                     "vtb_over_update_bandwidth": round(d["vtb_TBps"] / d["update_TBps"], 3)}
        res["flag_over_plain_it_per_s"] = round(res["pbox_flag"]["it_per_s"] / q["it_per_s"], 4)
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    for key, role in (("primal", "primal"), ("dual", "dual"), ("pbox", "pbox"), ("pbox_again", "pbox"),
                      ("dual_again", "dual"), ("primal_again", "primal")):
        res[key] = child(a, role)
        sys.stderr.write(f"{key}: {json.dumps(res[key])}\n")
        sys.stderr.flush()
    pb = res["pbox"]
    for base in ("dual", "primal"):
        q = res[base]
        res[f"pbox_over_{base}"] = {k: round(pb[k] / q[k], 3) for k in ("price_us", "update_us", "rest_us", "it_per_s")}
    if a.solve and a.solve_shape:
        res["solve"] = child(a, "solve")
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
