"""Dual simplex loop at C3's shape against the primal explicit pass.

Dual side: the covering LP of tests/dual_ref.py (m=4096, n=16384, window=-1,
SPX_ALGO_DUAL).  After a warm-up it times a block of dual pivots: it/s of an
untimed context, and from a timing context the mean k_dual_price and
k_dual_update times (the hipEvents the dispatch records) and k_dual_price's
algorithmic bandwidth, 8(m+1) x streamed non-basic columns / time.

Primal side, same process sequence on the same device: the headline LP (seeded
generator) at the same shape with window=-1, the explicit pass's it/s and its
mean k_price / k_update times.  --parent-root DIR measures that side with a
built checkout of the parent commit (its package and its libsimplex.so);
without it this build is used, whose primal kernels are the parent's, unchanged.

--dual-pricing {dantzig,steepest} is the dual side's leaving-row rule.  With
--parent-root the parent's dual loop (Dantzig: the only rule it has) is timed
in the same session too ("dual_parent"), which is what this build's kernels
are compared with.  --solve also times a whole solve of the covering LP to the
optimum under the rule (pivots and seconds, refactor_every = --refactor), and
--solve-shape M N SEED adds further shapes to that.

--boxed measures bounded variables (spx_set_bounds; tests/dual_box_ref.py
boxed(m, n, seed): the same covering LP with upper bounds): for both rules, at
the same timed-pivot protocol, this build's boxed kernels ("boxed_<rule>"), its
unbounded kernels on the plain covering LP ("plain_<rule>"), the boxed kernels
on that plain LP's pivots ("boxedk_<rule>": one finite bound that no x reaches,
so both walk the same pivots and the kernel times compare like for like), and with
--parent-root the parent's unbounded dual loop beside them ("parent_<rule>"),
all between two runs of the primal explicit pass.  rest_us is what a pass takes
beyond k_dual_price and k_dual_update (1e6 / it_per_s - price_us - update_us):
k_dual_step and the launch gaps.  --solve then times whole boxed solves under
both rules at the shape and at every --solve-shape, each checked by the CPU
certificate recomputed from the returned basis and placements
(tests/dual_box_ref.py certificate); --solve-max-iter caps a solve.

--long-step (with --boxed) adds the bound-flipping ratio test
(SPX_DUAL_RATIO_LONG_STEP) under both rules: this build's long-step pass on the
boxed LP ("long_<rule>"), on the plain LP's pivots with one bound no x reaches
("longk_<rule>": no pass flips, so its kernels compare like for like with
"boxedk_<rule>" and the update figure is the one without flips), and with
--parent-root the parent's textbook boxed pass on the boxed LP
("parentbox_<rule>").  A long-step record's kernel times come from
spx_pass_times: walk_us is the span from the end of k_dual_price to the end of
k_dual_flips (k_dual_long + k_dual_flips and their launch gaps); flips holds the
counters over the timed passes, and flip_hist the flips per pass of a separate
context stepped one pass at a time (index = flips, value = passes).
update_flip_us is derived: the update's mean on the boxed LP is flip_frac x
update_flip_us + (1 - flip_frac) x longk's update_us.  A run whose LP ends
before --k passes is marked "short" and averaged over the passes that pivoted.
--solve then also times whole long-step solves ("solve_long_<rule>") and, with
--parent-root, the parent's textbook ones ("solve_parent_<rule>").

    python tools/dual_bench.py [--k 1000 --warm 200] [--dual-pricing steepest] [--solve]
                               [--parent-root DIR] [--out profiles/dual_c3.json]
    python tools/dual_bench.py --boxed --parent-root DIR --solve --solve-shape 1024 4096 4
                               --out profiles/dual_box_c3.json
    python tools/dual_bench.py --boxed --long-step --parent-root DIR --solve --solve-shape 1024 4096 4
                               --out profiles/dual_long_c3.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.environ.get("SPX_BENCH_ROOT") or ROOT)  # (the primal child of --parent-root: that checkout)
sys.path.insert(1, os.path.join(ROOT, "tests"))

PEAK = 8.0e12  # MI355X HBM bytes/s the fractions are quoted against


def measure_long(make_ctx, k, warm):
    """The long-step pass: it/s from an untimed context, the three timed spans
    of spx_pass_times from a timing one, the flips per pass from a third."""
    with make_ctx(False) as ctx:
        ctx.iterate(warm)
        _, p0 = ctx.iterate(0)
        t0 = time.perf_counter()
        st, p1 = ctx.iterate(k)
        dt = time.perf_counter() - t0
    with make_ctx(True) as ctx:
        ctx.iterate(warm)
        ctx.pass_times()
        b0, f0 = ctx.info(), ctx.dual_flips()
        _, q0 = ctx.iterate(0)
        _, q1 = ctx.iterate(k)
        pt = ctx.pass_times()
        b1, f1 = ctx.info(), ctx.dual_flips()
    n = max(q1 - q0, 1)  # (passes that pivoted: all k unless the LP ended first)
    price_us, update_us = 1e3 * pt["price_ms"] / n, 1e3 * pt["update_ms"] / n
    walk_us = 1e3 * (pt["price_minloc_ms"] - pt["price_ms"]) / n
    hist = {}
    with make_ctx(False) as ctx:
        ctx.iterate(warm)
        last = ctx.dual_flips()[0]
        for _ in range(min(k, n)):
            ctx.iterate(1)
            cur = ctx.dual_flips()[0]
            hist[cur - last] = hist.get(cur - last, 0) + 1
            last = cur
    bytes_price = 0.5 * (b0["bytes_price"] + b1["bytes_price"])
    fp = f1[1] - f0[1]
    return {"pivots": p1 - p0, "status": int(st), "it_per_s": round((p1 - p0) / dt, 1), "short": bool(q1 - q0 < k),
            "price_us": round(price_us, 2), "update_us": round(update_us, 2), "walk_us": round(walk_us, 2),
            "rest_us": round(1e6 * dt / max(p1 - p0, 1) - price_us - update_us, 2),
            "timed_passes": int(n), "bytes_price": bytes_price, "bytes_update": b1["bytes_update"],
            "price_TBps": round(bytes_price / (price_us * 1e-6) / 1e12, 3),
            "price_frac_of_8TBps": round(bytes_price / (price_us * 1e-6) / PEAK, 3),
            "flips": {"columns": f1[0] - f0[0], "passes": fp, "max_since_create": f1[2]},
            "flip_frac": round(fp / n, 3), "flips_per_flipping_pass": round((f1[0] - f0[0]) / max(fp, 1), 2),
            "flip_hist": [hist.get(i, 0) for i in range(max(hist, default=0) + 1)]}


def measure(make_ctx, k, warm, rest=False):
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
        ctx.iterate(k)
        kt = ctx.kernel_times()
        b1 = ctx.info()
    nl = max(kt["price_launches"], 1)
    price_us = 1e3 * kt["price_ms"] / nl
    update_us = 1e3 * kt["update_ms"] / max(kt["update_launches"], 1)
    bytes_price = 0.5 * (b0["bytes_price"] + b1["bytes_price"])
    res = {"pivots": p1 - p0, "status": int(st), "it_per_s": round((p1 - p0) / dt, 1),
            "price_us": round(price_us, 2), "update_us": round(update_us, 2),
            "timed_passes": kt["price_launches"],
            "bytes_price": bytes_price, "bytes_update": b1["bytes_update"],
            "price_TBps": round(bytes_price / (price_us * 1e-6) / 1e12, 3),
            "price_frac_of_8TBps": round(bytes_price / (price_us * 1e-6) / PEAK, 3),
            "update_TBps": round(b1["bytes_update"] / (update_us * 1e-6) / 1e12, 3)}
    if rest:  # (--boxed) the pass outside its two big kernels
        res["rest_us"] = round(1e6 * dt / max(p1 - p0, 1) - price_us - update_us, 2)
    return res


def run_primal(a):
    import simplex_method_gpu_amd as spx

    def make(timing):
        return spx.Context(m=a.m, n=a.n, seed=0, device=0, window=-1, timing=timing)

    return measure(make, a.k, a.warm, a.rest)


def rule_kw(a, spx):
    """(the parent's Context has no dual_pricing / dual_ratio: the defaults pass nothing)"""
    kw = {"dual_pricing": spx.DUAL_PRICING_STEEPEST} if a.dual_pricing == "steepest" else {}
    if a.long_step and a.role:
        kw["dual_ratio"] = spx.DUAL_RATIO_LONG_STEP
    return kw


def run_dual(a):
    import numpy as np

    import dual_ref
    import simplex_method_gpu_amd as spx

    kw = rule_kw(a, spx)
    if a.boxed:
        import dual_box_ref

        A, b, c, u = dual_box_ref.boxed(a.m, a.n, a.seed)
        kw["upper"] = u
    else:
        A, b, c = dual_ref.covering(a.m, a.n, a.seed)
        if a.boxed_kernels:  # one finite bound no x reaches: the boxed kernels on the plain LP's pivots
            u = np.full(a.n, np.inf)
            u[0] = 1e30
            kw["upper"] = u
    A_cols = np.ascontiguousarray(A.T)
    del A

    def make(timing):
        return spx.Context(A_cols, b, c, device=0, window=-1, algorithm=spx.ALGO_DUAL, timing=timing, **kw)

    res = measure_long(make, a.k, a.warm) if a.long_step else measure(make, a.k, a.warm, a.rest)
    res["dual_pricing"] = a.dual_pricing
    res["dual_ratio"] = "long" if a.long_step else "textbook"
    if a.boxed or a.boxed_kernels:
        res["boxed"] = "lp" if a.boxed else "kernels"
    return res


def run_solve(a):
    """Whole solves to the optimum: the first after a warm-up solve of the same context."""
    import numpy as np

    import dual_ref
    import simplex_method_gpu_amd as spx

    out = []
    for (m, n, seed) in [(a.m, a.n, a.seed)] + [tuple(s) for s in a.solve_shape]:
        kw = rule_kw(a, spx)
        if a.boxed:
            import dual_box_ref

            A, b, c, u = dual_box_ref.boxed(m, n, seed)
            kw["upper"] = u
        else:
            A, b, c = dual_ref.covering(m, n, seed)
        A_cols = np.ascontiguousarray(A.T)
        if not a.boxed:
            del A
        with spx.Context(A_cols, b, c, device=0, window=-1, algorithm=spx.ALGO_DUAL,
                         refactor_every=a.refactor, **kw) as ctx:
            ctx.iterate(20)  # (first-launch costs)
            ctx.reset()
            t0 = time.perf_counter()
            r = ctx.solve(a.solve_max_iter) if a.solve_max_iter > 0 else ctx.solve()
            dt = time.perf_counter() - t0
            xu = ctx.primal() if a.boxed else None
            fl = ctx.dual_flips() if a.long_step else None
        rec = {"m": m, "n": n, "seed": seed, "dual_pricing": a.dual_pricing, "refactor_every": a.refactor,
               "status": int(r.status), "pivots": r.pivots, "z": r.z, "seconds": round(dt, 4),
               "it_per_s": round(r.pivots / dt, 1), "dual_ratio": "long" if a.long_step else "textbook"}
        if fl is not None:
            rec["flips"] = list(fl)
        if a.boxed and int(r.status) == 1:  # the CPU certificate, from the basis and the placements alone
            viol, dviol, zc = dual_box_ref.certificate(A, b, c, u, r.b_ixs, xu[1])
            rec.update({"at_upper": int(xu[1].sum()), "cert_bound_violation": viol, "cert_dual_violation": dviol,
                        "cert_z_rel": abs(zc - r.z) / abs(zc), "cert_ok": bool(viol <= 1e-9 and dviol <= 1e-7)})
        if a.boxed and int(r.status) == 4:  # infeasible: a row whose range over the box misses its bounds
            row, margin = dual_box_ref.farkas(A, b, u, r.b_ixs, xu[1])
            rec.update({"farkas_row": row, "farkas_margin": margin, "cert_ok": bool(row >= 0 and margin > 1e-7)})
        out.append(rec)
    return out


def main_boxed(a):
    """--boxed: parent / plain / boxed for both rules, then the solves."""
    res = {"m": a.m, "n": a.n, "k": a.k, "warm": a.warm, "covering_seed": a.seed,
           "parent": "parent commit" if a.parent_root else None}
    plan = [("primal", "primal", bool(a.parent_root), "dantzig", False)]
    for rule in ("dantzig", "steepest"):
        if a.parent_root:
            plan.append((f"parent_{rule}", "dual", True, rule, False))
        plan.append((f"plain_{rule}", "dual", False, rule, False))
        plan.append((f"boxedk_{rule}", "dual", False, rule, "kernels"))
        plan.append((f"boxed_{rule}", "dual", False, rule, True))
        if a.long_step:
            if a.parent_root:
                plan.append((f"parentbox_{rule}", "dual", True, rule, True))
            plan.append((f"longk_{rule}", "dual", False, rule, "kernels", True))
            plan.append((f"long_{rule}", "dual", False, rule, True, True))
    if a.solve:
        plan += [("solve_steepest", "solve", False, "steepest", True), ("solve_dantzig", "solve", False, "dantzig", True)]
        if a.long_step:
            plan += [("solve_long_steepest", "solve", False, "steepest", True, True),
                     ("solve_long_dantzig", "solve", False, "dantzig", True, True)]
            if a.parent_root:
                plan += [("solve_parent_steepest", "solve", True, "steepest", True),
                         ("solve_parent_dantzig", "solve", True, "dantzig", True)]
    plan.append(("primal_again", "primal", bool(a.parent_root), "dantzig", False))
    for key, role, parent, rule, boxed, *lng in plan:
        res[key] = child(a, role, parent, rule, boxed, key, bool(lng))
        sys.stderr.write(f"{key}: {json.dumps(res[key])}\n")
        sys.stderr.flush()
    for rule in ("dantzig", "steepest"):
        for top in ("boxed", "boxedk"):
            bx = res[f"{top}_{rule}"]
            for base in ("parent", "plain"):
                if f"{base}_{rule}" in res:
                    q = res[f"{base}_{rule}"]
                    res[f"{rule}_{top}_over_{base}"] = {k: round(bx[k] / q[k], 3)
                                                        for k in ("price_us", "update_us", "rest_us", "it_per_s")}
        if a.long_step:
            lk, lg = res[f"longk_{rule}"], res[f"long_{rule}"]
            for top, bases in (("longk", ("boxedk", "parent")), ("long", ("boxed", "parentbox"))):
                for base in bases:
                    if f"{base}_{rule}" in res:
                        q = res[f"{base}_{rule}"]
                        res[f"{rule}_{top}_over_{base}"] = {k: round(res[f"{top}_{rule}"][k] / q[k], 3)
                                                            for k in ("price_us", "update_us", "rest_us", "it_per_s")}
            if lg["flip_frac"] > 0:  # the mixture's other component: passes with flips
                lg["update_flip_us"] = round((lg["update_us"] - (1 - lg["flip_frac"]) * lk["update_us"])
                                             / lg["flip_frac"], 2)
    return res


def child(a, role, parent, rule, boxed, key, long_step=False):
    env = dict(os.environ)
    if parent:
        env["SPX_BENCH_ROOT"] = os.path.abspath(a.parent_root)
    cmd = [sys.executable, os.path.abspath(__file__), "--role", role, "--m", str(a.m), "--n", str(a.n),
           "--seed", str(a.seed), "--k", str(a.k), "--warm", str(a.warm), "--dual-pricing", rule,
           "--refactor", str(a.refactor), "--solve-max-iter", str(a.solve_max_iter), "--rest"]
    if boxed:
        cmd.append("--boxed-kernels" if boxed == "kernels" else "--boxed")
    if long_step:
        cmd.append("--long-step")
    for shape in a.solve_shape:
        cmd += ["--solve-shape"] + [str(v) for v in shape]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        sys.stderr.write(out.stdout + out.stderr)
        raise SystemExit(f"{key} run failed ({out.returncode})")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dual-pricing", default="dantzig", choices=["dantzig", "steepest"])
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--solve-shape", type=int, nargs=3, action="append", default=[], metavar=("M", "N", "SEED"))
    ap.add_argument("--refactor", type=int, default=500)
    ap.add_argument("--boxed", action="store_true")
    ap.add_argument("--long-step", action="store_true", help="with --boxed: the bound-flipping ratio test too")
    ap.add_argument("--boxed-kernels", action="store_true", help=argparse.SUPPRESS)  # (children of --boxed)
    ap.add_argument("--rest", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--solve-max-iter", type=int, default=0)
    ap.add_argument("--role", default=None, choices=[None, "primal", "dual", "solve"])
    a = ap.parse_args()
    if a.role:  # a child: one side, one JSON line
        run = {"primal": run_primal, "dual": run_dual, "solve": run_solve}[a.role]
        print(json.dumps(run(a)), flush=True)
        return
    if a.long_step and not a.boxed:
        ap.error("--long-step measures the boxed passes: give --boxed")
    if a.boxed:
        res = main_boxed(a)
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    res = {"m": a.m, "n": a.n, "k": a.k, "warm": a.warm, "covering_seed": a.seed,
           "primal_build": "parent commit" if a.parent_root else "this build"}
    # the primal side before and after: drift of the box
    plan = [("primal", "primal", bool(a.parent_root), "dantzig")]
    if a.parent_root:
        plan.append(("dual_parent", "dual", True, "dantzig"))
    plan.append(("dual", "dual", False, a.dual_pricing))
    if a.solve:
        plan.append(("solve", "solve", False, a.dual_pricing))
    plan.append(("primal_again", "primal", bool(a.parent_root), "dantzig"))
    for key, role, parent, rule in plan:
        res[key] = child(a, role, parent, rule, False, key)
    d, p = res["dual"], res["primal"]
    res["price_ratio_dual_over_primal"] = round(d["price_us"] / p["price_us"], 3)
    res["update_ratio_dual_over_primal"] = round(d["update_us"] / p["update_us"], 3)
    if a.parent_root:
        dp = res["dual_parent"]
        res["price_ratio_over_parent_dual"] = round(d["price_us"] / dp["price_us"], 3)
        res["update_ratio_over_parent_dual"] = round(d["update_us"] / dp["update_us"], 3)
        res["it_per_s_ratio_over_parent_dual"] = round(d["it_per_s"] / dp["it_per_s"], 3)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
