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

    python tools/dual_bench.py [--k 1000 --warm 200] [--dual-pricing steepest] [--solve]
                               [--parent-root DIR] [--out profiles/dual_c3.json]
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


def measure(make_ctx, k, warm):
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
    return {"pivots": p1 - p0, "status": int(st), "it_per_s": round((p1 - p0) / dt, 1),
            "price_us": round(price_us, 2), "update_us": round(update_us, 2),
            "timed_passes": kt["price_launches"],
            "bytes_price": bytes_price, "bytes_update": b1["bytes_update"],
            "price_TBps": round(bytes_price / (price_us * 1e-6) / 1e12, 3),
            "price_frac_of_8TBps": round(bytes_price / (price_us * 1e-6) / PEAK, 3),
            "update_TBps": round(b1["bytes_update"] / (update_us * 1e-6) / 1e12, 3)}


def run_primal(a):
    import simplex_method_gpu_amd as spx

    def make(timing):
        return spx.Context(m=a.m, n=a.n, seed=0, device=0, window=-1, timing=timing)

    return measure(make, a.k, a.warm)


def rule_kw(a, spx):
    """(the parent's Context has no dual_pricing: Dantzig passes nothing)"""
    return {"dual_pricing": spx.DUAL_PRICING_STEEPEST} if a.dual_pricing == "steepest" else {}


def run_dual(a):
    import numpy as np

    import dual_ref
    import simplex_method_gpu_amd as spx

    A, b, c = dual_ref.covering(a.m, a.n, a.seed)
    A_cols = np.ascontiguousarray(A.T)
    del A

    def make(timing):
        return spx.Context(A_cols, b, c, device=0, window=-1, algorithm=spx.ALGO_DUAL, timing=timing,
                           **rule_kw(a, spx))

    res = measure(make, a.k, a.warm)
    res["dual_pricing"] = a.dual_pricing
    return res


def run_solve(a):
    """Whole solves to the optimum: the first after a warm-up solve of the same context."""
    import numpy as np

    import dual_ref
    import simplex_method_gpu_amd as spx

    out = []
    for (m, n, seed) in [(a.m, a.n, a.seed)] + [tuple(s) for s in a.solve_shape]:
        A, b, c = dual_ref.covering(m, n, seed)
        A_cols = np.ascontiguousarray(A.T)
        del A
        with spx.Context(A_cols, b, c, device=0, window=-1, algorithm=spx.ALGO_DUAL,
                         refactor_every=a.refactor, **rule_kw(a, spx)) as ctx:
            ctx.iterate(20)  # (first-launch costs)
            ctx.reset()
            t0 = time.perf_counter()
            r = ctx.solve()
            dt = time.perf_counter() - t0
        out.append({"m": m, "n": n, "seed": seed, "dual_pricing": a.dual_pricing, "refactor_every": a.refactor,
                    "status": int(r.status), "pivots": r.pivots, "z": r.z, "seconds": round(dt, 4)})
    return out


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
    ap.add_argument("--role", default=None, choices=[None, "primal", "dual", "solve"])
    a = ap.parse_args()
    if a.role:  # a child: one side, one JSON line
        run = {"primal": run_primal, "dual": run_dual, "solve": run_solve}[a.role]
        print(json.dumps(run(a)), flush=True)
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
        env = dict(os.environ)
        if parent:
            env["SPX_BENCH_ROOT"] = os.path.abspath(a.parent_root)
        cmd = [sys.executable, os.path.abspath(__file__), "--role", role, "--m", str(a.m), "--n", str(a.n),
               "--seed", str(a.seed), "--k", str(a.k), "--warm", str(a.warm), "--dual-pricing", rule,
               "--refactor", str(a.refactor)]
        for shape in a.solve_shape:
            cmd += ["--solve-shape"] + [str(v) for v in shape]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"{key} run failed ({out.returncode})")
        res[key] = json.loads(out.stdout.strip().splitlines()[-1])
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
