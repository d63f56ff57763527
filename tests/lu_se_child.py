"""One run of general_lu / free_feasible (m, n, seed) under steepest edge with free
columns, in a process of its own, for tests/test_gpu_primal_lu_se.py (not a test
module): the parent sets SPX_PBOX_SE_LDS, which the library reads once per
context, and this process stores what it reached.  K > 0 stops after K pivots.

usage: python lu_se_child.py OUT.npz KIND M N SEED K [global_y | price_grid=G | refactor_every=R]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import primal_lu_se_ref  # noqa: E402
import simplex_method_gpu_amd as spx  # noqa: E402


def main():
    out, kind = sys.argv[1], sys.argv[2]
    m, n, seed, k = map(int, sys.argv[3:7])
    kw = {}
    for a in sys.argv[7:]:
        if a == "global_y":
            kw["global_y"] = True
        else:
            name, v = a.split("=")
            assert name in ("price_grid", "refactor_every"), a
            kw[name] = int(v)
    gen = primal_lu_se_ref.general_lu if kind == "general" else primal_lu_se_ref.free_feasible
    A, b, c, l, u = gen(m, n, seed)
    S = spx.PRIMAL_PRICING_STEEPEST
    with spx.Context(np.ascontiguousarray(A.T), b, c, algorithm=spx.ALGO_PRIMAL_BOX, lower=l, upper=u, trace=200,
                     primal_phase1=kind == "general", primal_pricing=S, primal_phase1_pricing=S, primal_free_pricing=S,
                     **kw) as ctx:
        if k > 0:
            status, pivots = ctx.iterate(k)
            z = ctx.objective()
        else:
            r = ctx.solve()
            status, pivots, z = r.status, r.pivots, r.z
        tp, tq = ctx.trace()
        w = ctx.primal_weights()
        s = ctx.state(binv=True)
        x, up = ctx.primal()
        np.savez(out, status=int(status), pivots=pivots, z=z, tp=tp, tq=tq, w=w, b_ixs=s["b_ixs"], x_b=s["x_b"],
                 y=s["y"], binv=s["binv"], x=x, up=up, flips=np.array(ctx.primal_flips()),
                 ph=np.array(ctx.primal_phase1()), lds_vecs=ctx.loop_layout()["pbox_se_lds_vecs"],
                 price_grid=ctx.config()["price_grid"])


if __name__ == "__main__":
    main()
