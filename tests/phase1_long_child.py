"""One run of a golden family (m, n, seed) under phase 1's long-step ratio test,
in a process of its own, for tests/test_gpu_primal_phase1_long.py (not a test
module): the parent sets SPX_PBOX_LONG_CAP, which the library reads once per
context, and this process stores what it reached.  K > 0 stops after K pivots.

usage: python phase1_long_child.py OUT.npz FAMILY PRICING M N SEED K
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import primal_phase1_long_ref as ref  # noqa: E402
import simplex_method_gpu_amd as spx  # noqa: E402


def context(family, pricing, lp, **kw):
    """boxed_general: upper bounds only (the kernels without free columns);
    general_lu: general bounds (the *_f kernels)."""
    A, b, c, l, u = lp
    rule = spx.PRIMAL_PRICING_STEEPEST if pricing == "steepest" else spx.PRIMAL_PRICING_DANTZIG
    kw.setdefault("trace", 200)
    if family == "general_lu":
        kw["lower"] = l
    ctx = spx.Context(np.ascontiguousarray(A.T), b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, primal_phase1=True,
                      primal_pricing=rule, primal_phase1_pricing=rule, primal_free_pricing=rule, **kw)
    return ctx


def main():
    out, family, pricing = sys.argv[1:4]
    m, n, seed, k = map(int, sys.argv[4:8])
    with context(family, pricing, ref.lp_of(family, m, n, seed)) as ctx:
        ctx.set_primal_phase1_ratio(spx.PRIMAL_RATIO_LONG_STEP)
        if k > 0:
            status, pivots = ctx.iterate(k)
            z = ctx.objective()
        else:
            r = ctx.solve()
            status, pivots, z = r.status, r.pivots, r.z
        tp, tq = ctx.trace()
        s = ctx.state(binv=True)
        x, up = ctx.primal()
        np.savez(out, status=int(status), pivots=pivots, z=z, tp=tp, tq=tq, b_ixs=s["b_ixs"], x_b=s["x_b"], y=s["y"],
                 binv=s["binv"], x=x, up=up, flips=np.array(ctx.primal_flips()), ph=np.array(ctx.primal_phase1()),
                 ls=np.array(ctx.primal_long_steps()))


if __name__ == "__main__":
    main()
