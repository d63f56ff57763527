"""One solve of boxed_general(m, n, seed) with steepest edge through phase 1, in a
process of its own, for tests/test_gpu_primal_phase1_se.py (not a test module):
the parent sets SPX_PBOX_SE_LDS, which the library reads once per context, and
this process stores what it reached.

usage: python phase1_se_child.py OUT.npz M N SEED
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import primal_phase1_ref  # noqa: E402
import simplex_method_gpu_amd as spx  # noqa: E402


def main():
    out = sys.argv[1]
    m, n, seed = map(int, sys.argv[2:5])
    A, b, c, u = primal_phase1_ref.boxed_general(m, n, seed)
    with spx.Context(np.ascontiguousarray(A.T), b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, trace=200,
                     primal_phase1=True, primal_pricing=spx.PRIMAL_PRICING_STEEPEST,
                     primal_phase1_pricing=spx.PRIMAL_PRICING_STEEPEST) as ctx:
        r = ctx.solve()
        tp, tq = ctx.trace()
        w = ctx.primal_weights()
        s = ctx.state(binv=True)
        x, up = ctx.primal()
        np.savez(out, status=int(r.status), pivots=r.pivots, z=r.z, tp=tp, tq=tq, w=w, b_ixs=s["b_ixs"], x_b=s["x_b"],
                 y=s["y"], binv=s["binv"], up=up, flips=np.array(ctx.primal_flips()), ph=np.array(ctx.primal_phase1()),
                 lds_vecs=ctx.loop_layout()["pbox_se_lds_vecs"])


if __name__ == "__main__":
    main()
