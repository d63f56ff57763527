"""Generate tests/golden/dual_optima.json: the golden values of the dual
simplex tests (tests/test_dual_cpu.py, tests/test_gpu_dual.py).

For every covering LP of tests/dual_ref.py SHAPES: the optimum found by an
independent solver (scipy HiGHS dual simplex).  For the shapes with m <= 256
also the numpy reference's (tests/dual_ref.py) optimum, pivot count, first 200
(p, q) pairs and final basis.  The m = 1024 reference run takes minutes in
numpy, so that shape carries the HiGHS optimum only.  The tests read the JSON
and need no scipy.

    python tests/golden/make_golden_dual.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
from scipy.optimize import linprog

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import dual_ref  # noqa: E402

TRACE = 200


def highs_optimum(A, b, c):
    res = linprog(-c, A_eq=A, b_eq=b, bounds=(0, None), method="highs-ds",
                  options={"primal_feasibility_tolerance": 1e-10,
                           "dual_feasibility_tolerance": 1e-10})
    assert res.status == 0, res.message
    return float(-res.fun)


def main():
    out = {"generator": "tests/dual_ref.py covering(m, n, seed): numpy default_rng; G=U(0,1), "
                        "h=U(1,2)*ns/8, cost=U(1,2); A=[-G|I], b=-h, c=[-cost|0]",
           "solver": "scipy %s linprog(method='highs-ds')" % __import__("scipy").__version__,
           "cases": []}
    for (m, n, seed) in dual_ref.SHAPES:
        A, b, c = dual_ref.covering(m, n, seed)
        z = highs_optimum(A, b, c)
        case = {"m": m, "n": n, "seed": seed, "highs_z": z}
        if (m, n, seed) in dual_ref.TRACED:
            r = dual_ref.dual_simplex(A, b, c, trace_cap=TRACE)
            assert r.status == dual_ref.OPTIMUM
            rel = abs(r.z - z) / abs(z)
            print(f"m={m} n={n} seed={seed}: highs z={z:.13g} ref z={r.z:.13g} pivots={r.pivots} rel={rel:.1e}")
            case.update({"ref_z": r.z, "ref_pivots": r.pivots,
                         "ref_trace_p": [int(p) for p, _ in r.trace],
                         "ref_trace_q": [int(q) for _, q in r.trace],
                         "ref_b_ixs": [int(j) for j in r.b_ixs]})
        else:
            print(f"m={m} n={n} seed={seed}: highs z={z:.13g}")
        out["cases"].append(case)
    with open(os.path.join(HERE, "dual_optima.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
