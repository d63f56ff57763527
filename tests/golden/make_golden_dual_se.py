"""Generate tests/golden/dual_se_optima.json: the golden values of the dual
steepest-edge tests (tests/test_dual_se_cpu.py, tests/test_gpu_dual_se.py).

For every covering LP of tests/dual_ref.py SHAPES: the numpy reference's
(tests/dual_se_ref.py) pivot count, first 200 (p, q) pairs, final basis and
optimum under dual steepest-edge pricing, the pivot count of the Dantzig
reference (tests/dual_ref.py) beside it, and the smallest relative gap between
the best and the second-best key over the whole solve for both argmins (the
leaving row and the ratio test).  A case whose gap is below MIN_GAP is refused:
above it, the pivot sequence does not depend on the fp64 summation order, which
is what makes the pivot-for-pivot comparison with the GPU legitimate.  z is
checked against tests/golden/dual_optima.json's HiGHS optimum (`highs_z`), which
the tests read from that file.  The m = 1024 Dantzig run takes about a minute.

    python tests/golden/make_golden_dual_se.py
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import dual_ref  # noqa: E402
import dual_se_ref  # noqa: E402

TRACE = 200
MIN_GAP = 1e-6
Z_REL = 1e-9


def main():
    with open(os.path.join(HERE, "dual_optima.json")) as f:
        highs = {(c["m"], c["n"], c["seed"]): c["highs_z"] for c in json.load(f)["cases"]}
    out = {"generator": "tests/dual_ref.py covering(m, n, seed)",
           "reference": "tests/dual_se_ref.py dual_simplex_se (exact row norms of B^-1, first index on ties)",
           "min_gap": MIN_GAP, "cases": []}
    for (m, n, seed) in dual_ref.SHAPES:
        A, b, c = dual_ref.covering(m, n, seed)
        r = dual_se_ref.dual_simplex_se(A, b, c, trace_cap=TRACE)
        assert r.status == dual_ref.OPTIMUM
        z = highs[(m, n, seed)]
        rel = abs(r.z - z) / abs(z)
        dz = dual_ref.dual_simplex(A, b, c, trace_cap=0)
        assert dz.status == dual_ref.OPTIMUM
        print(f"m={m} n={n} seed={seed}: z={r.z:.13g} (HiGHS rel {rel:.1e}) steepest pivots={r.pivots} "
              f"Dantzig pivots={dz.pivots} gap_row={r.gap_row:.2e} gap_ratio={r.gap_ratio:.2e}", flush=True)
        if rel > Z_REL:
            raise SystemExit(f"m={m}: z differs from HiGHS by {rel:.1e} relative")
        if min(r.gap_row, r.gap_ratio) < MIN_GAP:
            raise SystemExit(f"m={m}: a key gap of {min(r.gap_row, r.gap_ratio):.1e} is below {MIN_GAP:g}: the pivot "
                             "sequence of this case is not a legitimate golden value")
        out["cases"].append({"m": m, "n": n, "seed": seed, "ref_z": r.z, "ref_pivots": r.pivots,
                             "dantzig_pivots": dz.pivots, "gap_row": r.gap_row, "gap_ratio": r.gap_ratio,
                             "ref_trace_p": [int(p) for p, _ in r.trace],
                             "ref_trace_q": [int(q) for _, q in r.trace],
                             "ref_b_ixs": [int(j) for j in r.b_ixs]})
    with open(os.path.join(HERE, "dual_se_optima.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
