"""Generate tests/golden/primal_box_optima.json: the golden values of the
bounded primal simplex tests (tests/test_primal_box_cpu.py,
tests/test_gpu_primal_box.py).

For every LP of tests/primal_box_ref.py boxed_primal(m, n, seed) at the shapes
of tests/dual_ref.py SHAPES, from the slack basis: the numpy reference's
(tests/primal_box_ref.py) optimum, pivot count, first 200 (p, q) pairs, final
basis and final at-upper set, the flip-pass and to-upper counts, the smallest
relative gaps of the two argmins and between u_p and t_q over the whole solve,
and scipy's HiGHS optimum of the bounded LP.  A case is refused when z differs
from HiGHS by more than Z_REL relative or one of the three gaps is below MIN_GAP
(the thresholds of the other generators here): above MIN_GAP the pass sequence
does not depend on the fp64 summation order, which is what makes the
pivot-for-pivot comparison with the GPU legitimate.  A traced case without a
flip pass or without a pivot to an upper bound is refused too: it would not
exercise what the loop adds.

`resolve`: the cost re-solve case at RESOLVE_SHAPE.  tests/dual_box_ref.py
boxed(m, n, seed, flipc) is solved by the boxed dual reference (steepest edge);
from that basis and those placements the objective becomes cost_variant(c) and
the bounded primal reference re-solves.  Stored per flipc: HiGHS's optimum of
the new LP and the reference's re-solve pivots, flip passes and to-upper pivots.
`dual_cost`: HiGHS's optima of that LP (flipc 0) with every bound finite
(all_bounded: with only the structural bounds finite, 10 slacks without a bound
have a negative reduced cost under the new objective at the old basis, which the
dual loop refuses by name) under c and under cost_variant(c), for spx_set_cost
under the dual loop.

    python tests/golden/make_golden_primal_box.py [--resolve-only]
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
import dual_box_ref  # noqa: E402
import primal_box_ref as ref  # noqa: E402

TRACE = 200
MIN_GAP = 1e-6
Z_REL = 1e-9
RESOLVE_SHAPE = (256, 1024, 3)


def highs(A, b, c, u):
    bounds = [(0.0, None if not np.isfinite(x) else float(x)) for x in u]
    r = linprog(-c, A_eq=A, b_eq=b, bounds=bounds, method="highs")
    return r.status, (-float(r.fun) if r.status == 0 else None)


def resolve_case():
    m, n, seed = RESOLVE_SHAPE
    res = {"m": m, "n": n, "seed": seed, "flipc": []}
    for flipc in (0, 1):
        A, b, c, u = dual_box_ref.boxed(m, n, seed, bool(flipc))
        first = dual_box_ref.dual_simplex_box(A, b, c, u, rule=dual_box_ref.STEEPEST, trace_cap=0)
        assert first.status == dual_ref.OPTIMUM
        c2 = ref.cost_variant(c, n - m, seed)
        st, hz = highs(A, b, c2, u)
        assert st == 0, st
        r = ref.primal_simplex_box(A, b, c2, u, basis=first.b_ixs, at_upper=first.at_upper, trace_cap=0)
        assert r.status == dual_ref.OPTIMUM, r.status
        rel = abs(r.z - hz) / abs(hz)
        print(f"re-solve flipc={flipc}: z={hz:.13g} (HiGHS rel {rel:.1e}) pivots={r.pivots} flips={r.flips} "
              f"to_upper={r.to_upper}", flush=True)
        if rel > Z_REL or r.pivots == 0:
            raise SystemExit(f"re-solve flipc={flipc}: z differs from HiGHS by {rel:.1e} relative, {r.pivots} pivots")
        res["flipc"].append({"flipc": flipc, "highs_z": hz, "dual_highs_z": highs(A, b, c, u)[1],
                             "ref_pivots": r.pivots, "flips": r.flips, "to_upper": r.to_upper})
    # set_cost under the dual loop: every bound finite, so every column has a dual feasible side
    A, b, c, u = dual_box_ref.boxed(m, n, seed, False)
    ub = ref.all_bounded(u, n - m)
    c3 = ref.cost_variant(c, n - m, seed)
    st0, hz0 = highs(A, b, c, ub)
    st3, hz3 = highs(A, b, c3, ub)
    assert st0 == 0 and st3 == 0, (st0, st3)
    print(f"dual set_cost: z={hz0:.13g} -> {hz3:.13g}", flush=True)
    res["dual_cost"] = {"first_highs_z": hz0, "highs_z": hz3}
    return res


def main():
    path = os.path.join(HERE, "primal_box_optima.json")
    if "--resolve-only" in sys.argv[1:]:
        with open(path) as f:
            out = json.load(f)
        out["resolve"] = resolve_case()
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
        return
    out = {"generator": "tests/primal_box_ref.py boxed_primal(m, n, seed)",
           "reference": "tests/primal_box_ref.py primal_simplex_box (first index on ties)",
           "min_gap": MIN_GAP, "cases": []}
    for (m, n, seed) in dual_ref.SHAPES:
        traced = (m, n, seed) in dual_ref.TRACED
        A, b, c, u = ref.boxed_primal(m, n, seed)
        st, hz = highs(A, b, c, u)
        assert st == 0, (m, st)
        r = ref.primal_simplex_box(A, b, c, u, trace_cap=TRACE)
        assert r.status == dual_ref.OPTIMUM, (m, r.status)
        rel = abs(r.z - hz) / abs(hz)
        gap = min(r.gap_price, r.gap_ratio, r.gap_flip)
        print(f"m={m} n={n} seed={seed}: z={r.z:.13g} (HiGHS rel {rel:.1e}) pivots={r.pivots} flips={r.flips} "
              f"to_upper={r.to_upper} at_upper={int(r.at_upper.sum())} gap_price={r.gap_price:.2e} "
              f"gap_ratio={r.gap_ratio:.2e} gap_flip={r.gap_flip:.2e}", flush=True)
        if rel > Z_REL:
            raise SystemExit(f"m={m}: z differs from HiGHS by {rel:.1e} relative")
        if gap < MIN_GAP:
            raise SystemExit(f"m={m}: a gap of {gap:.1e} is below {MIN_GAP:g}: the pass sequence of this case is "
                             "not a legitimate golden value")
        if traced and (r.flips == 0 or r.to_upper == 0):
            raise SystemExit(f"m={m}: {r.flips} flip passes, {r.to_upper} pivots to an upper bound: the case does "
                             "not exercise the bounded ratio test")
        out["cases"].append({"m": m, "n": n, "seed": seed, "traced": int(traced),
                             "highs_z": hz, "ref_z": r.z, "ref_pivots": r.pivots, "flips": r.flips,
                             "to_upper": r.to_upper, "gap_price": r.gap_price, "gap_ratio": r.gap_ratio,
                             "gap_flip": r.gap_flip,
                             "ref_trace_p": [int(p) for p, _ in r.trace],
                             "ref_trace_q": [int(q) for _, q in r.trace],
                             "ref_b_ixs": [int(j) for j in r.b_ixs],
                             "ref_at_upper": [int(j) for j in np.flatnonzero(r.at_upper)]})
    out["resolve"] = resolve_case()
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
