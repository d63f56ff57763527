"""Generate tests/golden/primal_box_se_optima.json: the golden values of the
steepest-edge tests of the bounded primal loop (tests/test_primal_box_se_cpu.py,
tests/test_gpu_primal_box_se.py).

For every LP of tests/primal_box_ref.py boxed_primal(m, n, seed) at the shapes
of tests/dual_ref.py SHAPES, from the slack basis: the numpy restatement's
(tests/primal_box_se_ref.py) optimum, pivot count, first 200 (p, q) pairs, final
basis and at-upper set, flip-pass and to-upper counts, the three gaps (the
pricing gap on the steepest-edge key), the weight drift (recurrence against the
recomputed 1 + ||B^-1 A_j||^2: entering columns during the solve, all non-basic
columns at the end) and scipy's HiGHS optimum.  A case is refused when z is off
HiGHS by more than Z_REL relative, when a gap is below MIN_GAP, or when a traced
case has no flip pass or no to-upper pivot.  Every shape passes with the seeds
of dual_ref.SHAPES: no seed had to be replaced.

`resolve`: the cost re-solve of make_golden_primal_box.py under steepest edge.
From the boxed dual reference's optimal basis and placements the objective
becomes cost_variant(c) and the restatement re-solves with the weights
restarted at 1 + ||A_j||^2 (what the library does after spx_set_algorithm);
stored per flipc: its pivots, flip passes and to-upper pivots.

    python tests/golden/make_golden_primal_box_se.py
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
import primal_box_ref  # noqa: E402
import primal_box_se_ref as ref  # noqa: E402

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
        c2 = primal_box_ref.cost_variant(c, n - m, seed)
        st, hz = highs(A, b, c2, u)
        assert st == 0, st
        r = ref.primal_simplex_box_se(A, b, c2, u, basis=first.b_ixs, at_upper=first.at_upper, trace_cap=0)
        assert r.status == dual_ref.OPTIMUM, r.status
        rel = abs(r.z - hz) / abs(hz)
        gap = min(r.gap_price, r.gap_ratio, r.gap_flip)
        print(f"re-solve flipc={flipc}: z={hz:.13g} (HiGHS rel {rel:.1e}) pivots={r.pivots} flips={r.flips} "
              f"to_upper={r.to_upper} gap={gap:.2e}", flush=True)
        if rel > Z_REL or r.pivots == 0:
            raise SystemExit(f"re-solve flipc={flipc}: z differs from HiGHS by {rel:.1e} relative, {r.pivots} pivots")
        if gap < MIN_GAP:
            raise SystemExit(f"re-solve flipc={flipc}: a gap of {gap:.1e} is below {MIN_GAP:g}")
        res["flipc"].append({"flipc": flipc, "highs_z": hz, "ref_pivots": r.pivots, "flips": r.flips,
                             "to_upper": r.to_upper, "gap_price": r.gap_price, "gap_ratio": r.gap_ratio,
                             "gap_flip": r.gap_flip})
    return res


def main():
    path = os.path.join(HERE, "primal_box_se_optima.json")
    out = {"generator": "tests/primal_box_ref.py boxed_primal(m, n, seed)",
           "reference": "tests/primal_box_se_ref.py primal_simplex_box_se (first index on ties)",
           "min_gap": MIN_GAP, "cases": []}
    for (m, n, seed) in dual_ref.SHAPES:
        traced = (m, n, seed) in dual_ref.TRACED
        A, b, c, u = ref.boxed_primal(m, n, seed)
        st, hz = highs(A, b, c, u)
        assert st == 0, (m, st)
        r = ref.primal_simplex_box_se(A, b, c, u, trace_cap=TRACE)
        assert r.status == dual_ref.OPTIMUM, (m, r.status)
        rel = abs(r.z - hz) / abs(hz)
        gap = min(r.gap_price, r.gap_ratio, r.gap_flip)
        print(f"m={m} n={n} seed={seed}: z={r.z:.13g} (HiGHS rel {rel:.1e}) pivots={r.pivots} flips={r.flips} "
              f"to_upper={r.to_upper} at_upper={int(r.at_upper.sum())} gap_price={r.gap_price:.2e} "
              f"gap_ratio={r.gap_ratio:.2e} gap_flip={r.gap_flip:.2e} drift={r.drift_enter:.2e} / "
              f"{r.drift_final:.2e}", flush=True)
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
                             "gap_flip": r.gap_flip, "drift": r.drift, "drift_enter": r.drift_enter,
                             "drift_final": r.drift_final,
                             "ref_trace_p": [int(p) for p, _ in r.trace],
                             "ref_trace_q": [int(q) for _, q in r.trace],
                             "ref_b_ixs": [int(j) for j in r.b_ixs],
                             "ref_at_upper": [int(j) for j in np.flatnonzero(r.at_upper)]})
    out["resolve"] = resolve_case()
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
