"""Generate tests/golden/dual_box_optima.json: the golden values of the boxed
dual simplex tests (tests/test_dual_box_cpu.py, tests/test_gpu_dual_box.py).

For every covering LP of tests/dual_ref.py SHAPES with the bounds of
tests/dual_box_ref.py boxed(m, n, seed, flipc), flipc False and True, under
Dantzig and steepest-edge leaving rows: the numpy reference's
(tests/dual_box_ref.py) optimum, pivot count, first 200 (p, q) pairs, final
basis and final at-upper set, the smallest relative gap between the best and
the second-best key of both argmins over the whole solve, and scipy's HiGHS
optimum of the bounded LP.  A case is refused when z differs from HiGHS by more
than Z_REL relative or a gap is below MIN_GAP (the thresholds of the other
generators here): above MIN_GAP the pivot sequence does not depend on the fp64
summation order, which is what makes the pivot-for-pivot comparison with the
GPU legitimate.

`resolve`: the bound re-solve case at RESOLVE_SHAPE.  From the boxed LP, u is
tightened (every 8th finite structural bound halved; the tightened LP must stay
feasible for HiGHS), then loosened (every 16th finite bound of the tightened u
set to +inf).  A column that sits non-basic at its upper bound at the tightened
optimum has e_j < -eps there, and without that bound no side on which it is
dual feasible: spx_set_bounds refuses that by name (SPX_ERR_STATE), as the
reference does (`loose_all_bad_column`: the column it names).  Every one of the
16 possible offsets of "every 16th" hits at least one such column here (7 with
offset 0), so the loosened LP that is re-solved (`loose`) keeps the bound of
those columns (`loose_kept`) and drops the others of the stride.  Stored:
HiGHS's optimum of both LPs and the reference's pivot counts of fresh solves of
both, per rule.

    python tests/golden/make_golden_dual_box.py [--resolve-only]
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
import dual_box_ref as ref  # noqa: E402

TRACE = 200
MIN_GAP = 1e-6
Z_REL = 1e-9
RESOLVE_SHAPE = (256, 1024, 3)
RULES = (ref.DANTZIG, ref.STEEPEST)


def highs(A, b, c, u):
    bounds = [(0.0, None if not np.isfinite(x) else float(x)) for x in u]
    r = linprog(-c, A_eq=A, b_eq=b, bounds=bounds, method="highs")
    return r.status, (-float(r.fun) if r.status == 0 else None)


def tighten(u, ns):
    u = u.copy()
    k = np.where(np.isfinite(u[:ns]))[0][::8]
    u[k] *= 0.5
    return u


def loosen(u):
    u = u.copy()
    k = np.where(np.isfinite(u))[0][::16]
    u[k] = np.inf
    return u


def resolve_case():
    m, n, seed = RESOLVE_SHAPE
    A, b, c, u = ref.boxed(m, n, seed, False)
    u1 = tighten(u, n - m)
    res = {"m": m, "n": n, "seed": seed, "flipc": 0}
    tight = {rule: ref.dual_simplex_box(A, b, c, u1, rule=rule, trace_cap=0) for rule in RULES}
    up = tight[ref.DANTZIG].at_upper
    assert (tight[ref.STEEPEST].at_upper == up).all()  # one optimal vertex
    u2_all = loosen(u1)
    bad = ref.dual_simplex_box(A, b, c, u2_all, basis=tight[ref.DANTZIG].b_ixs, at_upper=up & np.isfinite(u2_all))
    assert bad.status == ref.NOT_DUAL_FEASIBLE
    res["loose_all_bad_column"] = bad.bad_column
    kept = np.flatnonzero(up & ~np.isfinite(u2_all))
    u2 = u2_all.copy()
    u2[kept] = u1[kept]
    res["loose_kept"] = [int(j) for j in kept]
    for name, uu in (("tight", u1), ("loose", u2)):
        st, hz = highs(A, b, c, uu)
        if st != 0:
            raise SystemExit(f"re-solve: the {name} LP is not feasible for HiGHS (status {st}): change the stride")
        res[name + "_highs_z"] = hz
        for rule in RULES:
            r = tight[rule] if name == "tight" else ref.dual_simplex_box(A, b, c, uu, rule=rule, trace_cap=0)
            assert r.status == dual_ref.OPTIMUM
            assert abs(r.z - hz) <= Z_REL * abs(hz)
            res[f"{name}_fresh_pivots_{rule}"] = r.pivots
            print(f"re-solve {name} {rule}: z={hz:.13g} fresh pivots={r.pivots}", flush=True)
    return res


def main():
    path = os.path.join(HERE, "dual_box_optima.json")
    if "--resolve-only" in sys.argv[1:]:
        with open(path) as f:
            out = json.load(f)
        out["resolve"] = resolve_case()
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
        return
    out = {"generator": "tests/dual_box_ref.py boxed(m, n, seed, flipc)",
           "reference": "tests/dual_box_ref.py dual_simplex_box (first index on ties)",
           "min_gap": MIN_GAP, "cases": []}
    for (m, n, seed) in dual_ref.SHAPES:
        for flipc in (False, True):
            A, b, c, u = ref.boxed(m, n, seed, flipc)
            st, hz = highs(A, b, c, u)
            assert st == 0, (m, flipc, st)
            for rule in RULES:
                r = ref.dual_simplex_box(A, b, c, u, rule=rule, trace_cap=TRACE)
                assert r.status == dual_ref.OPTIMUM, (m, flipc, rule, r.status)
                rel = abs(r.z - hz) / abs(hz)
                gap = min(r.gap_row, r.gap_ratio)
                print(f"m={m} n={n} seed={seed} flipc={int(flipc)} {rule}: z={r.z:.13g} (HiGHS rel {rel:.1e}) "
                      f"pivots={r.pivots} to_upper={r.to_upper} at_upper={int(r.at_upper.sum())} placed={r.placed} "
                      f"gap_row={r.gap_row:.2e} gap_ratio={r.gap_ratio:.2e}", flush=True)
                if rel > Z_REL:
                    raise SystemExit(f"m={m}: z differs from HiGHS by {rel:.1e} relative")
                if gap < MIN_GAP:
                    raise SystemExit(f"m={m} flipc={flipc} {rule}: a key gap of {gap:.1e} is below {MIN_GAP:g}: the "
                                     "pivot sequence of this case is not a legitimate golden value")
                out["cases"].append({"m": m, "n": n, "seed": seed, "flipc": int(flipc), "rule": rule,
                                     "highs_z": hz, "ref_z": r.z, "ref_pivots": r.pivots, "to_upper": r.to_upper,
                                     "placed": r.placed, "gap_row": r.gap_row, "gap_ratio": r.gap_ratio,
                                     "ref_trace_p": [int(p) for p, _ in r.trace],
                                     "ref_trace_q": [int(q) for _, q in r.trace],
                                     "ref_b_ixs": [int(j) for j in r.b_ixs],
                                     "ref_at_upper": [int(j) for j in np.flatnonzero(r.at_upper)]})
    out["resolve"] = resolve_case()
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
