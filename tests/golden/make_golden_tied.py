"""Generate tests/golden/tied_optima.json: the golden values of the exact-tie
tests (tests/test_tied_cpu.py, tests/test_gpu_tied.py).

One case per loop variant (tests/tied_lp.py VARIANTS: the dual loop under
Dantzig and steepest-edge rows, the boxed dual loop under both, the long-step
ratio test under both, the bounded primal loop, its phase 1 on a feasible and
on an infeasible LP, general bounds with free columns on a bounded and -- at
65 x 200 only -- on an unbounded LP) at each of tied_lp.shapes(variant), on the
integer interval-matrix LPs of tests/tied_lp.py.  Each case records scipy's
HiGHS status and optimum,
the numpy reference's status, pivot count, first 200 (p, q) pairs, final basis
and at-upper set, its flip / to-upper / phase-1 counters and its tie counters
(the passes in which a decision met an exact tie).

For every case the seed is the first of 0, 1, 2, ... at which all of these hold
(they are conditions, not measurements):
  - the reference ends (no cycling within MAX_PIVOTS) with HiGHS's status, and
    its z equals HiGHS's exactly;
  - x_b, y and B^-1 held integers only after every pass;
  - at 65 x 200 and larger, every tie counter that applies to the variant is >=
    1; a long-step case also has a walk over >= 3 consecutive equal keys.
  - a general-bounds case (tied_lp.LU_VARIANTS, the *_f kernels), at every
    shape: a free column enters and one is basic at the end, at least one
    pricing tie has a free column among the tied minima (`free_price`), at
    least one pass has a fixed column enter and flip at once; the unbounded
    case ends on a free entering column that no row blocks.  Their HiGHS values
    come from linprog(method="highs") with bounds=list(zip(l, u)).
Because every number is an exact integer the reference's pass sequence does not
depend on the order of any sum, which is what makes the pass-for-pass
comparison with the GPU legitimate in the presence of ties.

    python tests/golden/make_golden_tied.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
from scipy.optimize import linprog

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import tied_lp  # noqa: E402

TRACE = 200
MAX_PIVOTS = 5000
MAX_SEED = 400
MIXED_AT = (65, 256)   # boxed dual cases at these m use tied_covering's `mixed` costs
STATUS = {0: "optimum", 2: "infeasible", 3: "unbounded"}
WANT = {"phase1_infeasible": "infeasible", "free_unbounded": "unbounded"}


def highs(A, b, c, u):
    bounds = [(0.0, None if not np.isfinite(x) else float(x)) for x in u]
    r = linprog(-c, A_eq=A, b_eq=b, bounds=bounds, method="highs-ds")
    return STATUS.get(r.status, "status %d" % r.status), (-float(r.fun) if r.status == 0 else None)


def highs_lu(A, b, c, l, u):
    bounds = [(None if not np.isfinite(lo) else float(lo), None if not np.isfinite(hi) else float(hi))
              for lo, hi in zip(l, u)]
    r = linprog(-c, A_eq=A, b_eq=b, bounds=bounds, method="highs")
    return STATUS.get(r.status, "status %d" % r.status), (-float(r.fun) if r.status == 0 else None)


def record(variant, m, n, seed, mixed):
    """The case's golden record, or the reason it is refused."""
    lp = tied_lp.case_lp(variant, m, n, seed, mixed)
    r = tied_lp.case_ref(variant, lp, max_iter=MAX_PIVOTS, trace_cap=TRACE)
    want = WANT.get(variant, "optimum")
    lu = variant in tied_lp.LU_VARIANTS
    if r.status != want:
        return None, f"reference status {r.status}"
    if not r.integral:
        return None, "a non-integer value"
    applies = tied_lp.VARIANTS[variant]
    if m >= 65:
        missing = [k for k in applies if r.ties[k] < 1]
        if missing:
            return None, f"no tie of kind {missing}"
        if variant.startswith("long_") and r.walk_run < 3:
            return None, f"longest equal-key walk {r.walk_run}"
    if lu:
        if r.free_entered < 1 or r.free_basic < 1:
            return None, f"free columns entered {r.free_entered}, basic at the end {r.free_basic}"
        if r.ties["free_price"] < 1:
            return None, "no pricing tie with a free column among the minima"
        if r.fixed_flips < 1:
            return None, "no fixed column enters and flips"
        if want == "unbounded" and not np.isneginf(lp[3][r.ray_col]):
            return None, "unbounded through a column that is not free"
    hs, hz = highs_lu(*lp) if lu else highs(*lp)
    if hs != want:
        return None, f"HiGHS says {hs}"
    if hz is not None and r.z != hz:
        return None, f"z {r.z!r} != HiGHS {hz!r}"
    case = {"variant": variant, "m": m, "n": n, "seed": seed, "mixed": int(mixed), "highs_status": hs, "highs_z": hz,
            "ref_status": r.status, "ref_pivots": r.pivots,
            "ref_trace_p": [int(p) for p, _ in r.trace], "ref_trace_q": [int(q) for _, q in r.trace],
            "ref_b_ixs": [int(j) for j in r.b_ixs],
            "ref_at_upper": [int(j) for j in np.flatnonzero(getattr(r, "at_upper", []))],
            "ties": {k: int(r.ties[k]) for k in applies}}
    for k in ("to_upper", "placed", "flips", "flip_passes", "max_flips", "walk_run", "p1_passes", "p1_pivots", "ninf0",
              "ninf", "free_entered", "free_basic", "fixed_flips", "ray_col"):
        if hasattr(r, k):
            case[k] = int(getattr(r, k))
    return case, None


def main():
    out = {"generator": "tests/tied_lp.py case_lp(variant, m, n, seed, mixed)",
           "reference": "tests/tied_lp.py case_ref(variant, lp): the *_ref.py loop of the variant (first index on ties)",
           "solver": "scipy %s linprog(method='highs-ds')" % __import__("scipy").__version__,
           "cases": []}
    for variant in tied_lp.VARIANTS:
        for (m, n) in tied_lp.shapes(variant):
            mixed = variant.startswith(("box_", "long_")) and m in MIXED_AT
            for seed in range(MAX_SEED):
                case, why = record(variant, m, n, seed, mixed)
                if case is not None:
                    break
            else:
                raise SystemExit(f"{variant} {m}x{n}: no seed below {MAX_SEED} meets the conditions (last: {why})")
            print(f"{variant} {m}x{n} seed={seed}: {case['ref_status']} z={case['highs_z']} pivots={case['ref_pivots']} "
                  f"ties={case['ties']} " + " ".join(f"{k}={case[k]}" for k in ("flips", "max_flips", "walk_run",
                                                                                  "to_upper", "placed", "p1_passes",
                                                                                  "p1_pivots", "ninf0", "free_entered",
                                                                                  "free_basic", "fixed_flips",
                                                                                  "ray_col") if k in case),
                  flush=True)
            out["cases"].append(case)
    long_cases = [c for c in out["cases"] if c["variant"].startswith("long_")]
    assert any(c["ties"]["slope0"] >= 1 for c in long_cases) and any(c["walk_run"] >= 3 for c in long_cases)
    with open(os.path.join(HERE, "tied_optima.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
