"""Generate tests/golden/dual_long_optima.json: the golden values of the
bound-flipping (long-step) ratio test's tests (tests/test_dual_long_cpu.py,
tests/test_gpu_dual_long.py).

For every boxed covering LP of tests/golden/dual_box_optima.json (dual_ref.SHAPES
with the bounds of dual_box_ref.boxed(m, n, seed, flipc), flipc 0 and 1) under
Dantzig and steepest-edge leaving rows: the numpy reference's
(tests/dual_long_ref.py) pivot count, first 200 (p, q) pairs, final basis, final
at-upper set and the three flip counters under the long-step ratio test, with
its four gaps.  z is checked against the `highs_z` dual_box_optima.json already
holds for the same LP (scipy is not needed).  A case is refused when z differs
from HiGHS by more than Z_REL relative, or when the row-key gap, the walk-key gap
or the slope margin is below MIN_GAP: above it neither the pivot sequence nor
the flip sets depend on the fp64 summation order, which is what makes the
pivot-for-pivot comparison with the GPU legitimate.

    python tests/golden/make_golden_dual_long.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import dual_ref  # noqa: E402
import dual_long_ref as ref  # noqa: E402

TRACE = 200
MIN_GAP = 1e-6
Z_REL = 1e-9
RULES = (ref.DANTZIG, ref.STEEPEST)


def main():
    with open(os.path.join(HERE, "dual_box_optima.json")) as f:
        box = {(c["m"], c["n"], c["seed"], c["flipc"], c["rule"]): c for c in json.load(f)["cases"]}
    out = {"generator": "tests/dual_box_ref.py boxed(m, n, seed, flipc)",
           "reference": "tests/dual_long_ref.py dual_simplex_long, ratio=LONG_STEP (first index on ties)",
           "highs_z": "tests/golden/dual_box_optima.json, the same LP",
           "min_gap": MIN_GAP, "cases": []}
    for (m, n, seed) in dual_ref.SHAPES:
        for flipc in (0, 1):
            A, b, c, u = ref.boxed(m, n, seed, bool(flipc))
            for rule in RULES:
                g = box[(m, n, seed, flipc, rule)]
                hz = g["highs_z"]
                r = ref.dual_simplex_long(A, b, c, u, rule=rule, trace_cap=TRACE)
                assert r.status == dual_ref.OPTIMUM, (m, flipc, rule, r.status)
                rel = abs(r.z - hz) / abs(hz)
                print(f"m={m} n={n} seed={seed} flipc={flipc} {rule}: z={r.z:.13g} (HiGHS rel {rel:.1e}) pivots "
                      f"{g['ref_pivots']} -> {r.pivots} flips={r.counters} at_upper={int(r.at_upper.sum())} "
                      f"gap_row={r.gap_row:.2e} gap_walk={r.gap_walk:.2e} gap_slope={r.gap_slope:.2e}", flush=True)
                if rel > Z_REL:
                    raise SystemExit(f"m={m}: z differs from HiGHS by {rel:.1e} relative")
                gap = min(r.gap_row, r.gap_walk, r.gap_slope)
                if gap < MIN_GAP:
                    raise SystemExit(f"m={m} flipc={flipc} {rule}: a gap of {gap:.1e} is below {MIN_GAP:g}: the pivot "
                                     "and flip sequence of this case is not a legitimate golden value")
                out["cases"].append({"m": m, "n": n, "seed": seed, "flipc": flipc, "rule": rule, "highs_z": hz,
                                     "ref_z": r.z, "ref_pivots": r.pivots, "textbook_pivots": g["ref_pivots"],
                                     "to_upper": r.to_upper, "placed": r.placed,
                                     "flips": r.flips, "flip_passes": r.flip_passes, "max_flips": r.max_flips,
                                     "gap_row": r.gap_row, "gap_walk": r.gap_walk, "gap_slope": r.gap_slope,
                                     "ref_trace_p": [int(p) for p, _ in r.trace],
                                     "ref_trace_q": [int(q) for _, q in r.trace],
                                     "ref_b_ixs": [int(j) for j in r.b_ixs],
                                     "ref_at_upper": [int(j) for j in np.flatnonzero(r.at_upper)]})
    with open(os.path.join(HERE, "dual_long_optima.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
