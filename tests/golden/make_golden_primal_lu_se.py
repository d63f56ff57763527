"""Generate tests/golden/primal_lu_se_optima.json: the golden values of the tests
of steepest-edge pricing with free columns in the bounded primal loop
(tests/test_primal_lu_se_cpu.py, tests/test_gpu_primal_lu_se.py).

`general` (tests/primal_lu_ref.py general_lu: a slack basis infeasible on both
sides, so the solve goes through phase 1) and `feasible`
(tests/primal_lu_se_ref.py free_feasible: a feasible slack basis, phase 2 only),
each at SHAPES from the slack basis: the numpy restatement's
(tests/primal_lu_se_ref.py primal_simplex_lu_se) optimum, pivot count, first 200
(p, q) pairs, final basis and at-upper set, the flip and to-upper counts, the
phase-1 counters, the free columns that entered and that are basic at the end,
the recurrence's drift on the entering columns and at the end, the smallest
relative gaps of the two argmins (the pricing gap on the steepest-edge key) and
between u_p and t_q, the Dantzig pivot count of primal_lu_ref.primal_simplex_lu,
and scipy's HiGHS optimum with the bounds as they are.

A case is refused when its smallest gap is below MIN_GAP (above it the pass
sequence does not depend on the fp64 summation order, and every case is compared
pass for pass on the device: change the seed, never the bar), when z differs from
HiGHS by more than Z_REL relative, when no free column entered or none is basic
at the end, when steepest edge needs no fewer pivots than Dantzig, when the
Dantzig solve ends elsewhere, or (`general`) when it has no phase-1 pivot.

    python tests/golden/make_golden_primal_lu_se.py
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
import primal_lu_ref  # noqa: E402
import primal_lu_se_ref as ref  # noqa: E402

TRACE = 200
MIN_GAP = 1e-6
Z_REL = 1e-9
SHAPES = [(7, 20, 0), (65, 200, 1), (130, 390, 2), (256, 1024, 3)]


def highs(A, b, c, l, u):
    bounds = [(None if not np.isfinite(lo) else float(lo), None if not np.isfinite(hi) else float(hi))
              for lo, hi in zip(l, u)]
    r = linprog(-c, A_eq=A, b_eq=b, bounds=bounds, method="highs")
    return r.status, (-float(r.fun) if r.status == 0 else None)


def one(name, gen, m, n, seed, need_p1):
    A, b, c, l, u = gen(m, n, seed)
    st, hz = highs(A, b, c, l, u)
    assert st == 0, (name, m, st)
    r = ref.primal_simplex_lu_se(A, b, c, l, u, trace_cap=TRACE)
    dz = primal_lu_ref.primal_simplex_lu(A, b, c, l, u, trace_cap=0)
    gap = min(r.gap_price, r.gap_ratio, r.gap_flip)
    print(f"{name} m={m} n={n} seed={seed}: {r.status} z={r.z:.13g} (HiGHS {hz:.13g}, rel {abs(r.z - hz) / abs(hz):.1e}) "
          f"pivots={r.pivots} (Dantzig {dz.pivots}) flips={r.flips} to_upper={r.to_upper} p1 {r.p1_passes}/{r.p1_pivots} "
          f"ninf0={r.ninf0} free entered {r.free_entered} basic {r.free_basic} gaps {r.gap_price:.2e} {r.gap_ratio:.2e} "
          f"{r.gap_flip:.2e} drift {r.drift_enter:.1e} {r.drift_final:.1e}", flush=True)
    tag = f"{name} m={m}"
    if r.status != dual_ref.OPTIMUM or dz.status != dual_ref.OPTIMUM:
        raise SystemExit(f"{tag}: status {r.status}, Dantzig {dz.status}")
    if abs(r.z - hz) > Z_REL * abs(hz) or abs(dz.z - hz) > Z_REL * abs(hz):
        raise SystemExit(f"{tag}: z {r.z!r} / Dantzig {dz.z!r} differs from HiGHS {hz!r}")
    if gap < MIN_GAP:
        raise SystemExit(f"{tag}: smallest gap {gap:.2e} below {MIN_GAP:.0e}: change the seed")
    if r.free_entered <= 0 or r.free_basic <= 0:
        raise SystemExit(f"{tag}: free entered {r.free_entered}, basic {r.free_basic}")
    if not r.pivots < dz.pivots:
        raise SystemExit(f"{tag}: {r.pivots} pivots, Dantzig {dz.pivots}")
    if need_p1 and r.p1_pivots == 0:
        raise SystemExit(f"{tag}: no phase-1 pivot")
    if not need_p1 and (r.ninf0 != 0 or r.p1_passes != 0):
        raise SystemExit(f"{tag}: the slack basis is not feasible")
    return {"m": m, "n": n, "seed": seed, "highs_z": hz, "ref_z": r.z, "ref_pivots": r.pivots,
            "dantzig_pivots": dz.pivots,
            "ref_trace_p": [int(p) for p, _ in r.trace], "ref_trace_q": [int(q) for _, q in r.trace],
            "ref_b_ixs": [int(j) for j in r.b_ixs], "ref_at_upper": [int(j) for j in np.flatnonzero(r.at_upper)],
            "flips": r.flips, "to_upper": r.to_upper, "p1_passes": r.p1_passes, "p1_pivots": r.p1_pivots,
            "ninf0": r.ninf0, "free_entered": r.free_entered, "free_basic": r.free_basic,
            "fixed_flips": r.fixed_flips, "drift_enter": r.drift_enter, "drift_final": r.drift_final,
            "gap_price": r.gap_price, "gap_ratio": r.gap_ratio, "gap_flip": r.gap_flip,
            "ties": {k: int(v) for k, v in r.ties.items()}}


def main():
    out = {"generators": {"general": "tests/primal_lu_ref.py general_lu(m, n, seed)",
                          "feasible": "tests/primal_lu_se_ref.py free_feasible(m, n, seed)"},
           "reference": "tests/primal_lu_se_ref.py primal_simplex_lu_se (first index on ties)",
           "min_gap": MIN_GAP, "general": [], "feasible": []}
    for (m, n, seed) in SHAPES:
        out["general"].append(one("general", ref.general_lu, m, n, seed, True))
    for (m, n, seed) in SHAPES:
        out["feasible"].append(one("feasible", ref.free_feasible, m, n, seed, False))
    with open(os.path.join(HERE, "primal_lu_se_optima.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
