"""Generate tests/golden/primal_phase1_optima.json: the golden values of the
primal phase-1 tests (tests/test_primal_phase1_cpu.py,
tests/test_gpu_primal_phase1.py).

`cases`: for every LP of tests/primal_phase1_ref.py boxed_general(m, n, seed) at
SHAPES, from the slack basis (neither primal nor dual feasible): the numpy
reference's (tests/primal_phase1_ref.py) optimum, pivot count, first 200 (p, q)
pairs, final basis and at-upper set, the flip and to-upper counts, the phase-1
pass and pivot counts, the infeasible rows at entry, the smallest relative gaps
of the two argmins and between u_p and t_q over the whole solve, and scipy's
HiGHS optimum.  A case is refused when z differs from HiGHS by more than Z_REL
relative, when a gap is below MIN_GAP (the thresholds of
make_golden_primal_box.py: above MIN_GAP the pass sequence does not depend on
the fp64 summation order) or when it has no phase-1 pivot: pick another seed.

`infeasible`: boxed_general at INFEASIBLE_SHAPE made contradictory
(primal_phase1_ref.contradict); HiGHS must call it infeasible (status 2); the
reference's pivot count up to INFEASIBLE, and HiGHS's optimum after rows 0 and
1 get the right-hand side FEASIBLE_B01.

`stuck`: primal_box_ref.boxed_primal at STUCK_SHAPE solved to the optimum, then
cost_variant(c) and primal_phase1_ref.rhs_variant(b): the old basis must be out
of its bounds in some row and have a non-basic column without an upper bound
whose reduced cost is below -STUCK_D (so neither bounded loop takes it without
phase 1); HiGHS's optimum of the new LP and the reference's counts from that
basis.

    python tests/golden/make_golden_primal_phase1.py
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
import primal_box_ref  # noqa: E402
import primal_phase1_ref as ref  # noqa: E402

TRACE = 200
MIN_GAP = 1e-6
Z_REL = 1e-9
SHAPES = [(7, 20, 0), (65, 200, 1), (130, 390, 2), (256, 1024, 3)]
INFEASIBLE_SHAPE = (65, 200, 1)
FEASIBLE_B01 = (1000.0, 1000.0)
STUCK_SHAPE = (130, 390, 2)
STUCK_D = 1e-3


def highs(A, b, c, u):
    bounds = [(0.0, None if not np.isfinite(x) else float(x)) for x in u]
    r = linprog(-c, A_eq=A, b_eq=b, bounds=bounds, method="highs")
    return r.status, (-float(r.fun) if r.status == 0 else None)


def counts(r):
    return {"ref_pivots": r.pivots, "flips": r.flips, "to_upper": r.to_upper, "p1_passes": r.p1_passes,
            "p1_pivots": r.p1_pivots, "ninf0": r.ninf0, "gap_price": r.gap_price, "gap_ratio": r.gap_ratio,
            "gap_flip": r.gap_flip}


def check(name, r, hz, want=dual_ref.OPTIMUM):
    if r.status != want:
        raise SystemExit(f"{name}: status {r.status}")
    gap = min(r.gap_price, r.gap_ratio, r.gap_flip)
    if gap < MIN_GAP:
        raise SystemExit(f"{name}: a gap of {gap:.1e} is below {MIN_GAP:g}: pick another seed")
    if hz is not None:
        rel = abs(r.z - hz) / abs(hz)
        if rel > Z_REL:
            raise SystemExit(f"{name}: z differs from HiGHS by {rel:.1e} relative")
    if r.p1_pivots == 0:
        raise SystemExit(f"{name}: no phase-1 pivot")


def main():
    out = {"generator": "tests/primal_phase1_ref.py boxed_general(m, n, seed)",
           "reference": "tests/primal_phase1_ref.py primal_simplex_phase1 (first index on ties)",
           "min_gap": MIN_GAP, "cases": []}
    for (m, n, seed) in SHAPES:
        A, b, c, u = ref.boxed_general(m, n, seed)
        st, hz = highs(A, b, c, u)
        assert st == 0, (m, st)
        r = ref.primal_simplex_phase1(A, b, c, u, trace_cap=TRACE)
        print(f"m={m} n={n} seed={seed}: {r.status} z={r.z:.13g} (HiGHS {hz:.13g}) pivots={r.pivots} flips={r.flips} "
              f"to_upper={r.to_upper} p1 passes={r.p1_passes} pivots={r.p1_pivots} ninf0={r.ninf0} "
              f"gaps {r.gap_price:.2e} {r.gap_ratio:.2e} {r.gap_flip:.2e}", flush=True)
        check(f"m={m}", r, hz)
        case = {"m": m, "n": n, "seed": seed, "highs_z": hz, "ref_z": r.z,
                "ref_trace_p": [int(p) for p, _ in r.trace], "ref_trace_q": [int(q) for _, q in r.trace],
                "ref_b_ixs": [int(j) for j in r.b_ixs], "ref_at_upper": [int(j) for j in np.flatnonzero(r.at_upper)]}
        case.update(counts(r))
        out["cases"].append(case)

    m, n, seed = INFEASIBLE_SHAPE
    A, b, c, u = ref.boxed_general(m, n, seed)
    A2, b2, u2 = ref.contradict(A, b, u)
    st, _ = highs(A2, b2, c, u2)
    assert st == 2, st
    r = ref.primal_simplex_phase1(A2, b2, c, u2, trace_cap=0)
    print(f"infeasible: {r.status} after {r.pivots} pivots, ninf {r.ninf0} -> {r.ninf}", flush=True)
    check("infeasible", r, None, ref.INFEASIBLE)
    b3 = b2.copy()
    b3[0], b3[1] = FEASIBLE_B01
    st, hz = highs(A2, b3, c, u2)
    assert st == 0, st
    inf = {"m": m, "n": n, "seed": seed, "ninf_end": r.ninf, "feasible_b01": list(FEASIBLE_B01), "feasible_highs_z": hz}
    inf.update(counts(r))
    out["infeasible"] = inf

    m, n, seed = STUCK_SHAPE
    ns = n - m
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    first = primal_box_ref.primal_simplex_box(A, b, c, u, trace_cap=0)
    assert first.status == dual_ref.OPTIMUM
    c2 = primal_box_ref.cost_variant(c, ns, seed)
    b2 = ref.rhs_variant(b, seed)
    Binv = np.linalg.inv(A[:, first.b_ixs])
    beff = b2 - A[:, first.at_upper] @ u[first.at_upper]
    xb = Binv @ beff
    d = (c2[first.b_ixs] @ Binv) @ A - c2
    nonbasic = np.ones(n, dtype=bool)
    nonbasic[first.b_ixs] = False
    out_rows = int(np.count_nonzero((xb < -1e-6) | (xb > u[first.b_ixs] + 1e-6)))
    free_bad = int(np.count_nonzero(nonbasic & ~np.isfinite(u) & (d < -STUCK_D)))
    if out_rows == 0 or free_bad == 0:
        raise SystemExit(f"stuck: {out_rows} rows out of bounds, {free_bad} unbounded columns with d < -{STUCK_D}: "
                         "the old basis is feasible on one side; pick another seed")
    st, hz = highs(A, b2, c2, u)
    assert st == 0, st
    r = ref.primal_simplex_phase1(A, b2, c2, u, basis=first.b_ixs, at_upper=first.at_upper, trace_cap=0)
    print(f"stuck: {out_rows} rows out, {free_bad} unbounded columns priced out; {r.status} z={r.z:.13g} "
          f"(HiGHS {hz:.13g}) pivots={r.pivots} p1 {r.p1_passes}/{r.p1_pivots}", flush=True)
    check("stuck", r, hz)
    stuck = {"m": m, "n": n, "seed": seed, "first_pivots": first.pivots, "highs_z": hz, "rows_out": out_rows,
             "free_bad": free_bad}
    stuck.update(counts(r))
    out["stuck"] = stuck

    A, b, c, u = primal_box_ref.tiny_not_feasible()
    st, hz = highs(A, b, c, u)
    r = ref.primal_simplex_phase1(A, b, c, u)
    assert st == 0 and r.status == dual_ref.OPTIMUM and r.p1_pivots == 1, (st, r.status, r.p1_pivots)
    tiny = {"highs_z": hz, "x": [float(v) for v in r.primal(u)]}
    tiny.update(counts(r))
    out["tiny_not_feasible"] = tiny

    with open(os.path.join(HERE, "primal_phase1_optima.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
