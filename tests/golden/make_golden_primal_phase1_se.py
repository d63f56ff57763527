"""Generate tests/golden/primal_phase1_se_optima.json: the golden values of the
tests of steepest-edge pricing through phase 1 of the bounded primal loop
(tests/test_primal_phase1_se_cpu.py, tests/test_gpu_primal_phase1_se.py;
DESIGN.md §7l).

`cases`: for every LP of tests/primal_phase1_ref.py boxed_general(m, n, seed) at
SHAPES, from the slack basis: the numpy restatement's
(tests/primal_phase1_se_ref.py) optimum, pivot count, first 200 (p, q) pairs,
final basis and at-upper set, the flip and to-upper counts, the phase-1 pass and
pivot counts, the infeasible rows at entry, the smallest relative gaps of the
two argmins (the pricing gap on the steepest-edge key) and between u_p and t_q,
the exact ties, the recurrence's drift on the entering columns and at the end,
and scipy's HiGHS optimum.  A case is refused when z differs from HiGHS by more
than Z_REL relative or when it has no phase-1 pivot.  `traced` is set only where
all three gaps are >= MIN_GAP: above it the pass sequence does not depend on the
fp64 summation order, and only such a case is compared pass for pass on the
device.  The optima of the shapes primal_phase1_optima.json holds must agree
with it, and the pivot counts must be below its Dantzig counts.

`infeasible`: boxed_general at INFEASIBLE_SHAPE made contradictory
(primal_phase1_ref.contradict): HiGHS calls it infeasible, the restatement's
counts up to INFEASIBLE, and HiGHS's optimum after rows 0 and 1 get the
right-hand side FEASIBLE_B01.

`stuck`: the warm start of primal_phase1_optima.json -- primal_box_ref.boxed_primal
at STUCK_SHAPE solved to the optimum under steepest edge
(tests/primal_box_se_ref.py), then cost_variant(c) and rhs_variant(b) on the same
basis with the weights the first solve left (spx_set_cost and spx_set_rhs keep
them): HiGHS's optimum of the new LP and the restatement's counts from there.

    python tests/golden/make_golden_primal_phase1_se.py
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
import primal_box_se_ref  # noqa: E402
import primal_phase1_se_ref as ref  # noqa: E402

TRACE = 200
MIN_GAP = 1e-6
Z_REL = 1e-9
SHAPES = [(7, 20, 0), (65, 200, 1), (130, 390, 2), (256, 1024, 3), (512, 2048, 4), (1024, 4096, 4)]
INFEASIBLE_SHAPE = (65, 200, 1)
FEASIBLE_B01 = (1000.0, 1000.0)
STUCK_SHAPE = (130, 390, 2)


def highs(A, b, c, u):
    bounds = [(0.0, None if not np.isfinite(x) else float(x)) for x in u]
    r = linprog(-c, A_eq=A, b_eq=b, bounds=bounds, method="highs")
    return r.status, (-float(r.fun) if r.status == 0 else None)


def counts(r):
    gap = min(r.gap_price, r.gap_ratio, r.gap_flip)
    return {"ref_pivots": r.pivots, "flips": r.flips, "to_upper": r.to_upper, "p1_passes": r.p1_passes,
            "p1_pivots": r.p1_pivots, "p1_flips": r.p1_passes - r.p1_pivots, "ninf0": r.ninf0,
            "gap_price": r.gap_price, "gap_ratio": r.gap_ratio, "gap_flip": r.gap_flip, "traced": bool(gap >= MIN_GAP),
            "ties": {k: int(v) for k, v in r.ties.items()}, "drift_enter": r.drift_enter, "drift_final": r.drift_final}


def check(name, r, hz, want=dual_ref.OPTIMUM, need_p1=True):
    if r.status != want:
        raise SystemExit(f"{name}: status {r.status}")
    if hz is not None:
        rel = abs(r.z - hz) / abs(hz)
        if rel > Z_REL:
            raise SystemExit(f"{name}: z differs from HiGHS by {rel:.1e} relative")
    if need_p1 and r.p1_pivots == 0:
        raise SystemExit(f"{name}: no phase-1 pivot")


def main():
    with open(os.path.join(HERE, "primal_phase1_optima.json")) as f:
        dz = json.load(f)
    dantzig = {(c["m"], c["n"], c["seed"]): c for c in dz["cases"]}
    out = {"generator": "tests/primal_phase1_ref.py boxed_general(m, n, seed)",
           "reference": "tests/primal_phase1_se_ref.py primal_simplex_phase1_se (first index on ties)",
           "min_gap": MIN_GAP, "cases": []}
    for (m, n, seed) in SHAPES:
        A, b, c, u = ref.boxed_general(m, n, seed)
        st, hz = highs(A, b, c, u)
        assert st == 0, (m, st)
        r = ref.primal_simplex_phase1_se(A, b, c, u, trace_cap=TRACE)
        print(f"m={m} n={n} seed={seed}: {r.status} z={r.z:.13g} (HiGHS {hz:.13g}, rel {abs(r.z - hz) / abs(hz):.1e}) "
              f"pivots={r.pivots} flips={r.flips} to_upper={r.to_upper} p1 passes={r.p1_passes} pivots={r.p1_pivots} "
              f"ninf0={r.ninf0} gaps {r.gap_price:.2e} {r.gap_ratio:.2e} {r.gap_flip:.2e} ties {r.ties} drift "
              f"{r.drift_enter:.1e} {r.drift_final:.1e}", flush=True)
        check(f"m={m}", r, hz)
        d = dantzig.get((m, n, seed))
        if d is not None:
            if abs(d["highs_z"] - hz) > 1e-12 * abs(hz):
                raise SystemExit(f"m={m}: HiGHS optimum {hz!r} differs from primal_phase1_optima.json's {d['highs_z']!r}")
            if not r.pivots < d["ref_pivots"]:
                raise SystemExit(f"m={m}: {r.pivots} pivots, Dantzig {d['ref_pivots']}")
        case = {"m": m, "n": n, "seed": seed, "highs_z": hz, "ref_z": r.z,
                "dantzig_pivots": d["ref_pivots"] if d is not None else None,
                "ref_trace_p": [int(p) for p, _ in r.trace], "ref_trace_q": [int(q) for _, q in r.trace],
                "ref_b_ixs": [int(j) for j in r.b_ixs], "ref_at_upper": [int(j) for j in np.flatnonzero(r.at_upper)]}
        case.update(counts(r))
        out["cases"].append(case)

    m, n, seed = INFEASIBLE_SHAPE
    A, b, c, u = ref.boxed_general(m, n, seed)
    A2, b2, u2 = ref.contradict(A, b, u)
    st, _ = highs(A2, b2, c, u2)
    assert st == 2, st
    r = ref.primal_simplex_phase1_se(A2, b2, c, u2, trace_cap=0)
    print(f"infeasible: {r.status} after {r.pivots} pivots, {r.p1_passes} phase-1 passes, ninf {r.ninf0} -> {r.ninf}, gaps "
          f"{r.gap_price:.2e} {r.gap_ratio:.2e} {r.gap_flip:.2e}", flush=True)
    check("infeasible", r, None, ref.INFEASIBLE)
    b3 = b2.copy()
    b3[0], b3[1] = FEASIBLE_B01
    st, hz = highs(A2, b3, c, u2)
    assert st == 0, st
    inf = {"m": m, "n": n, "seed": seed, "ninf_end": r.ninf, "feasible_b01": list(FEASIBLE_B01), "feasible_highs_z": hz,
           "dantzig_pivots": dz["infeasible"]["ref_pivots"]}
    inf.update(counts(r))
    out["infeasible"] = inf

    A, b, c, u = ref.tiny_infeasible()
    r = ref.primal_simplex_phase1_se(A, b, c, u)
    assert r.status == ref.INFEASIBLE and r.pivots == 0, (r.status, r.pivots)
    out["tiny_infeasible"] = {"ref_pivots": r.pivots, "p1_passes": r.p1_passes}

    m, n, seed = STUCK_SHAPE
    ns = n - m
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    first = primal_box_se_ref.primal_simplex_box_se(A, b, c, u, trace_cap=0)
    assert first.status == dual_ref.OPTIMUM
    c2 = primal_box_ref.cost_variant(c, ns, seed)
    b2 = ref.rhs_variant(b, seed)
    st, hz = highs(A, b2, c2, u)
    assert st == 0, st
    if abs(dz["stuck"]["highs_z"] - hz) > 1e-12 * abs(hz):
        raise SystemExit("stuck: HiGHS optimum differs from primal_phase1_optima.json's")
    r = ref.primal_simplex_phase1_se(A, b2, c2, u, basis=first.b_ixs, at_upper=first.at_upper, weights=first.weights,
                                     trace_cap=0)
    print(f"stuck: first solve {first.pivots} pivots; {r.status} z={r.z:.13g} (HiGHS {hz:.13g}) pivots={r.pivots} p1 "
          f"{r.p1_passes}/{r.p1_pivots} ninf0={r.ninf0} gaps {r.gap_price:.2e} {r.gap_ratio:.2e} {r.gap_flip:.2e}", flush=True)
    check("stuck", r, hz)
    stuck = {"m": m, "n": n, "seed": seed, "first_pivots": first.pivots, "highs_z": hz,
             "first_gap": min(first.gap_price, first.gap_ratio, first.gap_flip),
             "dantzig_pivots": dz["stuck"]["ref_pivots"]}
    stuck.update(counts(r))
    stuck["traced"] = bool(stuck["traced"] and stuck["first_gap"] >= MIN_GAP)
    out["stuck"] = stuck

    with open(os.path.join(HERE, "primal_phase1_se_optima.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
