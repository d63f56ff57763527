"""Generate tests/golden/primal_lu_optima.json: the golden values of the
general-bounds tests (tests/test_primal_lu_cpu.py, tests/test_gpu_primal_lu.py).

`cases`: for every LP of tests/primal_lu_ref.py general_lu(m, n, seed) at SHAPES
(finite lower bounds of either sign, fixed columns, free columns), from the
slack basis: the numpy restatement's (tests/primal_lu_ref.py primal_simplex_lu)
optimum, pivot count, first 200 (p, q) pairs, final basis and at-upper set, the
flip and to-upper counts, the phase-1 counters, the smallest relative gaps of
the two argmins and between u_p and t_q, and scipy's HiGHS optimum with
bounds=list(zip(l, u)).  A case is refused by make_golden_primal_phase1.py's
rule: z differs from HiGHS by more than Z_REL, a gap is below MIN_GAP (above it
the pass sequence does not depend on the fp64 summation order), or there is no
phase-1 pivot; it is also refused when no free column ever enters.  Pick
another seed.

`shift`: primal_lu_ref.shift_lp at SHIFT_SHAPE (lower bounds and fixed columns
only, every range finite: both bounded loops take its slack basis): HiGHS's
optimum, its optimum after tests/primal_phase1_ref.py rhs_variant(b), its
optimum after primal_lu_ref.moved_lower(l) on top of that, and the
restatement's counts from the slack basis.

`infeasible`: general_lu at INFEASIBLE_SHAPE made contradictory
(primal_phase1_ref.contradict); HiGHS must call it infeasible (status 2).

`unbounded`: primal_lu_ref.tiny_unbounded_free(); HiGHS must call it unbounded
(status 3) and the restatement must get there with sigma = -1 and no pivot.

    python tests/golden/make_golden_primal_lu.py
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
import primal_lu_ref as ref  # noqa: E402
import primal_phase1_ref  # noqa: E402

TRACE = 200
MIN_GAP = 1e-6
Z_REL = 1e-9
SHAPES = [(7, 20, 0), (65, 200, 1), (130, 390, 2), (256, 1024, 3)]
SHIFT_SHAPE = (65, 200, 1)
INFEASIBLE_SHAPE = (65, 200, 1)


def highs(A, b, c, l, u):
    bounds = [(None if not np.isfinite(lo) else float(lo), None if not np.isfinite(hi) else float(hi))
              for lo, hi in zip(l, u)]
    r = linprog(-c, A_eq=A, b_eq=b, bounds=bounds, method="highs")
    return r.status, (-float(r.fun) if r.status == 0 else None)


def counts(r):
    return {"ref_pivots": r.pivots, "flips": r.flips, "to_upper": r.to_upper, "p1_passes": r.p1_passes,
            "p1_pivots": r.p1_pivots, "ninf0": r.ninf0, "gap_price": r.gap_price, "gap_ratio": r.gap_ratio,
            "gap_flip": r.gap_flip}


def check(name, r, hz, want=dual_ref.OPTIMUM, need_p1=True):
    if r.status != want:
        raise SystemExit(f"{name}: status {r.status}")
    gap = min(r.gap_price, r.gap_ratio, r.gap_flip)
    if gap < MIN_GAP:
        raise SystemExit(f"{name}: a gap of {gap:.1e} is below {MIN_GAP:g}: pick another seed")
    if hz is not None:
        rel = abs(r.z - hz) / abs(hz)
        if rel > Z_REL:
            raise SystemExit(f"{name}: z differs from HiGHS by {rel:.1e} relative")
    if need_p1 and r.p1_pivots == 0:
        raise SystemExit(f"{name}: no phase-1 pivot")


def main():
    out = {"generator": "tests/primal_lu_ref.py general_lu(m, n, seed)",
           "reference": "tests/primal_lu_ref.py primal_simplex_lu (first index on ties)",
           "min_gap": MIN_GAP, "cases": []}
    for (m, n, seed) in SHAPES:
        A, b, c, l, u = ref.general_lu(m, n, seed)
        st, hz = highs(A, b, c, l, u)
        assert st == 0, (m, st)
        r = ref.primal_simplex_lu(A, b, c, l, u, trace_cap=1 << 30)
        free = np.isneginf(l)
        free_entered = int(sum(bool(free[p]) for p, _ in r.trace))
        free_basic = int(np.count_nonzero(free[r.b_ixs]))
        print(f"m={m} n={n} seed={seed}: {r.status} z={r.z:.13g} (HiGHS {hz:.13g}) pivots={r.pivots} flips={r.flips} "
              f"to_upper={r.to_upper} p1 passes={r.p1_passes} pivots={r.p1_pivots} ninf0={r.ninf0} free columns "
              f"{int(free.sum())} (entered {free_entered}, basic at the end {free_basic}) lower {int(np.count_nonzero(np.isfinite(l) & (l != 0)))} "
              f"fixed {int(np.count_nonzero(l == u))} gaps {r.gap_price:.2e} {r.gap_ratio:.2e} {r.gap_flip:.2e}", flush=True)
        check(f"m={m}", r, hz)
        if free_entered == 0:
            raise SystemExit(f"m={m}: no free column enters")
        tr = r.trace[:TRACE]
        case = {"m": m, "n": n, "seed": seed, "highs_z": hz, "ref_z": r.z,
                "ref_trace_p": [int(p) for p, _ in tr], "ref_trace_q": [int(q) for _, q in tr],
                "ref_b_ixs": [int(j) for j in r.b_ixs], "ref_at_upper": [int(j) for j in np.flatnonzero(r.at_upper)],
                "free_entered": free_entered, "free_basic": free_basic}
        case.update(counts(r))
        out["cases"].append(case)

    m, n, seed = SHIFT_SHAPE
    A, b, c, l, u = ref.shift_lp(m, n, seed)
    st, hz = highs(A, b, c, l, u)
    assert st == 0, st
    r = ref.primal_simplex_lu(A, b, c, l, u, trace_cap=TRACE)
    print(f"shift: {r.status} z={r.z:.13g} (HiGHS {hz:.13g}) pivots={r.pivots} p1 {r.p1_passes}/{r.p1_pivots}", flush=True)
    check("shift", r, hz)
    b2 = primal_phase1_ref.rhs_variant(b, seed)
    st, hz_b = highs(A, b2, c, l, u)
    assert st == 0, st
    l2 = ref.moved_lower(l, u, seed)
    assert np.any(l2 != l)
    st, hz_l = highs(A, b2, c, l2, u)
    assert st == 0, st
    shift = {"m": m, "n": n, "seed": seed, "highs_z": hz, "ref_z": r.z, "rhs_highs_z": hz_b, "lower_highs_z": hz_l,
             "ref_trace_p": [int(p) for p, _ in r.trace], "ref_trace_q": [int(q) for _, q in r.trace],
             "ref_b_ixs": [int(j) for j in r.b_ixs], "ref_at_upper": [int(j) for j in np.flatnonzero(r.at_upper)]}
    shift.update(counts(r))
    out["shift"] = shift

    m, n, seed = INFEASIBLE_SHAPE
    A, b, c, l, u = ref.general_lu(m, n, seed)
    A2, b2, u2 = primal_phase1_ref.contradict(A, b, u)
    l2 = l.copy()
    l2[n - m], l2[n - m + 1] = 0.0, 0.0  # (contradict's two slacks: 0 <= s, no upper bound)
    st, _ = highs(A2, b2, c, l2, u2)
    assert st == 2, st
    r = ref.primal_simplex_lu(A2, b2, c, l2, u2, trace_cap=0)
    print(f"infeasible: {r.status} after {r.pivots} pivots, ninf {r.ninf0} -> {r.ninf}", flush=True)
    check("infeasible", r, None, primal_phase1_ref.INFEASIBLE)
    inf = {"m": m, "n": n, "seed": seed, "ninf_end": r.ninf}
    inf.update(counts(r))
    out["infeasible"] = inf

    A, b, c, l, u = ref.tiny_unbounded_free()
    st, _ = highs(A, b, c, l, u)
    assert st == 3, st
    r = ref.primal_simplex_lu(A, b, c, l, u)
    assert r.status == ref.UNBOUNDED and r.pivots == 0 and r.flips == 0, (r.status, r.pivots)
    out["unbounded"] = {"highs_status": st, "ref_pivots": r.pivots}

    with open(os.path.join(HERE, "primal_lu_optima.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
