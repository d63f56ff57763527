"""Generate tests/golden/primal_box_wexact_optima.json: the golden values of the
exact-weight tests of the bounded primal loop (tests/test_primal_box_wexact_cpu.py,
tests/test_gpu_primal_box_wexact.py).

`resolve`: the cost re-solve of make_golden_primal_box_se.py with the weights
started exactly.  The LP is tests/dual_box_ref.py boxed(m, n, seed, flipc); from
the boxed dual steepest-edge reference's optimal basis and placements the
objective becomes primal_box_ref.cost_variant(c) and the restatement
(tests/primal_box_se_ref.py) re-solves from weights = exact_weights(A,
inv(A[:, basis]), basic), what the library does under SPX_PRIMAL_WEIGHTS_EXACT
after spx_set_algorithm.  Stored per shape and flipc: pivots, flip passes,
to-upper pivots, the three gaps, the weight drift (entering columns, all
non-basic columns at the end), HiGHS's optimum, and beside them the pivot count
of the same re-solve from the reference framework 1 + ||A_j||^2; at 130 x 390
also the first 200 (p, q).  A case is refused ("pick another seed") when a gap
is below MIN_GAP, when z is off HiGHS by more than Z_REL relative, or, at
256 x 1024, when the exact start does not take fewer pivots than the reference
framework.  Every case passes with the seeds below.

`one_step`: the restatement's own weight error one pivot after an exact start:
40 Dantzig pivots on primal_box_ref.boxed_primal(m, n, seed), the exact weights
of that basis, one steepest-edge pivot, and the largest relative difference
between the recurrence's weights and the exact weights of the new basis.  The
GPU test's tolerance for a recurrence step on top of a refresh is 100 x this.

    python tests/golden/make_golden_primal_box_wexact.py
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
RESOLVE_SHAPES = [(130, 390, 2), (256, 1024, 3)]
TRACED_SHAPE = (130, 390, 2)
STRICT_SHAPE = (256, 1024, 3)  # the exact start must take fewer pivots here
ONE_STEP_SHAPES = [(65, 200, 1), (130, 390, 2)]
ONE_STEP_HEAD = 40


def highs(A, b, c, u):
    bounds = [(0.0, None if not np.isfinite(x) else float(x)) for x in u]
    r = linprog(-c, A_eq=A, b_eq=b, bounds=bounds, method="highs")
    return r.status, (-float(r.fun) if r.status == 0 else None)


def warm_weights(A, basis):
    basic = np.zeros(A.shape[1], dtype=bool)
    basic[basis] = True
    return ref.exact_weights(A, np.linalg.inv(A[:, basis]), basic)


def resolve(m, n, seed, flipc):
    """(exact-start result, reference-framework result, HiGHS z) of the re-solve."""
    A, b, c, u = dual_box_ref.boxed(m, n, seed, bool(flipc))
    first = dual_box_ref.dual_simplex_box(A, b, c, u, rule=dual_box_ref.STEEPEST, trace_cap=0)
    assert first.status == dual_ref.OPTIMUM
    c2 = primal_box_ref.cost_variant(c, n - m, seed)
    st, hz = highs(A, b, c2, u)
    assert st == 0, st
    w = warm_weights(A, first.b_ixs)
    r = ref.primal_simplex_box_se(A, b, c2, u, basis=first.b_ixs, at_upper=first.at_upper, weights=w, trace_cap=TRACE)
    r0 = ref.primal_simplex_box_se(A, b, c2, u, basis=first.b_ixs, at_upper=first.at_upper, trace_cap=0)
    return r, r0, hz


def resolve_case(m, n, seed, flipc):
    r, r0, hz = resolve(m, n, seed, flipc)
    name = f"re-solve {m}x{n} seed {seed} flipc={flipc}"
    assert r.status == dual_ref.OPTIMUM and r0.status == dual_ref.OPTIMUM, (r.status, r0.status)
    rel = abs(r.z - hz) / abs(hz)
    gap = min(r.gap_price, r.gap_ratio, r.gap_flip)
    print(f"{name}: z={hz:.13g} (HiGHS rel {rel:.1e}) pivots={r.pivots} (reference framework {r0.pivots}) "
          f"flips={r.flips} to_upper={r.to_upper} gap={gap:.2e} drift={r.drift_enter:.2e} / {r.drift_final:.2e}",
          flush=True)
    if rel > Z_REL or r.pivots == 0:
        raise SystemExit(f"{name}: z differs from HiGHS by {rel:.1e} relative, {r.pivots} pivots: pick another seed")
    if gap < MIN_GAP:
        raise SystemExit(f"{name}: a gap of {gap:.1e} is below {MIN_GAP:g}: pick another seed")
    if (m, n, seed) == STRICT_SHAPE and not r.pivots < r0.pivots:
        raise SystemExit(f"{name}: the exact start takes {r.pivots} pivots, the reference framework {r0.pivots}: "
                         "pick another seed")
    out = {"flipc": flipc, "highs_z": hz, "ref_pivots": r.pivots, "flips": r.flips, "to_upper": r.to_upper,
           "gap_price": r.gap_price, "gap_ratio": r.gap_ratio, "gap_flip": r.gap_flip,
           "drift_enter": r.drift_enter, "drift_final": r.drift_final, "reference_framework_pivots": r0.pivots}
    if (m, n, seed) == TRACED_SHAPE:
        out["ref_trace_p"] = [int(p) for p, _ in r.trace]
        out["ref_trace_q"] = [int(q) for _, q in r.trace]
    return out


def one_step(m, n, seed):
    """(weight error one pivot after an exact start, the (p, q) of that pivot)."""
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    head = primal_box_ref.primal_simplex_box(A, b, c, u, max_iter=ONE_STEP_HEAD, trace_cap=0)
    assert head.pivots == ONE_STEP_HEAD
    w = warm_weights(A, head.b_ixs)
    r = ref.primal_simplex_box_se(A, b, c, u, basis=head.b_ixs, at_upper=head.at_upper, weights=w, max_iter=1,
                                  trace_cap=1)
    assert r.pivots == 1, r.pivots
    return r.drift_final, r.trace[0]


def main():
    path = os.path.join(HERE, "primal_box_wexact_optima.json")
    out = {"generator": "tests/dual_box_ref.py boxed(m, n, seed, flipc), primal_box_ref.cost_variant",
           "reference": "tests/primal_box_se_ref.py primal_simplex_box_se(weights=exact_weights(...)) "
                        "(first index on ties)",
           "min_gap": MIN_GAP, "resolve": [], "one_step": []}
    for (m, n, seed) in RESOLVE_SHAPES:
        out["resolve"].append({"m": m, "n": n, "seed": seed,
                               "flipc": [resolve_case(m, n, seed, flipc) for flipc in (0, 1)]})
    for (m, n, seed) in ONE_STEP_SHAPES:
        err, (p, q) = one_step(m, n, seed)
        print(f"one step after an exact start, {m}x{n} seed {seed}: weight error {err:.2e} (pivot {p}, {q})", flush=True)
        out["one_step"].append({"m": m, "n": n, "seed": seed, "head_pivots": ONE_STEP_HEAD, "error": err,
                                "p": int(p), "q": int(q)})
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
