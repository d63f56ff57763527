"""CPU: exact ties in the dual, boxed dual, long-step, bounded primal and
phase-1 loops, and under general bounds with free columns.  The numpy
restatements (tests/*_ref.py, through
tests/tied_lp.py case_ref) on the integer interval-matrix LPs of
tests/tied_lp.py against their golden file (tests/golden/tied_optima.json,
written by tests/golden/make_golden_tied.py): the recorded passes, HiGHS's
status and optimum met exactly, integers only along the whole run, and the
tie counters that show each first-index rule was in fact exercised.

The tiny cases pin the long-step slope rule `slope' <= 0: the column enters`:
under `slope' < 0` exact_capacity() (x1 + x2 >= 3, u = (1, 2)) flips both
columns, runs out of candidates and is reported infeasible, as are a third of
the 7 x 20 LPs of test_long_step_small_lps.
"""
import json
import os

import numpy as np
import pytest

import dual_long_ref
import dual_ref
import primal_box_ref
import primal_phase1_ref
import tied_lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "tied_optima.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
IDS = [f"{g['variant']}-{g['m']}x{g['n']}" for g in GOLDEN]
COUNTERS = ("to_upper", "placed", "flips", "flip_passes", "max_flips", "walk_run", "p1_passes", "p1_pivots", "ninf0",
            "ninf", "free_entered", "free_basic", "fixed_flips", "ray_col")


def test_golden_covers_every_variant_and_shape():
    assert [(g["variant"], g["m"], g["n"]) for g in GOLDEN] == \
        [(v, m, n) for v in tied_lp.VARIANTS for (m, n) in tied_lp.shapes(v)]
    assert all(tied_lp.shapes(v) == tied_lp.SHAPES for v in tied_lp.VARIANTS if v != "free_unbounded")


@pytest.mark.parametrize("g", GOLDEN, ids=IDS)
def test_reference_reproduces_golden(g):
    lp = tied_lp.case_lp(g["variant"], g["m"], g["n"], g["seed"], bool(g["mixed"]))
    for v in lp:
        assert np.all((v == np.rint(v)) | np.isinf(v))
    r = tied_lp.case_ref(g["variant"], lp, trace_cap=200)
    print(f"{g['variant']} {g['m']}x{g['n']} seed={g['seed']}: {r.status} z={r.z} pivots={r.pivots} ties={r.ties}")
    assert r.status == g["ref_status"] == g["highs_status"]
    if g["highs_z"] is not None:
        assert r.z == g["highs_z"]  # exactly: both are integers
    assert r.pivots == g["ref_pivots"]
    assert [p for p, _ in r.trace] == g["ref_trace_p"]
    assert [q for _, q in r.trace] == g["ref_trace_q"]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(getattr(r, "at_upper", [])).tolist() == g["ref_at_upper"]
    for k in COUNTERS:
        assert (getattr(r, k) if hasattr(r, k) else None) == g.get(k), k
    assert r.integral  # x_b, y and B^-1 after every pass
    for v in (r.x_b, r.y, r.Binv):
        assert np.array_equal(v, np.rint(v))
    assert {k: r.ties[k] for k in tied_lp.VARIANTS[g["variant"]]} == g["ties"]


@pytest.mark.parametrize("g", [g for g in GOLDEN if g["m"] >= 65], ids=[i for g, i in zip(GOLDEN, IDS) if g["m"] >= 65])
def test_every_tie_rule_is_exercised(g):
    """At 65 x 200 and larger every tie counter that applies to the loop is at
    least 1, and every long-step case walks at least 3 consecutive equal keys."""
    assert set(g["ties"]) == set(tied_lp.VARIANTS[g["variant"]])
    assert all(v >= 1 for v in g["ties"].values()), g["ties"]
    if g["variant"].startswith("long_"):
        assert g["walk_run"] >= 3 and g["flips"] > 0


LU = [g for g in GOLDEN if g["variant"] in tied_lp.LU_VARIANTS]


@pytest.mark.parametrize("g", LU, ids=[i for g, i in zip(GOLDEN, IDS) if g["variant"] in tied_lp.LU_VARIANTS])
def test_free_rules_are_exercised(g):
    """At every shape of the general-bounds variants: a free column enters and
    one is basic at the end, a pricing tie has a free column among the tied
    minima, a fixed column enters and flips at once; the unbounded case ends on
    a free entering column.  The LP itself has fixed columns and free columns
    and, at 65 x 200 and larger (7 x 20 has three free columns and one fixed),
    lower bounds and free columns' costs of both signs."""
    A, b, c, l, u = tied_lp.case_lp(g["variant"], g["m"], g["n"], g["seed"])
    free = np.isneginf(l)
    assert free.any() and np.all(np.isposinf(u[free])) and np.any(l == u)
    if g["m"] >= 65:
        assert np.any(c[free] > 0) and np.any(c[free] < 0) and np.any(l[~free] < 0) and np.any(l[~free] > 0)
    assert np.all(np.isfinite(u[~free]))  # every other column, slacks included, has a finite range
    assert g["free_entered"] > 0 and g["free_basic"] > 0 and g["fixed_flips"] > 0 and g["ties"]["free_price"] > 0
    if g["variant"] == "free_unbounded":
        assert g["ref_status"] == "unbounded" and free[g["ray_col"]]
    else:
        assert g["ref_status"] == "optimum" and g["ray_col"] == -1


def test_exact_capacity_is_an_optimum():
    A, b, c, u = tied_lp.exact_capacity()
    for rule in (dual_long_ref.DANTZIG, dual_long_ref.STEEPEST):
        r = dual_long_ref.dual_simplex_long(A, b, c, u, rule=rule)
        assert r.status == dual_ref.OPTIMUM and r.z == -5.0 and r.pivots == 1
        assert r.primal(u).tolist() == [1.0, 2.0, 0.0]
        assert r.counters == (1, 1, 1) and r.ties["slope0"] == 1
        assert r.trace == [(1, 0)] and np.flatnonzero(r.at_upper).tolist() == [0]
        t = dual_long_ref.dual_simplex_long(A, b, c, u, rule=rule, ratio=dual_long_ref.TEXTBOOK)
        assert t.status == dual_ref.OPTIMUM and t.z == -5.0 and t.counters == (0, 0, 0)


def test_short_capacity_is_infeasible():
    A, b, c, u = tied_lp.short_capacity()
    for ratio in (dual_long_ref.LONG_STEP, dual_long_ref.TEXTBOOK):
        r = dual_long_ref.dual_simplex_long(A, b, c, u, ratio=ratio)
        assert r.status == dual_ref.INFEASIBLE
        if ratio == dual_long_ref.LONG_STEP:
            assert r.pivots == 0 and r.counters == (0, 0, 0) and not r.at_upper.any()


@pytest.mark.parametrize("mixed", [False, True])
def test_long_step_small_lps(mixed):
    """60 boxed 7 x 20 covering LPs, feasible by construction: the long-step
    loop reaches the textbook loop's optimum exactly under both row rules.
    (With `slope' < 0` 40 of the 120 runs end in a false "infeasible" without
    `mixed`, 34 with it.)"""
    for seed in range(60):
        lp = tied_lp.tied_covering(7, 20, seed, True, mixed)
        want = dual_long_ref.dual_simplex_long(*lp, ratio=dual_long_ref.TEXTBOOK, max_iter=500)
        assert want.status == dual_ref.OPTIMUM, seed
        for rule in (dual_long_ref.DANTZIG, dual_long_ref.STEEPEST):
            r = dual_long_ref.dual_simplex_long(*lp, rule=rule, max_iter=500)
            assert r.status == dual_ref.OPTIMUM and r.z == want.z and r.integral, (seed, rule, r.status, r.z, want.z)


def test_flip_tie():
    """u_p == t_q exactly: the pass is a flip, in both bounded primal references."""
    A, b, c, u = tied_lp.flip_tie()
    for solve in (primal_box_ref.primal_simplex_box, primal_phase1_ref.primal_simplex_phase1):
        r = solve(A, b, c, u)
        assert r.status == dual_ref.OPTIMUM and r.z == 6.0
        assert r.flips == 1 and r.pivots == 1 and r.ties["flip"] == 1
        assert r.primal(u).tolist() == [3.0, 0.0, 0.0] and r.trace == [(1, 0)]


def test_default_results_unchanged():
    """The additions to the references are counters only: a run on a generic LP
    reports no tie and the fields the other golden files rest on are there."""
    A, b, c = dual_ref.covering(7, 20, 0)
    r = dual_ref.dual_simplex(A, b, c)
    assert r.status == dual_ref.OPTIMUM and r.ties == {"row": 0, "ratio": 0} and not r.integral
    assert np.allclose(r.y @ A[:, r.b_ixs], c[r.b_ixs], atol=1e-9)
