"""CPU: the bound-flipping (long-step) ratio test of the boxed dual simplex loop
(SPX_DUAL_RATIO_LONG_STEP).  The numpy restatement
tests/dual_long_ref.py against its golden file
(tests/golden/dual_long_optima.json, written by
tests/golden/make_golden_dual_long.py) and the HiGHS optima of
tests/golden/dual_box_optima.json at the four traced shapes; with bounds nothing
can flip the reference is tests/dual_box_ref.py's loop pivot for pivot; the tiny
infeasible LP; the certificate at 1024 x 4096; the additions to the C-ABI and
the CLI that need no device."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dual_long_ref as ref
import dual_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = [ref.DANTZIG, ref.STEEPEST]


def _load(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        g = json.load(f)
    return {(c["m"], c["n"], c["seed"], c["flipc"], c["rule"]): c for c in g["cases"]}


@pytest.fixture(scope="module")
def long_golden():
    return _load("dual_long_optima.json")


@pytest.fixture(scope="module")
def box_golden():
    return _load("dual_box_optima.json")


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("flipc", [0, 1])
@pytest.mark.parametrize("m,n,seed", dual_ref.TRACED)
def test_long_ref_reproduces_golden(long_golden, box_golden, m, n, seed, flipc, rule):
    g = long_golden[(m, n, seed, flipc, rule)]
    A, b, c, u = ref.boxed(m, n, seed, bool(flipc))
    r = ref.dual_simplex_long(A, b, c, u, rule=rule, trace_cap=200)
    print(f"{m}x{n} flipc={flipc} {rule}: pivots {g['textbook_pivots']} -> {r.pivots} flips={r.counters} "
          f"z={r.z:.13g} gap_row={r.gap_row:.2e} gap_walk={r.gap_walk:.2e} gap_slope={r.gap_slope:.2e}")
    assert r.status == dual_ref.OPTIMUM
    assert r.pivots == g["ref_pivots"]
    assert [p for p, _ in r.trace] == g["ref_trace_p"]
    assert [q for _, q in r.trace] == g["ref_trace_q"]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(r.at_upper).tolist() == g["ref_at_upper"]
    assert r.counters == (g["flips"], g["flip_passes"], g["max_flips"])
    z = box_golden[(m, n, seed, flipc, rule)]["highs_z"]
    assert g["highs_z"] == z
    assert abs(r.z - z) <= 1e-9 * abs(z), (r.z, z)
    # the long step is exercised and pays: flips happen, fewer pivots than the textbook test
    if m > 7:
        assert r.flips > 0 and r.max_flips > 1 and r.pivots < g["textbook_pivots"]
    # what makes the pivot-for-pivot comparison with the GPU legitimate
    assert min(r.gap_row, r.gap_walk, r.gap_slope) >= 1e-6
    assert min(g["gap_row"], g["gap_walk"], g["gap_slope"]) >= 1e-6
    viol, dviol, zc = ref.certificate(A, b, c, u, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= 1e-9 * abs(z)
    x = r.primal(u)
    assert np.max(np.abs(A @ x - b)) <= 1e-9 * np.max(np.abs(b))


def test_golden_covers_every_case(long_golden):
    for (m, n, seed) in dual_ref.SHAPES:
        for flipc in (0, 1):
            for rule in RULES:
                assert (m, n, seed, flipc, rule) in long_golden


@pytest.mark.parametrize("rule", RULES)
def test_textbook_ratio_is_the_boxed_reference(rule):
    m, n, seed = dual_ref.SHAPES[1]
    A, b, c, u = ref.boxed(m, n, seed, True)
    r0 = ref.dual_simplex_box(A, b, c, u, rule=rule)
    r1 = ref.dual_simplex_long(A, b, c, u, rule=rule, ratio=ref.TEXTBOOK)
    assert r1.trace == r0.trace and r1.pivots == r0.pivots and r1.z == r0.z
    assert r1.b_ixs.tolist() == r0.b_ixs.tolist() and np.array_equal(r1.at_upper, r0.at_upper)
    assert r1.counters == (0, 0, 0) and (r1.gap_row, r1.gap_ratio) == (r0.gap_row, r0.gap_ratio)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("big", [1e30, np.inf])
def test_bounds_nothing_can_flip(rule, big):
    """Every finite bound of boxed() replaced by 1e30 (or +inf): u_j (-ahat_j)
    exceeds every slope, the first candidate enters, and the trace is
    dual_simplex_box's on the same bounds."""
    m, n, seed = dual_ref.SHAPES[2]
    A, b, c, u = ref.boxed(m, n, seed)
    u = np.where(np.isfinite(u), big, u)
    r0 = ref.dual_simplex_box(A, b, c, u, rule=rule)
    r1 = ref.dual_simplex_long(A, b, c, u, rule=rule)
    assert r0.status == r1.status == dual_ref.OPTIMUM
    assert r1.trace == r0.trace and r1.pivots == r0.pivots and r1.z == r0.z
    assert r1.b_ixs.tolist() == r0.b_ixs.tolist() and np.array_equal(r1.x_b, r0.x_b)
    assert r1.counters == (0, 0, 0)


def test_long_ref_reports_infeasible():
    """x1 + x2 >= 2 with x1, x2 <= 0.5: the walk flips both candidates and none
    enters, so nothing is changed and no counter moves."""
    A, b, c, u = ref.tiny_box_infeasible()
    for rule in RULES:
        r = ref.dual_simplex_long(A, b, c, u, rule=rule)
        assert r.status == dual_ref.INFEASIBLE and r.pivots == 0, r
        assert not r.at_upper.any() and r.counters == (0, 0, 0)
        assert r.b_ixs.tolist() == [2, 3]
        row, margin = ref.farkas(A, b, u, r.b_ixs, r.at_upper)
        assert row >= 0 and abs(margin - 1.0) <= 1e-12


def test_certificate_1024_steepest(long_golden, box_golden):
    m, n, seed = dual_ref.SHAPES[4]
    A, b, c, u = ref.boxed(m, n, seed)
    g = long_golden[(m, n, seed, 0, ref.STEEPEST)]
    r = ref.dual_simplex_long(A, b, c, u, rule=ref.STEEPEST, trace_cap=0)
    z = box_golden[(m, n, seed, 0, ref.STEEPEST)]["highs_z"]
    print(f"{m}x{n}: pivots {g['textbook_pivots']} -> {r.pivots} flips={r.counters} z={r.z:.13g} (HiGHS {z:.13g})")
    assert r.status == dual_ref.OPTIMUM and r.pivots == g["ref_pivots"]
    assert r.counters == (g["flips"], g["flip_passes"], g["max_flips"])
    assert abs(r.z - z) <= 1e-9 * abs(z)
    viol, dviol, zc = ref.certificate(A, b, c, u, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= 1e-9 * abs(z)


def test_new_functions_declared_and_exported(spx):
    L = spx._lib.load()
    txt = open(os.path.join(ROOT, "include", "simplex.h")).read()
    for name, val in (("SPX_DUAL_RATIO_TEXTBOOK", 0), ("SPX_DUAL_RATIO_LONG_STEP", 1), ("SPX_FLAG_DUAL_LONG_STEP", 4096)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert (spx.DUAL_RATIO_TEXTBOOK, spx.DUAL_RATIO_LONG_STEP, spx.FLAG_DUAL_LONG_STEP) == (0, 1, 4096)
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("spx_set_dual_ratio", "spx_get_dual_flips"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
        assert name in spx._lib.SIGNATURES
    assert L.spx_set_dual_ratio(None, 1) == -1  # SPX_ERR_ARG
    assert b"NULL" in L.spx_last_error()
    out = np.zeros(3, dtype=np.int64)
    assert L.spx_get_dual_flips(None, out.ctypes.data) == -1
    assert b"NULL" in L.spx_last_error()


def test_cli_usage_documents_dual_ratio():
    solver = os.path.join(ROOT, "solver")
    r = subprocess.run([solver, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--dual-ratio" in r.stderr
    r = subprocess.run([solver, "--dual-ratio", "harris", "x"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
