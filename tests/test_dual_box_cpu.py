"""CPU: boxed variables 0 <= x <= u in the dual simplex loop (spx_set_bounds;
DESIGN.md §7d).  The numpy restatement tests/dual_box_ref.py against its golden
file (tests/golden/dual_box_optima.json, written by
tests/golden/make_golden_dual_box.py: HiGHS optima of the bounded LPs, traces,
final bases and at-upper sets) at the four traced shapes, both flipc variants
and both leaving-row rules; with every bound infinite the reference is the
unbounded references' loop pivot for pivot; the additions to the C-ABI and the
CLI that need no device."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dual_box_ref as ref
import dual_ref
import dual_se_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def box_golden():
    with open(os.path.join(ROOT, "tests", "golden", "dual_box_optima.json")) as f:
        g = json.load(f)
    return {(c["m"], c["n"], c["seed"], c["flipc"], c["rule"]): c for c in g["cases"]}, g["resolve"]


@pytest.mark.parametrize("rule", [ref.DANTZIG, ref.STEEPEST])
@pytest.mark.parametrize("flipc", [0, 1])
@pytest.mark.parametrize("m,n,seed", dual_ref.TRACED)
def test_box_ref_reproduces_golden(box_golden, m, n, seed, flipc, rule):
    g = box_golden[0][(m, n, seed, flipc, rule)]
    A, b, c, u = ref.boxed(m, n, seed, bool(flipc))
    r = ref.dual_simplex_box(A, b, c, u, rule=rule, trace_cap=200)
    print(f"{m}x{n} flipc={flipc} {rule}: pivots={r.pivots} to_upper={r.to_upper} placed={r.placed} z={r.z:.13g} "
          f"gap_row={r.gap_row:.2e} gap_ratio={r.gap_ratio:.2e}")
    assert r.status == dual_ref.OPTIMUM
    assert r.pivots == g["ref_pivots"]
    assert [p for p, _ in r.trace] == g["ref_trace_p"]
    assert [q for _, q in r.trace] == g["ref_trace_q"]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(r.at_upper).tolist() == g["ref_at_upper"]
    z = g["highs_z"]
    assert abs(r.z - z) <= 1e-9 * abs(z), (r.z, z)
    # the boxed path is exercised: rows leave to upper bounds, columns end at them
    assert r.to_upper > 0 and len(g["ref_at_upper"]) > 0
    assert (r.placed > 0) == bool(flipc)
    # what makes the pivot-for-pivot comparison with the GPU legitimate
    assert min(r.gap_row, r.gap_ratio) >= 1e-6
    assert min(g["gap_row"], g["gap_ratio"]) >= 1e-6
    # the certificate from the basis and the placements alone
    viol, dviol, zc = ref.certificate(A, b, c, u, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= 1e-9 * abs(z)
    x = r.primal(u)
    assert np.max(np.abs(A @ x - b)) <= 1e-9 * np.max(np.abs(b))


def test_golden_covers_every_case(box_golden):
    cases, res = box_golden
    for (m, n, seed) in dual_ref.SHAPES:
        for flipc in (0, 1):
            assert (m, n, seed, flipc, ref.STEEPEST) in cases
    for k in ("tight_highs_z", "loose_highs_z", "tight_fresh_pivots_dantzig", "tight_fresh_pivots_steepest",
              "loose_fresh_pivots_dantzig", "loose_fresh_pivots_steepest"):
        assert k in res, k


def test_infinite_bounds_reproduce_the_unbounded_references():
    m, n, seed = dual_ref.SHAPES[1]
    A, b, c = dual_ref.covering(m, n, seed)
    u = np.full(n, np.inf)
    d0 = dual_ref.dual_simplex(A, b, c)
    d1 = ref.dual_simplex_box(A, b, c, u, rule=ref.DANTZIG)
    assert d1.status == d0.status == dual_ref.OPTIMUM
    assert d1.trace == d0.trace and d1.pivots == d0.pivots and d1.b_ixs.tolist() == d0.b_ixs.tolist()
    assert d1.z == d0.z and not d1.at_upper.any() and d1.to_upper == 0
    s0 = dual_se_ref.dual_simplex_se(A, b, c)
    s1 = ref.dual_simplex_box(A, b, c, u, rule=ref.STEEPEST)
    assert s1.trace == s0.trace and s1.pivots == s0.pivots and s1.b_ixs.tolist() == s0.b_ixs.tolist()
    assert s1.z == s0.z and (s1.gap_row, s1.gap_ratio) == (s0.gap_row, s0.gap_ratio)


def test_box_ref_refuses_a_column_without_a_bound():
    m, n, seed = dual_ref.SHAPES[0]
    A, b, c, u = ref.boxed(m, n, seed, True)
    j = int(np.flatnonzero(c > 0)[0])
    u = u.copy()
    u[j] = np.inf
    r = ref.dual_simplex_box(A, b, c, u)
    assert r.status == ref.NOT_DUAL_FEASIBLE and r.bad_column == j


def test_box_ref_reports_infeasible():
    for rule in (ref.DANTZIG, ref.STEEPEST):
        r = ref.dual_simplex_box(*ref.tiny_box_infeasible(), rule=rule)
        assert r.status == dual_ref.INFEASIBLE and r.pivots == 2, r
        A, b, c, u = ref.tiny_box_infeasible()
        row, margin = ref.farkas(A, b, u, r.b_ixs, r.at_upper)
        assert row >= 0 and abs(margin - 1.0) <= 1e-12  # x1 + x2 <= 1 against >= 2
    # ... and no such row at an optimum
    A, b, c, u = ref.boxed(7, 20, 0)
    r = ref.dual_simplex_box(A, b, c, u)
    assert ref.farkas(A, b, u, r.b_ixs, r.at_upper) == (-1, 0.0)


def test_new_functions_declared_and_exported(spx):
    L = spx._lib.load()
    txt = open(os.path.join(ROOT, "include", "simplex.h")).read()
    assert re.search(r"#define\s+SPX_ABI_VERSION\s+8\b", txt)
    assert L.spx_abi_version() == 8
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("spx_set_bounds", "spx_get_bounds", "spx_get_primal"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
        assert name in spx._lib.SIGNATURES
    v = np.zeros(4)
    assert L.spx_set_bounds(None, v.ctypes.data) == -1  # SPX_ERR_ARG
    assert b"NULL" in L.spx_last_error()
    assert L.spx_get_bounds(None, v.ctypes.data) == -1
    assert b"NULL" in L.spx_last_error()
    assert L.spx_get_primal(None, v.ctypes.data, None) == -1
    assert b"NULL" in L.spx_last_error()


def test_cli_usage_documents_bounds():
    r = subprocess.run([os.path.join(ROOT, "solver"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--bounds" in r.stderr
