"""CPU: the bounded primal simplex loop (SPX_ALGO_PRIMAL_BOX).
The numpy restatement tests/primal_box_ref.py against its golden file
(tests/golden/primal_box_optima.json, written by
tests/golden/make_golden_primal_box.py: HiGHS optima of the bounded LPs, traces,
final bases, at-upper sets, flip and to-upper counts) at the four traced shapes
and against the certificate; three hand-checkable LPs (a flip, an unbounded
column, a slack basis that is not primal feasible); with every bound infinite
the reference is the oracle's guarded loop; the additions to the C-ABI, the
Python package and the CLI that need no device."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dual_ref
import primal_box_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pbox_golden():
    with open(os.path.join(ROOT, "tests", "golden", "primal_box_optima.json")) as f:
        g = json.load(f)
    return {(c["m"], c["n"], c["seed"]): c for c in g["cases"]}, g["resolve"]


@pytest.mark.parametrize("m,n,seed", dual_ref.TRACED)
def test_ref_reproduces_golden(pbox_golden, m, n, seed):
    g = pbox_golden[0][(m, n, seed)]
    A, b, c, u = ref.boxed_primal(m, n, seed)
    r = ref.primal_simplex_box(A, b, c, u, trace_cap=200)
    print(f"{m}x{n}: pivots={r.pivots} flips={r.flips} to_upper={r.to_upper} z={r.z:.13g} "
          f"gap_price={r.gap_price:.2e} gap_ratio={r.gap_ratio:.2e} gap_flip={r.gap_flip:.2e}")
    assert r.status == dual_ref.OPTIMUM
    assert r.pivots == g["ref_pivots"]
    assert [p for p, _ in r.trace] == g["ref_trace_p"]
    assert [q for _, q in r.trace] == g["ref_trace_q"]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(r.at_upper).tolist() == g["ref_at_upper"]
    assert (r.flips, r.to_upper) == (g["flips"], g["to_upper"])
    z = g["highs_z"]
    assert abs(r.z - z) <= 1e-9 * abs(z), (r.z, z)
    # the bounded path is exercised: flip passes, rows leaving to upper bounds, columns ending at them
    assert r.flips > 0 and r.to_upper > 0 and len(g["ref_at_upper"]) > 0
    # what makes the pivot-for-pivot comparison with the GPU legitimate
    assert min(r.gap_price, r.gap_ratio, r.gap_flip) >= 1e-6
    assert min(g["gap_price"], g["gap_ratio"], g["gap_flip"]) >= 1e-6
    # the certificate from the basis and the placements alone
    viol, dviol, zc = ref.certificate(A, b, c, u, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= 1e-9 * abs(z)
    x = r.primal(u)
    assert np.max(np.abs(A @ x - b)) <= 1e-9 * np.max(np.abs(b))
    assert np.array_equal(x[r.at_upper], u[r.at_upper])


def test_golden_covers_every_case(pbox_golden):
    cases, res = pbox_golden
    for s in dual_ref.SHAPES:
        assert s in cases
        assert min(cases[s]["gap_price"], cases[s]["gap_ratio"], cases[s]["gap_flip"]) >= 1e-6
    assert (res["m"], res["n"], res["seed"]) == (256, 1024, 3)
    assert [f["flipc"] for f in res["flipc"]] == [0, 1]
    for f in res["flipc"]:
        assert f["ref_pivots"] > 0 and f["flips"] > 0 and f["to_upper"] > 0


def test_warm_start_and_pivot_limit():
    """A solve stopped after 40 pivots and continued from its basis and
    placements ends where the uninterrupted one does."""
    m, n, seed = dual_ref.SHAPES[1]
    A, b, c, u = ref.boxed_primal(m, n, seed)
    full = ref.primal_simplex_box(A, b, c, u)
    part = ref.primal_simplex_box(A, b, c, u, max_iter=40)
    assert part.status == dual_ref.MAX_ITER and part.pivots == 40 and part.trace == full.trace[:40]
    rest = ref.primal_simplex_box(A, b, c, u, basis=part.b_ixs, at_upper=part.at_upper)
    assert rest.status == dual_ref.OPTIMUM and rest.pivots == full.pivots - 40
    assert rest.b_ixs.tolist() == full.b_ixs.tolist() and np.array_equal(rest.at_upper, full.at_upper)
    assert abs(rest.z - full.z) <= 1e-12 * abs(full.z)


def test_infinite_bounds_are_the_guarded_primal_loop():
    """Every bound +inf: no flips, no row to upper, and an optimum of the LP
    without bounds by the certificate."""
    m, n, seed = dual_ref.SHAPES[1]
    A, b, c, _ = ref.boxed_primal(m, n, seed)
    u = np.full(n, np.inf)
    A = np.abs(A)  # (A >= 0 and b > 0: the LP has an optimum without bounds)
    r = ref.primal_simplex_box(A, b, c, u)
    assert r.status == dual_ref.OPTIMUM and r.flips == 0 and r.to_upper == 0 and not r.at_upper.any()
    viol, dviol, zc = ref.certificate(A, b, c, u, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7 and abs(zc - r.z) <= 1e-9 * abs(r.z)


def test_tiny_flip():
    A, b, c, u = ref.tiny_flip()
    r = ref.primal_simplex_box(A, b, c, u)
    assert r.status == dual_ref.OPTIMUM and (r.pivots, r.flips, r.to_upper) == (1, 1, 0)
    assert r.trace == [(1, 0)] and r.b_ixs.tolist() == [1]
    assert np.flatnonzero(r.at_upper).tolist() == [0]
    assert r.primal(u).tolist() == [1.0, 3.0, 0.0] and r.z == 5.0


def test_tiny_unbounded():
    r = ref.primal_simplex_box(*ref.tiny_unbounded())
    assert r.status == ref.UNBOUNDED and r.pivots == 1 and r.trace == [(0, 0)]


def test_tiny_not_primal_feasible():
    r = ref.primal_simplex_box(*ref.tiny_not_feasible())
    assert r.status == ref.NOT_PRIMAL_FEASIBLE and (r.bad_row, r.bad_column) == (1, 3) and r.pivots == 0
    # ... and a bounded slack below its b_i is the same refusal
    A, b, c, u = ref.tiny_flip()
    u = u.copy()
    u[2] = 3.0
    r = ref.primal_simplex_box(A, b, c, u)
    assert r.status == ref.NOT_PRIMAL_FEASIBLE and (r.bad_row, r.bad_column) == (0, 2)


def test_header_constants():
    txt = open(os.path.join(ROOT, "include", "simplex.h")).read()
    assert re.search(r"#define\s+SPX_ALGO_PRIMAL_BOX\s+2\b", txt)
    assert re.search(r"#define\s+SPX_ABI_VERSION\s+8\b", txt)
    assert re.search(r"#define\s+SPX_CONFIG_FIELDS\s+17\b", txt)


def test_new_functions_declared_and_exported(spx):
    L = spx._lib.load()
    assert L.spx_abi_version() == 8
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simplex.h")).read(), flags=re.S)
    for name in ("spx_set_cost", "spx_get_primal_flips"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
        assert name in spx._lib.SIGNATURES
    v = np.zeros(4)
    assert L.spx_set_cost(None, v.ctypes.data) == -1  # SPX_ERR_ARG
    assert b"NULL" in L.spx_last_error()
    assert L.spx_get_primal_flips(None, v.ctypes.data) == -1
    assert b"NULL" in L.spx_last_error()


def test_python_constants(spx):
    assert (spx.ALGO_PRIMAL, spx.ALGO_DUAL, spx.ALGO_PRIMAL_BOX) == (0, 1, 2)
    assert "ALGO_PRIMAL_BOX" in spx.__all__
    assert callable(spx.Context.set_cost) and callable(spx.Context.primal_flips)


def test_cli_usage_and_refusals():
    solver = os.path.join(ROOT, "solver")
    r = subprocess.run([solver, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--primal-box" in r.stderr
    sample = os.path.join(ROOT, "tests", "golden", "sample.txt")
    for extra, word in ((["--dual"], "--dual"), (["--mps"], "--mps"), (["--window", "8"], "--window"),
                        (["--tableau"], "--tableau")):
        r = subprocess.run([solver, "--primal-box"] + extra + [sample], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--primal-box" in r.stderr and word in r.stderr, (extra, r.stderr)
