"""CPU: the dual simplex additions to the C-ABI and the Python binding (status 4,
SPX_ALGO_DUAL, spx_set_algorithm, spx_set_rhs), and the numpy restatement of
the dual loop (tests/dual_ref.py) against the golden values the GPU tests use
(tests/golden/dual_optima.json: scipy HiGHS optima and the reference's own
pivot traces, written by tests/golden/make_golden_dual.py)."""
import json
import os
import re

import numpy as np
import pytest

import dual_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dual_golden():
    with open(os.path.join(ROOT, "tests", "golden", "dual_optima.json")) as f:
        return {(c["m"], c["n"], c["seed"]): c for c in json.load(f)["cases"]}


def test_status_and_constants(spx):
    L = spx._lib.load()
    assert L.spx_status_string(4) == b"Problem infeasible."
    assert L.spx_status_string(1) == b"Optimum found"  # (unchanged)
    assert spx.ALGO_PRIMAL == 0 and spx.ALGO_DUAL == 1
    assert spx.SolveStatus.Infeasible == 4
    assert L.spx_abi_version() == 8


def test_new_functions_declared_and_exported(spx):
    L = spx._lib.load()
    txt = open(os.path.join(ROOT, "include", "simplex.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("spx_set_algorithm", "spx_set_rhs"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
    assert re.search(r"#define\s+SPX_ALGO_DUAL\s+1\b", txt)
    assert re.search(r"#define\s+SPX_STATUS_INFEASIBLE\s+4\b", txt)
    assert re.search(r"\bint32_t\s+algorithm\s*;", txt)
    b = np.zeros(4)
    assert L.spx_set_algorithm(None, spx.ALGO_DUAL) == -1  # SPX_ERR_ARG
    assert L.spx_set_rhs(None, b.ctypes.data) == -1
    assert b"NULL" in L.spx_last_error()


def test_cli_usage_documents_dual():
    import subprocess

    r = subprocess.run([os.path.join(ROOT, "solver"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--dual" in r.stderr


def test_opts_algorithm_defaults_to_primal(spx):
    import ctypes

    o = spx._lib.SpxOpts()
    o.algorithm = 7
    spx._lib.load().spx_default_opts(ctypes.byref(o))
    assert o.algorithm == spx.ALGO_PRIMAL
    # the renamed field is the struct's last int32, where `reserved` was
    assert spx._lib.SpxOpts.algorithm.offset == spx._lib.SpxOpts.trace_cap.offset + 4


@pytest.mark.parametrize("m,n,seed", dual_ref.TRACED)
def test_dual_ref_reproduces_golden(dual_golden, m, n, seed):
    g = dual_golden[(m, n, seed)]
    A, b, c = dual_ref.covering(m, n, seed)
    assert np.all(b < 0) and np.all(c <= 0)  # the slack basis: primal infeasible, dual feasible
    r = dual_ref.dual_simplex(A, b, c, trace_cap=200)
    assert r.status == dual_ref.OPTIMUM
    assert r.pivots == g["ref_pivots"]
    assert [p for p, _ in r.trace] == g["ref_trace_p"]
    assert [q for _, q in r.trace] == g["ref_trace_q"]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert abs(r.z - g["highs_z"]) <= 1e-9 * abs(g["highs_z"]), (r.z, g["highs_z"])
    assert np.min(r.x_b) >= -1e-9


def test_dual_ref_reports_infeasible():
    A, b, c = dual_ref.tiny_infeasible()
    r = dual_ref.dual_simplex(A, b, c)
    assert r.status == dual_ref.INFEASIBLE and r.pivots == 1
