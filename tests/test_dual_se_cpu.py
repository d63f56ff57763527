"""CPU: dual steepest-edge pricing (SPX_DUAL_PRICING_STEEPEST).
The numpy restatement tests/dual_se_ref.py against its golden file
(tests/golden/dual_se_optima.json, written by tests/golden/make_golden_dual_se.py)
and against the HiGHS optima of tests/golden/dual_optima.json; the weight update
formula against the row norms of the next inverse; the additions to the C-ABI,
the Python binding and the CLI."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dual_ref
import dual_se_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return {(c["m"], c["n"], c["seed"]): c for c in json.load(f)["cases"]}


@pytest.fixture(scope="module")
def se_golden():
    return _cases("dual_se_optima.json")


@pytest.fixture(scope="module")
def dual_golden():
    return _cases("dual_optima.json")


@pytest.mark.parametrize("m,n,seed", dual_ref.SHAPES)
def test_se_ref_reproduces_golden(se_golden, dual_golden, m, n, seed):
    g = se_golden[(m, n, seed)]
    z = dual_golden[(m, n, seed)]["highs_z"]
    r = dual_se_ref.dual_simplex_se(*dual_ref.covering(m, n, seed), trace_cap=200)
    print(f"{m}x{n}: pivots={r.pivots} z={r.z:.13g} gap_row={r.gap_row:.2e} gap_ratio={r.gap_ratio:.2e}")
    assert r.status == dual_ref.OPTIMUM
    assert r.pivots == g["ref_pivots"]
    assert [p for p, _ in r.trace] == g["ref_trace_p"]
    assert [q for _, q in r.trace] == g["ref_trace_q"]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert abs(r.z - z) <= 1e-9 * abs(z), (r.z, z)
    assert np.min(r.x_b) >= -1e-9
    # what makes the pivot-for-pivot comparison with the GPU legitimate
    assert min(r.gap_row, r.gap_ratio) >= 1e-6
    assert min(g["gap_row"], g["gap_ratio"]) >= 1e-6


def test_golden_pivot_counts(se_golden, dual_golden):
    """The five steepest-edge counts, and the Dantzig counts beside them agree
    with the Dantzig golden file where that has one."""
    assert [se_golden[s]["ref_pivots"] for s in dual_ref.SHAPES] == [5, 34, 52, 181, 632]
    for s in dual_ref.TRACED:
        assert se_golden[s]["dantzig_pivots"] == dual_golden[s]["ref_pivots"]
    assert se_golden[dual_ref.SHAPES[4]]["dantzig_pivots"] == 4289


@pytest.mark.parametrize("shape", [dual_ref.SHAPES[3], dual_ref.SHAPES[4]], ids=["256x1024", "1024x4096"])
def test_steepest_halves_the_pivots(se_golden, shape):
    g = se_golden[shape]
    assert 2 * g["ref_pivots"] <= g["dantzig_pivots"], (g["ref_pivots"], g["dantzig_pivots"])


def test_update_formula_gives_next_row_norms():
    """w' of the update formula against the squared row norms of the next
    inverse at every pivot of 130 x 390."""
    m, n, seed = dual_ref.SHAPES[2]
    r = dual_se_ref.dual_simplex_se(*dual_ref.covering(m, n, seed), check_update=True)
    print(f"largest relative distance over {r.pivots} pivots: {r.update_err:.2e}")
    assert r.status == dual_ref.OPTIMUM and r.pivots == 52
    assert r.update_err <= 1e-10


def test_se_ref_from_a_basis():
    """Started from a basis the Dantzig loop reached, the reference arrives at
    the same optimum."""
    m, n, seed = dual_ref.SHAPES[1]
    A, b, c = dual_ref.covering(m, n, seed)
    mid = dual_ref.dual_simplex(A, b, c, max_iter=10)
    assert mid.status == dual_ref.MAX_ITER and mid.pivots == 10
    r = dual_se_ref.dual_simplex_se(A, b, c, basis=mid.b_ixs)
    full = dual_ref.dual_simplex(A, b, c)
    assert r.status == dual_ref.OPTIMUM
    assert abs(r.z - full.z) <= 1e-9 * abs(full.z)
    assert sorted(r.b_ixs.tolist()) == sorted(full.b_ixs.tolist())


def test_se_ref_reports_infeasible():
    r = dual_se_ref.dual_simplex_se(*dual_ref.tiny_infeasible())
    assert r.status == dual_ref.INFEASIBLE and r.pivots == 1


def test_constants(spx):
    assert spx.DUAL_PRICING_DANTZIG == 0 and spx.DUAL_PRICING_STEEPEST == 1
    assert spx.FLAG_DUAL_STEEPEST == 2048
    txt = open(os.path.join(ROOT, "include", "simplex.h")).read()
    assert re.search(r"#define\s+SPX_FLAG_DUAL_STEEPEST\s+2048\b", txt)
    assert re.search(r"#define\s+SPX_DUAL_PRICING_DANTZIG\s+0\b", txt)
    assert re.search(r"#define\s+SPX_DUAL_PRICING_STEEPEST\s+1\b", txt)
    assert re.search(r"#define\s+SPX_ABI_VERSION\s+8\b", txt)
    assert spx._lib.load().spx_abi_version() == 8


def test_new_functions_declared_and_exported(spx):
    L = spx._lib.load()
    txt = open(os.path.join(ROOT, "include", "simplex.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("spx_set_dual_pricing", "spx_get_dual_weights"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
        assert name in spx._lib.SIGNATURES
    w = np.zeros(4)
    assert L.spx_set_dual_pricing(None, spx.DUAL_PRICING_STEEPEST) == -1  # SPX_ERR_ARG
    assert b"NULL" in L.spx_last_error()
    assert L.spx_get_dual_weights(None, w.ctypes.data) == -1
    assert b"NULL" in L.spx_last_error()


def test_binding_rejects_a_bad_rule_before_the_library(spx):
    with pytest.raises(ValueError):
        spx.Context(np.zeros((2, 1)), np.zeros(1), np.zeros(2), dual_pricing=7)


def test_cli_usage_documents_dual_pricing():
    r = subprocess.run([os.path.join(ROOT, "solver"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--dual-pricing" in r.stderr
    r = subprocess.run([os.path.join(ROOT, "solver"), "--dual", "--dual-pricing", "devex", "x"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr
