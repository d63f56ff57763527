"""CPU: exact primal steepest-edge pricing for the bounded primal loop
(SPX_PRIMAL_PRICING_STEEPEST).  The numpy restatement
tests/primal_box_se_ref.py against its golden file
(tests/golden/primal_box_se_optima.json, written by
tests/golden/make_golden_primal_box_se.py), its pivot counts against the Dantzig
counts of tests/golden/primal_box_optima.json, the recurrence against the
recomputed weights, and the additions to the C-ABI, the Python package and the
CLI that need no device."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dual_ref
import primal_box_ref
import primal_box_se_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        g = json.load(f)
    g["by_shape"] = {(c["m"], c["n"], c["seed"]): c for c in g["cases"]}
    return g


@pytest.fixture(scope="module")
def golden():
    return _load("primal_box_se_optima.json")


@pytest.fixture(scope="module")
def dantzig():
    return _load("primal_box_optima.json")


@pytest.mark.parametrize("m,n,seed", dual_ref.TRACED)
def test_ref_reproduces_golden(golden, m, n, seed):
    g = golden["by_shape"][(m, n, seed)]
    A, b, c, u = ref.boxed_primal(m, n, seed)
    r = ref.primal_simplex_box_se(A, b, c, u, trace_cap=200)
    print(f"{m}x{n}: pivots={r.pivots} flips={r.flips} to_upper={r.to_upper} z={r.z:.13g} gaps {r.gap_price:.2e} "
          f"{r.gap_ratio:.2e} {r.gap_flip:.2e} drift {r.drift_enter:.2e} / {r.drift_final:.2e}")
    assert r.status == dual_ref.OPTIMUM
    assert r.pivots == g["ref_pivots"]
    assert [p for p, _ in r.trace] == g["ref_trace_p"]
    assert [q for _, q in r.trace] == g["ref_trace_q"]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(r.at_upper).tolist() == g["ref_at_upper"]
    assert (r.flips, r.to_upper) == (g["flips"], g["to_upper"])
    assert r.flips > 0 and r.to_upper > 0
    z = g["highs_z"]
    assert abs(r.z - z) <= 1e-9 * abs(z), (r.z, z)
    assert min(r.gap_price, r.gap_ratio, r.gap_flip) >= 1e-6
    assert min(g["gap_price"], g["gap_ratio"], g["gap_flip"]) >= golden["min_gap"] == 1e-6
    # the recurrence stays at the exactly recomputed weights (fp64 rounding over <= 421 pivots)
    assert r.drift <= 1e-9 and g["drift"] <= 1e-9
    viol, dviol, zc = primal_box_ref.certificate(A, b, c, u, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= 1e-9 * abs(z)


def test_golden_covers_every_shape(golden, dantzig):
    assert sorted(golden["by_shape"]) == sorted(dual_ref.SHAPES)
    for k, g in golden["by_shape"].items():
        d = dantzig["by_shape"][k]
        assert g["highs_z"] == d["highs_z"]  # the same LP, the same optimum
        assert abs(g["ref_z"] - g["highs_z"]) <= 1e-9 * abs(g["highs_z"])
        assert min(g["gap_price"], g["gap_ratio"], g["gap_flip"]) >= 1e-6
    res = golden["resolve"]
    assert (res["m"], res["n"], res["seed"]) == (256, 1024, 3) and [f["flipc"] for f in res["flipc"]] == [0, 1]
    for f, fd in zip(res["flipc"], dantzig["resolve"]["flipc"]):
        assert f["highs_z"] == fd["highs_z"] and f["ref_pivots"] > 0


@pytest.mark.parametrize("m,n,seed", dual_ref.SHAPES[1:])
def test_fewer_pivots_than_dantzig(golden, dantzig, m, n, seed):
    se, dz = golden["by_shape"][(m, n, seed)]["ref_pivots"], dantzig["by_shape"][(m, n, seed)]["ref_pivots"]
    print(f"{m}x{n}: steepest edge {se} pivots, Dantzig {dz}")
    assert se < dz


def test_recurrence_is_exact_in_exact_start_and_a_framework_otherwise():
    """From the slack basis the recurrence reproduces 1 + ||B^-1 A_j||^2 after
    40 pivots; restarted from that basis with given exact weights it walks on
    pass for pass; restarted with 1 + ||A_j||^2 it is a reference framework
    (the weights are not the exact norms) and still reaches the optimum."""
    m, n, seed = 65, 200, 1
    A, b, c, u = ref.boxed_primal(m, n, seed)
    full = ref.primal_simplex_box_se(A, b, c, u, trace_cap=1 << 20)
    part = ref.primal_simplex_box_se(A, b, c, u, max_iter=40)
    basic = np.zeros(n, dtype=bool)
    basic[part.b_ixs] = True
    ex = ref.exact_weights(A, part.Binv, basic)
    assert np.max(np.abs(part.weights[~basic] - ex[~basic]) / ex[~basic]) <= 1e-11
    cont = ref.primal_simplex_box_se(A, b, c, u, basis=part.b_ixs, at_upper=part.at_upper, weights=part.weights,
                                     trace_cap=1 << 20)
    assert cont.status == dual_ref.OPTIMUM and part.trace + cont.trace == full.trace
    warm = ref.primal_simplex_box_se(A, b, c, u, basis=part.b_ixs, at_upper=part.at_upper)
    assert warm.status == dual_ref.OPTIMUM and abs(warm.z - full.z) <= 1e-9 * abs(full.z)
    assert warm.drift_final > 1e-3  # not the exact norms


def test_header_and_bindings():
    with open(os.path.join(ROOT, "include", "simplex.h")) as f:
        h = f.read()
    for name, val in (("SPX_PRIMAL_PRICING_DANTZIG", 0), ("SPX_PRIMAL_PRICING_STEEPEST", 1),
                      ("SPX_FLAG_PRIMAL_STEEPEST", 16384), ("SPX_ABI_VERSION", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), h), name
    txt = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"int\s+spx_set_primal_pricing\(spx_ctx\*\s*ctx,\s*int32_t\s+rule\);", txt)
    assert re.search(r"int\s+spx_get_primal_weights\(spx_ctx\*\s*ctx,\s*double\*\s*w\s*\);", txt)
    import simplex_method_gpu_amd as spx
    from simplex_method_gpu_amd import _lib

    assert (spx.PRIMAL_PRICING_DANTZIG, spx.PRIMAL_PRICING_STEEPEST, spx.FLAG_PRIMAL_STEEPEST) == (0, 1, 16384)
    for name in ("PRIMAL_PRICING_DANTZIG", "PRIMAL_PRICING_STEEPEST", "FLAG_PRIMAL_STEEPEST"):
        assert name in spx.__all__
    assert callable(spx.Context.set_primal_pricing) and callable(spx.Context.primal_weights)
    L = _lib.load()
    assert L.spx_abi_version() == 8
    for name in ("spx_set_primal_pricing", "spx_get_primal_weights"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert L.spx_set_primal_pricing(None, spx.PRIMAL_PRICING_STEEPEST) == -1  # SPX_ERR_ARG
    assert b"NULL" in L.spx_last_error()
    assert L.spx_set_primal_pricing(None, 7) == -1
    w = np.zeros(4)
    assert L.spx_get_primal_weights(None, w.ctypes.data) == -1
    assert b"NULL" in L.spx_last_error()
    with pytest.raises(ValueError):
        spx.Context(m=4, n=8, seed=0, algorithm=spx.ALGO_PRIMAL_BOX, primal_pricing=7)


def test_cli_refuses_primal_pricing_without_primal_box():
    solver = os.path.join(ROOT, "solver")
    r = subprocess.run([solver, "--primal-pricing", "steepest", "--gen", "4", "8", "0"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "--primal-pricing" in r.stderr and "--primal-box" in r.stderr and "usage" in r.stderr
    r = subprocess.run([solver, "--primal-box", "--primal-pricing", "devex", "--gen", "4", "8", "0"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr
    r = subprocess.run([solver, "--help"], capture_output=True, text=True, timeout=60)
    assert "--primal-pricing" in r.stderr
