"""CPU: exact steepest-edge weights for a warm basis in the bounded primal loop
(SPX_PRIMAL_WEIGHTS_EXACT, spx_set_primal_weight_init, spx_refresh_primal_weights,
spx_pbox_wexact_times).  The numpy restatement against its golden
file (tests/golden/primal_box_wexact_optima.json, written by
tests/golden/make_golden_primal_box_wexact.py, whose functions this test runs
again), the exact start's pivot counts against the reference framework's, and
the additions to the C-ABI and the Python package that need no device."""
import importlib.util
import json
import os
import re

import pytest

import dual_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "simplex.h")
NEW_FUNCTIONS = ("spx_set_primal_weight_init", "spx_refresh_primal_weights", "spx_pbox_wexact_times")


def _json(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden():
    return _json("primal_box_wexact_optima.json")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location(
        "make_golden_primal_box_wexact", os.path.join(ROOT, "tests", "golden", "make_golden_primal_box_wexact.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_constants_and_prototypes():
    txt = open(HEADER).read()
    assert re.search(r"#define\s+SPX_PRIMAL_WEIGHTS_REFERENCE\s+0\b", txt)
    assert re.search(r"#define\s+SPX_PRIMAL_WEIGHTS_EXACT\s+1\b", txt)
    assert re.search(r"#define\s+SPX_FLAG_PRIMAL_EXACT_WEIGHTS\s+32768\b", txt)
    assert re.search(r"#define\s+SPX_ABI_VERSION\s+8\b", txt)
    assert re.search(r"int\s+spx_set_primal_weight_init\(spx_ctx\*\s*ctx,\s*int32_t\s+mode\);", txt)
    assert re.search(r"int\s+spx_refresh_primal_weights\(spx_ctx\*\s*ctx\);", txt)
    assert re.search(r"int\s+spx_pbox_wexact_times\(spx_ctx\*\s*ctx,\s*double\*\s*ms,\s*int64_t\*\s*launches\);", txt)


def test_binding_and_package(spx):
    L = spx._lib.load()
    assert L.spx_abi_version() == 8
    for name in NEW_FUNCTIONS:
        assert name in spx._lib.SIGNATURES and hasattr(L, name), name
    assert (spx.PRIMAL_WEIGHTS_REFERENCE, spx.PRIMAL_WEIGHTS_EXACT, spx.FLAG_PRIMAL_EXACT_WEIGHTS) == (0, 1, 32768)
    for name in ("set_primal_weight_init", "refresh_primal_weights", "wexact_times"):
        assert callable(getattr(spx.Context, name)), name
    # NULL contexts are refused before anything touches a device
    assert L.spx_set_primal_weight_init(None, 1) == -1
    assert L.spx_refresh_primal_weights(None) == -1
    assert L.spx_pbox_wexact_times(None, None, None) == -1


def test_context_refuses_an_unknown_mode(spx):
    with pytest.raises(ValueError, match="primal_weights"):
        spx.Context(m=4, n=8, seed=0, primal_weights=7)


@pytest.mark.parametrize("shape", [(130, 390, 2), (256, 1024, 3)])
@pytest.mark.parametrize("flipc", [0, 1])
def test_ref_reproduces_golden(golden, gen, shape, flipc):
    m, n, seed = shape
    case = {(c["m"], c["n"], c["seed"]): c for c in golden["resolve"]}[shape]
    g = case["flipc"][flipc]
    assert g["flipc"] == flipc
    r, r0, hz = gen.resolve(m, n, seed, flipc)
    print(f"{m}x{n} flipc={flipc}: exact start {r.pivots} pivots, reference framework {r0.pivots}; flips {r.flips}, "
          f"to upper {r.to_upper}, gaps {r.gap_price:.2e} {r.gap_ratio:.2e} {r.gap_flip:.2e}")
    assert r.status == dual_ref.OPTIMUM
    assert (r.pivots, r.flips, r.to_upper) == (g["ref_pivots"], g["flips"], g["to_upper"])
    assert r0.pivots == g["reference_framework_pivots"]
    for got, key in ((r.gap_price, "gap_price"), (r.gap_ratio, "gap_ratio"), (r.gap_flip, "gap_flip")):
        assert got == pytest.approx(g[key], rel=1e-6), key  # (a gap is a difference of keys: rounding moves its last digits)
    assert min(g["gap_price"], g["gap_ratio"], g["gap_flip"]) >= golden["min_gap"] == 1e-6
    assert abs(hz - g["highs_z"]) <= 1e-9 * abs(hz) and abs(r.z - hz) <= 1e-9 * abs(hz)
    # the start was exact: the recurrence stays at the exact norms (the drift itself is rounding noise)
    assert max(r.drift_enter, r.drift_final) <= 1e-9 and max(g["drift_enter"], g["drift_final"]) <= 1e-9
    if shape == (130, 390, 2):
        assert [p for p, _ in r.trace] == g["ref_trace_p"] and [q for _, q in r.trace] == g["ref_trace_q"]
        assert len(g["ref_trace_p"]) == min(200, g["ref_pivots"])


def test_exact_start_beats_the_reference_framework_at_256(golden):
    """Strictly fewer pivots than the counts primal_box_se_optima.json stores
    for the same re-solve from 1 + ||A_j||^2 (583 / 370)."""
    se = _json("primal_box_se_optima.json")["resolve"]
    assert (se["m"], se["n"], se["seed"]) == (256, 1024, 3)
    case = {(c["m"], c["n"], c["seed"]): c for c in golden["resolve"]}[(256, 1024, 3)]
    assert [f["ref_pivots"] for f in se["flipc"]] == [583, 370]
    for g, f in zip(case["flipc"], se["flipc"]):
        assert g["flipc"] == f["flipc"] and g["highs_z"] == f["highs_z"]
        assert g["reference_framework_pivots"] == f["ref_pivots"]
        assert g["ref_pivots"] < f["ref_pivots"], (g["ref_pivots"], f["ref_pivots"])


@pytest.mark.parametrize("k", [0, 1])
def test_one_step_error(golden, gen, k):
    g = golden["one_step"][k]
    assert (g["m"], g["n"], g["seed"]) == [(65, 200, 1), (130, 390, 2)][k] and g["head_pivots"] == 40
    err, (p, q) = gen.one_step(g["m"], g["n"], g["seed"])
    assert (int(p), int(q)) == (g["p"], g["q"])
    # rounding noise of one recurrence step: a few ulps of weights of order 1 to 100
    assert 0.0 < err <= 1e-13 and 0.0 < g["error"] <= 1e-13
