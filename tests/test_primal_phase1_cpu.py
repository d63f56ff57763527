"""CPU: the bounded primal loop's phase 1 (SPX_FLAG_PRIMAL_PHASE1; DESIGN.md
§7f).  The numpy restatement tests/primal_phase1_ref.py against its golden file
(tests/golden/primal_phase1_optima.json, written by
tests/golden/make_golden_primal_phase1.py: HiGHS optima, traces, final bases,
flip / to-upper / phase-1 counts) and against the certificate; the number of
infeasible rows never grows; a feasible entry is primal_box_ref's loop pass for
pass; hand-checkable LPs; the additions to the C-ABI, the Python package and
the CLI that need no device."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dual_ref
import primal_box_ref
import primal_phase1_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "primal_phase1_optima.json")) as f:
        g = json.load(f)
    g["by_shape"] = {(c["m"], c["n"], c["seed"]): c for c in g["cases"]}
    return g


@pytest.mark.parametrize("m,n,seed", [(7, 20, 0), (65, 200, 1), (130, 390, 2), (256, 1024, 3)])
def test_ref_reproduces_golden(golden, m, n, seed):
    g = golden["by_shape"][(m, n, seed)]
    A, b, c, u = ref.boxed_general(m, n, seed)
    # what the generator promises: the slack basis is feasible on neither side
    assert np.any(b < 0) and np.any(b > u[n - m:]) and np.any((c > 1e-3) & ~np.isfinite(u))
    r = ref.primal_simplex_phase1(A, b, c, u, trace_cap=200)
    print(f"{m}x{n}: pivots={r.pivots} flips={r.flips} to_upper={r.to_upper} phase 1 {r.p1_passes}/{r.p1_pivots} "
          f"ninf0={r.ninf0} z={r.z:.13g} gaps {r.gap_price:.2e} {r.gap_ratio:.2e} {r.gap_flip:.2e}")
    assert r.status == dual_ref.OPTIMUM
    assert r.pivots == g["ref_pivots"]
    assert [p for p, _ in r.trace] == g["ref_trace_p"]
    assert [q for _, q in r.trace] == g["ref_trace_q"]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(r.at_upper).tolist() == g["ref_at_upper"]
    assert (r.flips, r.to_upper) == (g["flips"], g["to_upper"])
    assert (r.p1_passes, r.p1_pivots, r.ninf0, r.ninf) == (g["p1_passes"], g["p1_pivots"], g["ninf0"], 0)
    assert r.p1_pivots > 0 and r.p1_passes >= r.p1_pivots and r.ninf0 > 0
    z = g["highs_z"]
    assert abs(r.z - z) <= 1e-9 * abs(z), (r.z, z)
    assert min(r.gap_price, r.gap_ratio, r.gap_flip) >= 1e-6
    assert min(g["gap_price"], g["gap_ratio"], g["gap_flip"]) >= golden["min_gap"] == 1e-6
    # ninf is monotone non-increasing over every pass, and phase 1 is one prefix of the passes
    h = r.ninf_hist
    assert h[0] == r.ninf0 and all(h[i + 1] <= h[i] for i in range(len(h) - 1))
    assert sum(1 for v in h if v > 0) == r.p1_passes
    # the certificate from the basis and the placements alone
    viol, dviol, zc = ref.certificate(A, b, c, u, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= 1e-9 * abs(z)
    x = r.primal(u)
    assert np.max(np.abs(A @ x - b)) <= 1e-9 * np.max(np.abs(b))


def test_golden_file_is_complete(golden):
    assert sorted(golden["by_shape"]) == [(7, 20, 0), (65, 200, 1), (130, 390, 2), (256, 1024, 3)]
    for g in golden["cases"]:
        assert abs(g["ref_z"] - g["highs_z"]) <= 1e-9 * abs(g["highs_z"])
        assert min(g["gap_price"], g["gap_ratio"], g["gap_flip"]) >= 1e-6
        assert g["p1_pivots"] > 0 and g["ninf0"] > 0
    assert golden["stuck"]["rows_out"] > 0 and golden["stuck"]["free_bad"] > 0


@pytest.mark.parametrize("m,n,seed", [(7, 20, 0), (65, 200, 1)])
def test_feasible_entry_is_the_plain_loop(m, n, seed):
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    want = primal_box_ref.primal_simplex_box(A, b, c, u, trace_cap=1 << 30)
    got = ref.primal_simplex_phase1(A, b, c, u, trace_cap=1 << 30)
    assert got.status == want.status == dual_ref.OPTIMUM
    assert got.trace == want.trace and got.pivots == want.pivots
    assert (got.flips, got.to_upper) == (want.flips, want.to_upper)
    assert (got.p1_passes, got.p1_pivots, got.ninf0) == (0, 0, 0)
    assert got.z == want.z and np.array_equal(got.x_b, want.x_b) and np.array_equal(got.at_upper, want.at_upper)
    assert (got.gap_price, got.gap_ratio, got.gap_flip) == (want.gap_price, want.gap_ratio, want.gap_flip)


def test_tiny_cases(golden):
    # x0 + s = -1, x0 <= 2: below, and the only column raises the violation
    A, b, c, u = ref.tiny_infeasible()
    r = ref.primal_simplex_phase1(A, b, c, u)
    assert r.status == ref.INFEASIBLE and r.pivots == 0 and (r.p1_passes, r.ninf0, r.ninf) == (0, 1, 1)
    # the slack basis x_b = (2, -1): one phase-1 pivot brings row 1 to 0, then phase 2
    A, b, c, u = primal_box_ref.tiny_not_feasible()
    assert primal_box_ref.primal_simplex_box(A, b, c, u).status == primal_box_ref.NOT_PRIMAL_FEASIBLE
    r = ref.primal_simplex_phase1(A, b, c, u)
    g = golden["tiny_not_feasible"]
    assert r.status == dual_ref.OPTIMUM and r.p1_pivots == 1 and r.ninf0 == 1
    assert r.trace[0] == (0, 1)  # x0 enters for row 1's slack
    assert r.z == 2.0 and abs(g["highs_z"] - 2.0) <= 1e-12
    x = r.primal(u)
    assert np.allclose(A @ x, b) and np.all(x >= 0) and np.all(x <= u)
    assert x.tolist() == g["x"]
    # an unbounded LP entered below its bounds: phase 1 first, then UNBOUNDED from phase 2
    A = np.array([[-1.0, 1.0, 1.0]])
    r = ref.primal_simplex_phase1(A, np.array([-1.0]), np.array([1.0, 1.0, 0.0]), np.full(3, np.inf))
    assert r.status == primal_box_ref.UNBOUNDED and r.p1_pivots == 1


def test_contradictory_rows(golden):
    g = golden["infeasible"]
    m, n, seed = g["m"], g["n"], g["seed"]
    A, b, c, u = ref.boxed_general(m, n, seed)
    A2, b2, u2 = ref.contradict(A, b, u)
    r = ref.primal_simplex_phase1(A2, b2, c, u2, trace_cap=0)
    assert r.status == ref.INFEASIBLE and r.pivots == g["ref_pivots"] and r.ninf == g["ninf_end"] > 0
    assert (r.p1_passes, r.p1_pivots, r.ninf0) == (g["p1_passes"], g["p1_pivots"], g["ninf0"])
    h = r.ninf_hist
    assert all(h[i + 1] <= h[i] for i in range(len(h) - 1))
    b3 = b2.copy()
    b3[0], b3[1] = g["feasible_b01"]
    r = ref.primal_simplex_phase1(A2, b3, c, u2, trace_cap=0)
    assert r.status == dual_ref.OPTIMUM and abs(r.z - g["feasible_highs_z"]) <= 1e-9 * abs(g["feasible_highs_z"])


def test_stuck_warm_start_reference(golden):
    """The golden stuck case, re-derived: an optimal basis after cost_variant and
    rhs_variant together is feasible on neither side, and the reference's
    phase 1 from it has the stored counts and HiGHS's optimum."""
    g = golden["stuck"]
    m, n, seed = g["m"], g["n"], g["seed"]
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    first = primal_box_ref.primal_simplex_box(A, b, c, u, trace_cap=0)
    assert first.status == dual_ref.OPTIMUM and first.pivots == g["first_pivots"]
    c2 = primal_box_ref.cost_variant(c, n - m, seed)
    b2 = ref.rhs_variant(b, seed)
    assert primal_box_ref.primal_simplex_box(A, b2, c2, u, basis=first.b_ixs, at_upper=first.at_upper).status \
        == primal_box_ref.NOT_PRIMAL_FEASIBLE
    import dual_box_ref
    assert dual_box_ref.dual_simplex_box(A, b2, c2, u, basis=first.b_ixs, at_upper=first.at_upper).status \
        == dual_box_ref.NOT_DUAL_FEASIBLE
    r = ref.primal_simplex_phase1(A, b2, c2, u, basis=first.b_ixs, at_upper=first.at_upper, trace_cap=0)
    assert r.status == dual_ref.OPTIMUM and r.pivots == g["ref_pivots"]
    assert (r.p1_passes, r.p1_pivots, r.ninf0, r.ninf) == (g["p1_passes"], g["p1_pivots"], g["ninf0"], 0)
    assert (r.flips, r.to_upper) == (g["flips"], g["to_upper"])
    assert min(r.gap_price, r.gap_ratio, r.gap_flip) >= 1e-6
    assert abs(r.z - g["highs_z"]) <= 1e-9 * abs(g["highs_z"])
    viol, dviol, _ = ref.certificate(A, b2, c2, u, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)


def test_header_and_bindings():
    with open(os.path.join(ROOT, "include", "simplex.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+SPX_FLAG_PRIMAL_PHASE1\s+8192\b", h)
    assert re.search(r"#define\s+SPX_ABI_VERSION\s+8\b", h)  # additive: the version stays
    assert re.search(r"int\s+spx_set_primal_phase1\(spx_ctx\*\s*ctx,\s*int32_t\s+on\);", h)
    assert re.search(r"int\s+spx_get_primal_phase1\(spx_ctx\*\s*ctx,\s*int64_t\s+out\[4\]\);", h)
    import simplex_method_gpu_amd as spx
    from simplex_method_gpu_amd import _lib

    assert spx.FLAG_PRIMAL_PHASE1 == 8192 and "FLAG_PRIMAL_PHASE1" in spx.__all__
    assert callable(spx.Context.set_primal_phase1) and callable(spx.Context.primal_phase1)
    # every function the header declares is bound, the names with a digit included
    txt = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = set(re.findall(r"\b(spx_[a-z0-9_]+)\s*\(", txt))
    assert {"spx_set_primal_phase1", "spx_get_primal_phase1", "spx_pbox_vtb_times"} <= declared
    assert declared == set(_lib.SIGNATURES) | set(_lib.SIGNATURES_NUMBERED)
    assert set(_lib.SIGNATURES_NUMBERED) == {"spx_set_primal_phase1", "spx_get_primal_phase1"}
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name


def test_cli_refuses_phase1_without_primal_box():
    solver = os.path.join(ROOT, "solver")
    r = subprocess.run([solver, "--phase1", "--gen", "4", "8", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--phase1" in r.stderr and "--primal-box" in r.stderr
    r = subprocess.run([solver, "--help"], capture_output=True, text=True, timeout=60)
    assert "--phase1" in r.stderr
