"""CPU: general bounds l <= x <= u for the bounded loops (spx_set_bounds_lu;
DESIGN.md §7j).  The numpy restatement tests/primal_lu_ref.py against its golden
file (tests/golden/primal_lu_optima.json, written by
tests/golden/make_golden_primal_lu.py: HiGHS optima with bounds=list(zip(l, u)),
traces, final bases, counters) and against the certificate on the unshifted
problem; with l = 0 and no free column it is primal_phase1_ref's loop pass for
pass; the infeasible and the unbounded case; the additions to the C-ABI, the
Python package and the CLI that need no device."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dual_ref
import primal_lu_ref as ref
import primal_phase1_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "primal_lu_optima.json")) as f:
        g = json.load(f)
    g["by_shape"] = {(c["m"], c["n"], c["seed"]): c for c in g["cases"]}
    return g


def _same_as_golden(r, g):
    assert r.status == dual_ref.OPTIMUM
    assert r.pivots == g["ref_pivots"]
    assert [p for p, _ in r.trace] == g["ref_trace_p"]
    assert [q for _, q in r.trace] == g["ref_trace_q"]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(r.at_upper).tolist() == g["ref_at_upper"]
    assert (r.flips, r.to_upper) == (g["flips"], g["to_upper"])
    assert (r.p1_passes, r.p1_pivots, r.ninf0, r.ninf) == (g["p1_passes"], g["p1_pivots"], g["ninf0"], 0)
    z = g["highs_z"]
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    assert min(r.gap_price, r.gap_ratio, r.gap_flip) >= 1e-6


@pytest.mark.parametrize("m,n,seed", [(7, 20, 0), (65, 200, 1), (130, 390, 2), (256, 1024, 3)])
def test_ref_reproduces_golden(golden, m, n, seed):
    g = golden["by_shape"][(m, n, seed)]
    A, b, c, l, u = ref.general_lu(m, n, seed)
    ns = n - m
    free = np.isneginf(l)
    # what the generator promises: about a fifth free with costs of either sign, about a third with a finite lower
    # bound of either sign, every free column without bounds at all
    assert abs(int(free[:ns].sum()) - ns / 5) <= 1 and np.any(c[free] > 0) and np.any(c[free] < 0)
    low = np.isfinite(l[:ns]) & (l[:ns] != 0)
    assert ns / 4 <= int(low.sum()) <= ns / 2 and np.any(l[:ns][low] < 0) and np.any(l[:ns][low] > 0)
    assert np.all(np.isposinf(u[free])) and not np.any(free[ns:]) and np.any(l[ns:] != 0)
    r = ref.primal_simplex_lu(A, b, c, l, u, trace_cap=200)
    print(f"{m}x{n}: pivots={r.pivots} flips={r.flips} to_upper={r.to_upper} phase 1 {r.p1_passes}/{r.p1_pivots} "
          f"ninf0={r.ninf0} z={r.z:.13g} gaps {r.gap_price:.2e} {r.gap_ratio:.2e} {r.gap_flip:.2e}")
    _same_as_golden(r, g)
    assert g["free_entered"] > 0 and g["free_basic"] == int(np.count_nonzero(free[r.b_ixs]))
    assert min(g["gap_price"], g["gap_ratio"], g["gap_flip"]) >= golden["min_gap"] == 1e-6
    # the caller's variables: inside [l, u], a non-basic column exactly at its bound, z = c.x, A x = b
    x = r.primal_lu(l, u)
    assert np.all(x >= l - 1e-9) and np.all(x <= u + 1e-9)
    nb = np.ones(n, dtype=bool)
    nb[r.b_ixs] = False
    want = np.where(r.at_upper, u, np.where(free, 0.0, l))
    assert np.array_equal(x[nb], want[nb])
    assert abs(float(c @ x) - r.z) <= REL * abs(r.z)
    assert np.max(np.abs(A @ x - b)) <= 1e-9 * max(1.0, np.max(np.abs(b)))
    # the certificate from the basis and the placements alone, on the unshifted problem
    viol, dviol, zc = ref.certificate_lu(A, b, c, l, u, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - g["highs_z"]) <= REL * abs(g["highs_z"])


def test_shift_case_reproduces_golden(golden):
    g = golden["shift"]
    m, n, seed = g["m"], g["n"], g["seed"]
    A, b, c, l, u = ref.shift_lp(m, n, seed)
    assert not np.any(np.isneginf(l)) and np.any(l == u) and np.any(l < 0) and np.any(l > 0) and np.all(np.isfinite(u))
    r = ref.primal_simplex_lu(A, b, c, l, u, trace_cap=200)
    _same_as_golden(r, g)
    viol, dviol, _ = ref.certificate_lu(A, b, c, l, u, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    # the shifted problem by hand: primal_simplex_phase1 on (A, b - A l, c, u - l) walks the same pivots
    s = primal_phase1_ref.primal_simplex_phase1(A, b - A @ l, c, u - l, trace_cap=200)
    assert s.trace == r.trace and s.pivots == r.pivots and s.b_ixs.tolist() == r.b_ixs.tolist()
    assert abs((s.z + float(c @ l)) - r.z) <= REL * abs(r.z)


@pytest.mark.parametrize("m,n,seed", [(7, 20, 0), (65, 200, 1)])
def test_zero_lower_is_phase1_ref(m, n, seed):
    """l = 0 and no free column: primal_simplex_phase1's pivots, counters and bits."""
    A, b, c, u = primal_phase1_ref.boxed_general(m, n, seed)
    want = primal_phase1_ref.primal_simplex_phase1(A, b, c, u, trace_cap=1 << 30)
    got = ref.primal_simplex_lu(A, b, c, np.zeros(n), u, trace_cap=1 << 30)
    assert got.status == want.status == dual_ref.OPTIMUM
    assert got.trace == want.trace and got.pivots == want.pivots
    assert (got.flips, got.to_upper, got.p1_passes, got.p1_pivots, got.ninf0) == \
        (want.flips, want.to_upper, want.p1_passes, want.p1_pivots, want.ninf0)
    assert np.array_equal(got.at_upper, want.at_upper) and got.ninf_hist == want.ninf_hist
    assert got.z == want.z and np.array_equal(got.x_shifted, want.x_b) and np.array_equal(got.Binv, want.Binv)


def test_infeasible_and_unbounded(golden):
    g = golden["infeasible"]
    m, n, seed = g["m"], g["n"], g["seed"]
    A, b, c, l, u = ref.general_lu(m, n, seed)
    A2, b2, u2 = primal_phase1_ref.contradict(A, b, u)
    l2 = l.copy()
    l2[n - m], l2[n - m + 1] = 0.0, 0.0
    r = ref.primal_simplex_lu(A2, b2, c, l2, u2, trace_cap=0)
    assert r.status == ref.INFEASIBLE and r.pivots == g["ref_pivots"] and r.ninf == g["ninf_end"] > 0
    assert (r.p1_passes, r.p1_pivots, r.ninf0) == (g["p1_passes"], g["p1_pivots"], g["ninf0"])
    # max -x0 with x0 free: it enters downwards (d > 0: sigma = -1) and no row blocks
    A, b, c, l, u = ref.tiny_unbounded_free()
    r = ref.primal_simplex_lu(A, b, c, l, u)
    assert r.status == ref.UNBOUNDED and r.pivots == 0 and r.flips == 0 and golden["unbounded"]["highs_status"] == 3
    # ... and bounded from below it stops at the bound: x0 = -3, z = 3
    r = ref.primal_simplex_lu(A, b, c, np.array([-3.0, 0.0]), u)
    assert r.status == dual_ref.OPTIMUM and r.z == 3.0 and r.primal_lu(np.array([-3.0, 0.0]), u).tolist() == [-3.0, 4.0]


def test_free_basic_row_never_blocks():
    """max x1 with x0 free basic in row 0 (x0 + x1 + s0 = 1) and x1 + s1 = 2: row
    0 has alpha > 0 and x0 would reach 0 at t = 1, but it is free, so row 1
    blocks at t = 2 and x0 ends at -1."""
    A = np.array([[1.0, 1.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0]])
    b = np.array([1.0, 2.0])
    c = np.array([0.0, 1.0, 0.0, 0.0])
    l = np.array([-np.inf, 0.0, 0.0, 0.0])
    u = np.full(4, np.inf)
    r = ref.primal_simplex_lu(A, b, c, l, u, basis=[0, 3])
    assert r.status == dual_ref.OPTIMUM and r.trace == [(1, 1)] and r.z == 2.0
    assert r.primal_lu(l, u).tolist() == [-1.0, 2.0, 0.0, 0.0]


def test_header_and_bindings():
    with open(os.path.join(ROOT, "include", "simplex.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+SPX_ABI_VERSION\s+8\b", h)  # additive: the version stays
    assert re.search(r"int\s+spx_set_bounds_lu\(spx_ctx\*\s*ctx,\s*const\s+double\*\s*lb[^,]*,\s*const\s+double\*\s*ub[^)]*\);", h)
    assert re.search(r"int\s+spx_get_bounds_lu\(spx_ctx\*\s*ctx,\s*double\*\s*lb[^,]*,\s*double\*\s*ub[^)]*\);", h)
    assert re.search(r"int\s+spx_set_bounds\(spx_ctx\*\s*ctx,\s*const\s+double\*\s*ub", h)  # unchanged
    assert "no non-zero or free lower bounds" not in re.sub(r"\s+\*\s+", " ", h)
    import simplex_method_gpu_amd as spx
    from simplex_method_gpu_amd import _lib

    assert callable(spx.Context.set_bounds_lu) and callable(spx.Context.bounds_lu)
    import inspect
    assert "lower" in inspect.signature(spx.Context.__init__).parameters
    txt = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = set(re.findall(r"\b(spx_[a-z0-9_]+)\s*\(", txt))
    assert {"spx_set_bounds_lu", "spx_get_bounds_lu"} <= declared
    assert declared == set(_lib.SIGNATURES) | set(_lib.SIGNATURES_NUMBERED)
    assert {"spx_set_bounds_lu", "spx_get_bounds_lu"} <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.spx_abi_version() == 8
    for name in ("spx_set_bounds_lu", "spx_get_bounds_lu"):
        assert hasattr(lib, name), name


def test_cli_refuses_lower_without_a_bounded_loop(tmp_path):
    solver = os.path.join(ROOT, "solver")
    lo = str(tmp_path / "lower.txt")
    with open(lo, "w") as f:
        f.write("\n".join(["-1"] * 8) + "\n")
    r = subprocess.run([solver, "--lower", lo, "--gen", "4", "8", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--lower" in r.stderr and "--primal-box" in r.stderr and "--dual" in r.stderr
    r = subprocess.run([solver, "--phase1", "--lower", lo, "--gen", "4", "8", "0"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "--phase1" in r.stderr  # the older refusal comes first, as it did
    r = subprocess.run([solver, "--help"], capture_output=True, text=True, timeout=60)
    assert "--lower" in r.stderr
