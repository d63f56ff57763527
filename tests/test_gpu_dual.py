"""GPU: the dual simplex loop (SPX_ALGO_DUAL) on covering LPs
max -cost.x, -G x + s = -h (b < 0: the slack basis is dual feasible and
primal infeasible).

Golden values (tests/golden/dual_optima.json, written by
tests/golden/make_golden_dual.py): the optimum of scipy HiGHS for every shape
and, for m <= 256, the pivot count, the first 200 (p, q) pairs and the final
basis of the numpy restatement tests/dual_ref.py.  The smallest relative gap
between the best and the second-best ratio key over those runs is 6.5e-4
(256 x 1024), so pivot-for-pivot equality does not depend on the fp64
summation order.  z is compared at 1e-9 relative, the tolerance against the
oracle elsewhere in the suite.

Shapes: 7 x 20 (m below one wave), 65 x 200 and 130 x 390 (m no multiple of 64
or 128: the L padding), 256 x 1024 (several rows per update workgroup, a
multi-workgroup pricing grid), 1024 x 4096 (C2's shape, certificate only).
"""
import json
import os

import numpy as np
import pytest

import dual_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9


@pytest.fixture(scope="module")
def dual_golden():
    with open(os.path.join(ROOT, "tests", "golden", "dual_optima.json")) as f:
        return {(c["m"], c["n"], c["seed"]): c for c in json.load(f)["cases"]}


_LPS = {}


def _lp(m, n, seed):
    """(A_cols (n, m), b, c) of the covering LP, built once per shape."""
    if (m, n, seed) not in _LPS:
        A, b, c = dual_ref.covering(m, n, seed)
        _LPS[(m, n, seed)] = (np.ascontiguousarray(A.T), b, c)
    return _LPS[(m, n, seed)]


def _solve_dual(spx, m, n, seed, **kw):
    A, b, c = _lp(m, n, seed)
    with spx.Context(A, b, c, window=-1, trace=200, algorithm=spx.ALGO_DUAL, **kw) as ctx:
        r = ctx.solve()
        tp, tq = ctx.trace()
    return r, tp.tolist(), tq.tolist()


def _check_against_golden(spx, g, r, tp, tq, trace=True):
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - g["highs_z"]) <= REL * abs(g["highs_z"]), (r.z, g["highs_z"])
    assert sorted(r.b_ixs.tolist()) == sorted(g["ref_b_ixs"])
    if trace:
        assert r.b_ixs.tolist() == g["ref_b_ixs"]  # the same pivots: the same basis order
        k = min(g["ref_pivots"], 200)
        assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
        assert tp[:k] == g["ref_trace_p"][:k]
        assert tq[:k] == g["ref_trace_q"][:k]


@pytest.mark.parametrize("m,n,seed", dual_ref.TRACED)
def test_trace_parity(spx, dual_golden, m, n, seed):
    r, tp, tq = _solve_dual(spx, m, n, seed)
    print(f"{m}x{n}: z={r.z:.13g} pivots={r.pivots} (golden {dual_golden[(m, n, seed)]['ref_pivots']})")
    _check_against_golden(spx, dual_golden[(m, n, seed)], r, tp, tq)
    assert np.min(r.x_b) >= -1e-9


@pytest.mark.parametrize("kw,trace", [({"global_y": True}, True), ({"price_grid": 3}, True),
                                      ({"refactor_every": 50}, False)],
                         ids=["global_y", "price_grid3", "refactor50"])
def test_variants_256(spx, dual_golden, kw, trace):
    m, n, seed = 256, 1024, 3
    r, tp, tq = _solve_dual(spx, m, n, seed, **kw)
    print(f"{kw}: z={r.z:.13g} pivots={r.pivots}")
    _check_against_golden(spx, dual_golden[(m, n, seed)], r, tp, tq, trace=trace)


def test_certificate_1024(spx, dual_golden):
    """C2's shape, refactor_every=500: status, z against HiGHS, and the
    certificate recomputed on the CPU from the returned basis (as
    tests/test_gpu_certificate.py: the duals solve B^T y = c_B on the CPU)."""
    m, n, seed = dual_ref.SHAPES[4]
    A, b, c = _lp(m, n, seed)
    with spx.Context(A, b, c, window=-1, algorithm=spx.ALGO_DUAL, refactor_every=500) as ctx:
        r = ctx.solve()
    g = dual_golden[(m, n, seed)]
    print(f"{m}x{n}: z={r.z:.13g} (HiGHS {g['highs_z']:.13g}) pivots={r.pivots}")
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - g["highs_z"]) <= REL * abs(g["highs_z"]), (r.z, g["highs_z"])
    bix = np.asarray(r.b_ixs, dtype=np.int64)
    assert len(set(bix.tolist())) == m
    B = np.ascontiguousarray(A[bix].T)
    res = B @ r.x_b - b
    assert np.max(np.abs(res)) <= 1e-9 * np.max(np.abs(b)), np.max(np.abs(res))
    assert np.min(r.x_b) >= -1e-9, np.min(r.x_b)
    y = np.linalg.solve(B.T, c[bix])
    e = A @ y - c
    print(f"primal residual {np.max(np.abs(res)):.2e}, min x_b {np.min(r.x_b):.2e}, min reduced cost {np.min(e):.2e}")
    assert np.min(e) >= -1e-9, np.min(e)


def test_infeasible(spx):
    A, b, c = dual_ref.tiny_infeasible()
    with spx.Context(np.ascontiguousarray(A.T), b, c, window=-1, algorithm=spx.ALGO_DUAL) as ctx:
        r = ctx.solve()
    assert r.status == spx.SolveStatus.Infeasible and r.pivots == 1, r


def test_not_dual_feasible_then_primal(spx, oracle):
    """Some c_j > 0: the slack basis is not dual feasible, the dual loop
    refuses it (SPX_ERR_STATE) and the primal loop solves the same context."""
    A, b, c = oracle.generate(64, 256, 0)
    ref = oracle.solve(A, b, c, eps=1e-7)
    with spx.Context(A, b, c, window=-1, algorithm=spx.ALGO_DUAL) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.iterate(1)
        assert ei.value.code == -5 and "not dual feasible" in str(ei.value)
        ctx.set_algorithm(spx.ALGO_PRIMAL)
        r = ctx.solve()
    assert r.status == spx.SolveStatus.OptimumFound and r.pivots == ref.pivots
    assert abs(r.z - ref.z) <= REL * abs(ref.z)


def test_resolve_after_rhs_change(spx, oracle):
    """Primal solve, 16 entries of b halved (b2 >= 0 still, so a fresh primal
    solve of (A, b2, c) is the independent reference), then set_rhs + the dual
    loop from the old optimal basis.  With these seeds x_b = B^-1 b2 has 16
    negative entries (checked on the CPU), so the dual loop has to pivot."""
    m, n = 256, 1024
    A, b, c = oracle.generate(m, n, 0)
    idx = np.random.default_rng(0).choice(m, 16, replace=False)
    b2 = b.copy()
    b2[idx] *= 0.5
    with spx.Context(A, b2, c, window=-1) as fresh:
        ref = fresh.solve()
    assert ref.status == spx.SolveStatus.OptimumFound
    with spx.Context(A, b, c, window=-1) as ctx:
        r0 = ctx.solve()
        assert r0.status == spx.SolveStatus.OptimumFound
        ctx.set_rhs(b2)
        s = ctx.state()
        assert s["status"] == spx.SolveStatus.MaxIter and s["pivots"] == r0.pivots
        assert np.min(s["x_b"]) < -1e-9  # the old basis is primal infeasible for b2
        ctx.set_algorithm(spx.ALGO_DUAL)
        r = ctx.solve()
        dual_pivots = r.pivots - r0.pivots
        print(f"fresh primal solve: {ref.pivots} pivots; dual re-solve: {dual_pivots} pivots "
              f"(after {r0.pivots}); z={r.z:.13g} vs {ref.z:.13g}")
        assert r.status == spx.SolveStatus.OptimumFound
        assert dual_pivots > 0
        assert abs(r.z - ref.z) <= REL * abs(ref.z), (r.z, ref.z)
        assert sorted(r.b_ixs.tolist()) == sorted(ref.b_ixs.tolist())
        # readbacks after dual passes, and the primal loop agrees it is optimal
        assert abs(ctx.objective() - r.z) <= REL * abs(r.z)
        assert np.min(ctx.reduced_costs()) >= -1e-7 - 1e-9
        ctx.set_algorithm(spx.ALGO_PRIMAL)
        st, piv = ctx.iterate(1)
        assert st == spx.SolveStatus.OptimumFound and piv == r.pivots


def test_state_consistent_after_dual_passes(spx):
    """Mid-solve readback after dual passes: B^-1 (with its pending rank-1
    update), x_b and y against the basis on the CPU; then spx_reinvert and
    spx_set_basis keep the solve going to the same optimum."""
    m, n, seed = 130, 390, 2
    A, b, c = _lp(m, n, seed)
    with spx.Context(A, b, c, window=-1, algorithm=spx.ALGO_DUAL) as ctx:
        st, piv = ctx.iterate(40)
        assert st == spx.SolveStatus.MaxIter and piv == 40
        s = ctx.state(binv=True)
        bix = np.asarray(s["b_ixs"], dtype=np.int64)
        B = np.ascontiguousarray(A[bix].T)
        assert np.max(np.abs(s["binv"] @ B - np.eye(m))) <= 1e-9
        assert np.max(np.abs(B @ s["x_b"] - b)) <= 1e-9 * np.max(np.abs(b))
        assert np.max(np.abs(B.T @ s["y"] - c[bix])) <= 1e-9
        ctx.reinvert()
        ctx.iterate(10)
        basis = ctx.state()["b_ixs"]
        ctx.set_basis(basis)
        r = ctx.solve()
    z_ref = dual_ref.dual_simplex(*dual_ref.covering(m, n, seed)).z
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - z_ref) <= REL * abs(z_ref)


def _write_lp(path, A, b, c):
    """The reference's LP text format: m n, A row-major, b, c (%.17g: exact)."""
    m, n = A.shape
    with open(path, "w") as f:
        f.write(f"{m} {n}\n")
        for row in A:
            f.write(" ".join("%.17g" % v for v in row) + "\n")
        f.write(" ".join("%.17g" % v for v in b) + "\n")
        f.write(" ".join("%.17g" % v for v in c) + "\n")


def test_cli_dual(dual_golden, tmp_path):
    """./solver --dual FILE: the primal CLI's output format; "Problem
    infeasible." for status 4; a slack basis that is not dual feasible is an
    error exit with a message."""
    import subprocess

    solver = os.path.join(ROOT, "solver")

    def run(*args):
        return subprocess.run([solver, *args], capture_output=True, text=True, timeout=120)

    m, n, seed = 7, 20, 0
    p = str(tmp_path / "cover.txt")
    _write_lp(p, *dual_ref.covering(m, n, seed))
    r = run("--dual", "--json", p)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    g = dual_golden[(m, n, seed)]
    assert lines[:g["ref_pivots"] + 1] == [f"# Iteration {i}" for i in range(1, g["ref_pivots"] + 2)]
    assert lines[g["ref_pivots"] + 1].startswith("Optimum found: ")
    js = json.loads(lines[-1])
    assert js["status"] == 1 and js["pivots"] == g["ref_pivots"]
    assert abs(js["z"] - g["highs_z"]) <= REL * abs(g["highs_z"])
    q = str(tmp_path / "infeasible.txt")
    _write_lp(q, *dual_ref.tiny_infeasible())
    r = run("--dual", "--no-iter-lines", q)
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "Problem infeasible.", (r.stdout, r.stderr)
    r = run("--dual", os.path.join(ROOT, "tests", "golden", "sample.txt"))  # c = (3, 2, 0, 0) > 0
    assert r.returncode != 0 and "not dual feasible" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("kw", [{"window": 64}, {"nranks": 2}, {"tableau": True}],
                         ids=["window64", "nranks2", "tableau"])
def test_out_of_scope_raises_at_construction(spx, kw):
    A, b, c = _lp(65, 200, 1)
    with pytest.raises(spx.SimplexError) as ei:
        spx.Context(A, b, c, algorithm=spx.ALGO_DUAL, **kw)
    assert ei.value.code == -1 and "dual simplex loop does not run" in str(ei.value)


def test_out_of_scope_calls_return_state_error(spx):
    A, b, c = _lp(65, 200, 1)
    with spx.Context(A, b, c, algorithm=spx.ALGO_DUAL) as ctx:  # window 0 resolves to the explicit B^-1
        assert ctx.config()["window"] == 0
        with pytest.raises(spx.SimplexError) as ei:
            ctx.price()
        assert ei.value.code == -5 and "primal loop only" in str(ei.value)
    with spx.Context(A, b, c, window=8) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_algorithm(spx.ALGO_DUAL)
        assert ei.value.code == -5 and "eta window" in str(ei.value)
