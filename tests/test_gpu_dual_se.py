"""GPU: dual steepest-edge pricing of the dual simplex loop
(SPX_DUAL_PRICING_STEEPEST) on the covering LPs of
tests/dual_ref.py.

Golden values (tests/golden/dual_se_optima.json, written by
tests/golden/make_golden_dual_se.py): pivot count, the first 200 (p, q) pairs
and the final basis of the numpy restatement tests/dual_se_ref.py; the optima
are HiGHS's (tests/golden/dual_optima.json).  The smallest relative gap between
the best and the second-best key over those runs is 2.6e-4 for the leaving row
and 3.6e-5 for the ratio test (1024 x 4096; 4.6e-4 at the traced shapes), so
pivot-for-pivot equality does not depend on the fp64 summation order.

Shapes: 7 x 20 (m below one wave), 65 x 200 (L = 128 padding), 130 x 390
(L = 256, m no multiple of 64), 256 x 1024 (several rows per update workgroup,
a multi-workgroup pricing grid), 1024 x 4096 (certificate and pivot count).

Weights are compared with the squared row norms of numpy's inverse of the basis
matrix at 1e-9 relative: the covering LPs' basis matrices compared here have
condition numbers below 2e4 (1.7e4 at 256 x 1024 after 60 pivots), so an
inverse's rows carry relative errors of the order of 2e4 * 2.2e-16 = 4e-12, far
below that; the largest error seen over all the comparisons, the oracle
generator's LPs included, is 9e-14.
"""
import json
import os

import numpy as np
import pytest

import dual_ref
import dual_se_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9


def _cases(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return {(c["m"], c["n"], c["seed"]): c for c in json.load(f)["cases"]}


@pytest.fixture(scope="module")
def se_golden():
    return _cases("dual_se_optima.json")


@pytest.fixture(scope="module")
def highs_z():
    return {k: c["highs_z"] for k, c in _cases("dual_optima.json").items()}


_LPS = {}


def _lp(m, n, seed):
    """(A_cols (n, m), b, c) of the covering LP, built once per shape."""
    if (m, n, seed) not in _LPS:
        A, b, c = dual_ref.covering(m, n, seed)
        _LPS[(m, n, seed)] = (np.ascontiguousarray(A.T), b, c)
    return _LPS[(m, n, seed)]


def _ctx(spx, m, n, seed, **kw):
    A, b, c = _lp(m, n, seed)
    kw.setdefault("dual_pricing", spx.DUAL_PRICING_STEEPEST)
    return spx.Context(A, b, c, window=-1, trace=200, algorithm=spx.ALGO_DUAL, **kw)


def _solve(spx, m, n, seed, **kw):
    with _ctx(spx, m, n, seed, **kw) as ctx:
        r = ctx.solve()
        tp, tq = ctx.trace()
    return r, tp.tolist(), tq.tolist()


def _check_against_golden(spx, g, z, r, tp, tq, trace=True):
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    assert sorted(r.b_ixs.tolist()) == sorted(g["ref_b_ixs"])
    if trace:
        assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
        k = min(g["ref_pivots"], 200)
        assert tp[:k] == g["ref_trace_p"][:k]
        assert tq[:k] == g["ref_trace_q"][:k]
        assert r.b_ixs.tolist() == g["ref_b_ixs"]  # the same pivots: the same basis order


def _cpu_weights(A_cols, b_ixs):
    """Squared row norms of the inverse of the basis matrix, in basis order."""
    B = np.ascontiguousarray(A_cols[np.asarray(b_ixs, dtype=np.int64)].T)
    return dual_se_ref.row_norms2(np.linalg.inv(B))


def _check_weights(ctx, A_cols, what):
    w = ctx.dual_weights()
    ref = _cpu_weights(A_cols, ctx.state()["b_ixs"])
    err = float(np.max(np.abs(w - ref) / ref))
    print(f"{what}: largest relative weight error {err:.2e}")
    assert err <= REL, (what, err)


@pytest.mark.parametrize("m,n,seed", dual_ref.TRACED)
def test_trace_parity(spx, se_golden, highs_z, m, n, seed):
    g = se_golden[(m, n, seed)]
    r, tp, tq = _solve(spx, m, n, seed)
    print(f"{m}x{n}: z={r.z:.13g} pivots={r.pivots} (golden {g['ref_pivots']}, Dantzig {g['dantzig_pivots']})")
    _check_against_golden(spx, g, highs_z[(m, n, seed)], r, tp, tq)
    assert np.min(r.x_b) >= -1e-9


@pytest.mark.parametrize("m,n,seed,first,second", [(130, 390, 2, 7, 13), (256, 1024, 3, 60, 0)],
                         ids=["130x390_after_7+13", "256x1024_after_60"])
def test_weights_are_row_norms(spx, se_golden, m, n, seed, first, second):
    """The weights the passes keep (two spx_iterate calls: they survive the
    call boundary), then recomputed after spx_reinvert and spx_set_basis."""
    g = se_golden[(m, n, seed)]
    A = _lp(m, n, seed)[0]
    with _ctx(spx, m, n, seed) as ctx:
        ctx.iterate(first)
        if second:
            ctx.iterate(second)
        s = ctx.state()
        k = first + second
        assert s["pivots"] == k
        tp, tq = ctx.trace()
        assert tp.tolist() == g["ref_trace_p"][:k] and tq.tolist() == g["ref_trace_q"][:k]
        _check_weights(ctx, A, f"{m}x{n} after {k} pivots")
        ctx.reinvert()
        _check_weights(ctx, A, "after reinvert")
        ctx.set_basis(ctx.state()["b_ixs"])
        _check_weights(ctx, A, "after set_basis")


@pytest.mark.parametrize("kw,trace", [({"global_y": True}, True), ({"price_grid": 3}, True),
                                      ({"refactor_every": 50}, False)],
                         ids=["global_y", "price_grid3", "refactor50"])
def test_variants_256(spx, se_golden, highs_z, kw, trace):
    m, n, seed = 256, 1024, 3
    r, tp, tq = _solve(spx, m, n, seed, **kw)
    print(f"{kw}: z={r.z:.13g} pivots={r.pivots}")
    _check_against_golden(spx, se_golden[(m, n, seed)], highs_z[(m, n, seed)], r, tp, tq, trace=trace)


def test_certificate_1024(spx, se_golden, highs_z):
    """C2's shape, refactor_every=500: status, z against HiGHS, the certificate
    recomputed on the CPU from the returned basis (as
    tests/test_gpu_dual.py::test_certificate_1024), and at most half the
    Dantzig rule's pivots."""
    m, n, seed = dual_ref.SHAPES[4]
    A, b, c = _lp(m, n, seed)
    g = se_golden[(m, n, seed)]
    z = highs_z[(m, n, seed)]
    with spx.Context(A, b, c, window=-1, algorithm=spx.ALGO_DUAL, refactor_every=500,
                     dual_pricing=spx.DUAL_PRICING_STEEPEST) as ctx:
        r = ctx.solve()
    print(f"{m}x{n}: z={r.z:.13g} (HiGHS {z:.13g}) pivots={r.pivots} (reference {g['ref_pivots']}, "
          f"Dantzig {g['dantzig_pivots']})")
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    assert g["dantzig_pivots"] == 4289
    assert 2 * r.pivots <= g["dantzig_pivots"], r.pivots
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


def test_resolve_after_rhs_change(spx, oracle):
    """tests/test_gpu_dual.py::test_resolve_after_rhs_change's recipe, repaired
    by the steepest-edge dual loop: a context created for the primal loop,
    solved by the explicit pass, set_rhs, then set_algorithm(ALGO_DUAL) +
    set_dual_pricing(STEEPEST).  The weights right after the switch come from
    k_dual_norms."""
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
        assert np.min(ctx.state()["x_b"]) < -1e-9  # the old basis is primal infeasible for b2
        ctx.set_algorithm(spx.ALGO_DUAL)
        ctx.set_dual_pricing(spx.DUAL_PRICING_STEEPEST)
        assert ctx.config()["dual_pricing"] == spx.DUAL_PRICING_STEEPEST
        _check_weights(ctx, A, "after the switch")
        r = ctx.solve()
        dual_pivots = r.pivots - r0.pivots
        print(f"fresh primal solve: {ref.pivots} pivots; steepest dual re-solve: {dual_pivots} pivots; "
              f"z={r.z:.13g} vs {ref.z:.13g}")
        assert r.status == spx.SolveStatus.OptimumFound
        assert dual_pivots > 0
        assert abs(r.z - ref.z) <= REL * abs(ref.z), (r.z, ref.z)
        assert sorted(r.b_ixs.tolist()) == sorted(ref.b_ixs.tolist())
        _check_weights(ctx, A, "at the optimum")


def test_weights_with_a_pending_primal_update(spx, oracle):
    """k_dual_norms applies the rank-1 update the primal explicit pass leaves
    pending: 30 primal pivots, the switch, the weights (no dual pass runs: the
    basis need not be dual feasible for that)."""
    m, n = 130, 390
    A, b, c = oracle.generate(m, n, 0)
    with spx.Context(A, b, c, window=-1, dual_pricing=spx.DUAL_PRICING_STEEPEST) as ctx:
        st, piv = ctx.iterate(30)
        assert st == spx.SolveStatus.MaxIter and piv == 30
        with pytest.raises(spx.SimplexError) as ei:
            ctx.dual_weights()  # the primal loop keeps none
        assert ei.value.code == -5
        ctx.set_algorithm(spx.ALGO_DUAL)
        _check_weights(ctx, A, "30 primal pivots, then the switch")


def test_rule_switched_mid_solve(spx, highs_z):
    """20 Dantzig dual pivots at 130 x 390, then steepest edge to the optimum:
    the pivots of the reference started from that basis (36; its smallest key
    gap on this path is 1.3e-2)."""
    m, n, seed = 130, 390, 2
    A, b, c = _lp(m, n, seed)
    with _ctx(spx, m, n, seed, dual_pricing=spx.DUAL_PRICING_DANTZIG) as ctx:
        st, piv = ctx.iterate(20)
        assert st == spx.SolveStatus.MaxIter and piv == 20
        with pytest.raises(spx.SimplexError) as ei:
            ctx.dual_weights()
        assert ei.value.code == -5  # SPX_ERR_STATE under Dantzig
        mid = ctx.state()["b_ixs"]
        ctx.set_dual_pricing(spx.DUAL_PRICING_STEEPEST)
        _check_weights(ctx, A, "after 20 Dantzig pivots")
        r = ctx.solve()
        tp, tq = ctx.trace()
    ref = dual_se_ref.dual_simplex_se(*dual_ref.covering(m, n, seed), basis=mid)
    print(f"20 Dantzig + {r.pivots - 20} steepest pivots (reference {ref.pivots}); gaps {ref.gap_row:.1e} "
          f"{ref.gap_ratio:.1e}")
    z = highs_z[(m, n, seed)]
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    assert r.pivots == 20 + ref.pivots
    assert list(zip(tp[20:].tolist(), tq[20:].tolist())) == ref.trace
    assert r.b_ixs.tolist() == ref.b_ixs.tolist()


def test_infeasible(spx):
    A, b, c = dual_ref.tiny_infeasible()
    with spx.Context(np.ascontiguousarray(A.T), b, c, window=-1, algorithm=spx.ALGO_DUAL,
                     dual_pricing=spx.DUAL_PRICING_STEEPEST) as ctx:
        r = ctx.solve()
    assert r.status == spx.SolveStatus.Infeasible and r.pivots == 1, r


def test_errors(spx):
    with _ctx(spx, 7, 20, 0, dual_pricing=spx.DUAL_PRICING_DANTZIG) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.dual_weights()
        assert ei.value.code == -5 and "Dantzig" in str(ei.value)
        for bad in (-1, 2):
            with pytest.raises(spx.SimplexError) as ei:
                ctx.set_dual_pricing(bad)
            assert ei.value.code == -1
        assert ctx.config()["dual_pricing"] == spx.DUAL_PRICING_DANTZIG
        ctx.set_dual_pricing(spx.DUAL_PRICING_STEEPEST)
        assert ctx.dual_weights().tolist() == [1.0] * 7  # the slack basis: B^-1 = I


def test_cli_dual_pricing(se_golden, highs_z, tmp_path):
    """./solver --dual --dual-pricing steepest FILE."""
    import subprocess

    m, n, seed = 65, 200, 1
    A, b, c = dual_ref.covering(m, n, seed)
    p = str(tmp_path / "cover.txt")
    with open(p, "w") as f:
        f.write(f"{m} {n}\n")
        for row in A:
            f.write(" ".join("%.17g" % v for v in row) + "\n")
        f.write(" ".join("%.17g" % v for v in b) + "\n")
        f.write(" ".join("%.17g" % v for v in c) + "\n")
    r = subprocess.run([os.path.join(ROOT, "solver"), "--dual", "--dual-pricing", "steepest", "--json",
                        "--no-iter-lines", p], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.splitlines()[-1])
    z = highs_z[(m, n, seed)]
    assert js["status"] == 1 and js["pivots"] == se_golden[(m, n, seed)]["ref_pivots"]
    assert abs(js["z"] - z) <= REL * abs(z)
