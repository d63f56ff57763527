"""GPU: boxed variables 0 <= x <= u in the dual simplex loop (spx_set_bounds;
DESIGN.md §7d) on the covering LPs of tests/dual_ref.py with the bounds of
tests/dual_box_ref.py boxed(m, n, seed, flipc).

Golden values (tests/golden/dual_box_optima.json, written by
tests/golden/make_golden_dual_box.py): pivot count, the first 200 (p, q) pairs,
the final basis and the final at-upper set of the numpy restatement
tests/dual_box_ref.py, and HiGHS's optimum of the bounded LP.  The smallest
relative gap between the best and the second-best key over those runs is 1.0e-5
at the traced shapes (the generator refuses a case below 1e-6), so
pivot-for-pivot equality does not depend on the fp64 summation order.

Shapes: 7 x 20 (m below one wave), 65 x 200 (L = 128, heavy padding), 130 x 390
(L = 256, m no multiple of 64), 256 x 1024 (multi-chunk columns, several rows
per update workgroup, a multi-workgroup pricing grid), 1024 x 4096 (optimum and
certificate).  flipc = 1 gives bounded structurals a positive c_j: dual feasible
only at their upper bound, so the entry normalisation places them there.

Bound re-solve: loosening a bound is either invisible to the dual method (the
column is basic or at lower: the basis stays optimal) or takes away the only
side on which a column at upper is dual feasible, which spx_set_bounds refuses by
name.  "Every 16th finite bound to +inf" hits 7 columns of the second kind at
the tightened optimum (at least one for each of the 16 offsets), so that step is
tested both ways: the refusal naming the first such column, and the re-solve
with those 7 bounds kept (the golden file's `loose_kept`).
"""
import json
import os
import subprocess

import numpy as np
import pytest

import dual_box_ref as ref
import dual_ref
import dual_se_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9
RULES = [ref.DANTZIG, ref.STEEPEST]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "dual_box_optima.json")) as f:
        g = json.load(f)
    return {(c["m"], c["n"], c["seed"], c["flipc"], c["rule"]): c for c in g["cases"]}, g["resolve"]


_LPS = {}


def _lp(m, n, seed, flipc):
    """(A_cols (n, m), b, c, u, A (m, n)) of the boxed covering LP, built once."""
    k = (m, n, seed, int(flipc))
    if k not in _LPS:
        A, b, c, u = ref.boxed(m, n, seed, bool(flipc))
        _LPS[k] = (np.ascontiguousarray(A.T), b, c, u, A)
    return _LPS[k]


def _rule(spx, rule):
    return spx.DUAL_PRICING_STEEPEST if rule == ref.STEEPEST else spx.DUAL_PRICING_DANTZIG


def _ctx(spx, m, n, seed, flipc, rule, upper="lp", **kw):
    At, b, c, u, _ = _lp(m, n, seed, flipc)
    kw.setdefault("trace", 200)
    return spx.Context(At, b, c, window=-1, algorithm=spx.ALGO_DUAL, dual_pricing=_rule(spx, rule),
                       upper=u if isinstance(upper, str) else upper, **kw)


def _check_primal(x, up, A, b, u):
    res = float(np.max(np.abs(A @ x - b)))
    assert res <= 1e-9 * np.max(np.abs(b)), res
    assert np.min(x) >= -1e-9 and np.max(x - u) <= 1e-9, (np.min(x), np.max(x - u))
    assert np.array_equal(x[up], u[up])  # exactly the bound
    return res


def _check_against_golden(spx, g, r, tp, tq, x, up, lp, trace=True):
    _, b, c, u, A = lp
    z = g["highs_z"]
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    assert sorted(r.b_ixs.tolist()) == sorted(g["ref_b_ixs"])
    assert np.flatnonzero(up).tolist() == g["ref_at_upper"]
    _check_primal(x, up, A, b, u)
    assert abs(float(c @ x) - z) <= REL * abs(z)
    if trace:
        assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
        k = min(g["ref_pivots"], 200)
        assert tp[:k] == g["ref_trace_p"][:k]
        assert tq[:k] == g["ref_trace_q"][:k]
        assert r.b_ixs.tolist() == g["ref_b_ixs"]  # the same pivots: the same basis order


def _solve(spx, m, n, seed, flipc, rule, **kw):
    with _ctx(spx, m, n, seed, flipc, rule, **kw) as ctx:
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        assert np.array_equal(ctx.bounds(), _lp(m, n, seed, flipc)[3])
    return r, tp.tolist(), tq.tolist(), x, up


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("flipc", [0, 1])
@pytest.mark.parametrize("m,n,seed", dual_ref.TRACED)
def test_trace_parity(spx, golden, m, n, seed, flipc, rule):
    g = golden[0][(m, n, seed, flipc, rule)]
    r, tp, tq, x, up = _solve(spx, m, n, seed, flipc, rule)
    print(f"{m}x{n} flipc={flipc} {rule}: z={r.z:.13g} pivots={r.pivots} (golden {g['ref_pivots']}, "
          f"{g['to_upper']} rows left to upper, {len(g['ref_at_upper'])} at upper, {g['placed']} placed at entry)")
    _check_against_golden(spx, g, r, tp, tq, x, up, _lp(m, n, seed, flipc))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("flipc", [0, 1])
@pytest.mark.parametrize("kw", [{"global_y": True}, {"price_grid": 3}, {"refactor_every": 50}],
                         ids=["global_y", "price_grid3", "refactor50"])
def test_variants_256(spx, golden, kw, flipc, rule):
    """The global-memory ratio test, a three-workgroup pricing grid and a
    reinversion every 50 pivots (k_box_rhs before it) walk the same pivots."""
    m, n, seed = 256, 1024, 3
    r, tp, tq, x, up = _solve(spx, m, n, seed, flipc, rule, **kw)
    print(f"{kw} flipc={flipc} {rule}: z={r.z:.13g} pivots={r.pivots}")
    _check_against_golden(spx, golden[0][(m, n, seed, flipc, rule)], r, tp, tq, x, up, _lp(m, n, seed, flipc))


@pytest.mark.parametrize("flipc", [0, 1])
def test_certificate_1024(spx, golden, flipc):
    """Steepest edge at 1024 x 4096: z against HiGHS and the certificate
    recomputed on the CPU from the returned basis and placements."""
    m, n, seed = dual_ref.SHAPES[4]
    At, b, c, u, A = _lp(m, n, seed, flipc)
    g = golden[0][(m, n, seed, flipc, ref.STEEPEST)]
    z = g["highs_z"]
    with _ctx(spx, m, n, seed, flipc, ref.STEEPEST, trace=0) as ctx:
        r = ctx.solve()
        x, up = ctx.primal()
    print(f"{m}x{n} flipc={flipc}: z={r.z:.13g} (HiGHS {z:.13g}) pivots={r.pivots} (reference {g['ref_pivots']})")
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    assert len(set(r.b_ixs.tolist())) == m
    res = _check_primal(x, up, A, b, u)
    viol, dviol, zc = ref.certificate(A, b, c, u, r.b_ixs, up)
    print(f"primal residual {res:.2e}, bound violation {viol:.2e}, reduced-cost sign violation {dviol:.2e}")
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= REL * abs(z)
    assert int(up.sum()) == len(g["ref_at_upper"])


@pytest.mark.parametrize("rule", RULES)
def test_infinite_bounds_change_nothing(spx, rule):
    """All bounds infinite through spx_set_bounds, and finite bounds set and
    removed again: the trace of a context that never called it, bit for bit."""
    m, n, seed = 256, 1024, 3
    At, b, c, u, _ = _lp(m, n, seed, 0)
    with _ctx(spx, m, n, seed, 0, rule, upper=None) as ctx:
        r0 = ctx.solve()
        t0 = [t.tolist() for t in ctx.trace()]
        x0, up0 = ctx.primal()
        assert not up0.any() and np.isinf(ctx.bounds()).all()
    with _ctx(spx, m, n, seed, 0, rule, upper=np.full(n, np.inf)) as ctx:
        r1 = ctx.solve()
        t1 = [t.tolist() for t in ctx.trace()]
    with _ctx(spx, m, n, seed, 0, rule) as ctx:
        ctx.set_bounds(None)
        assert np.isinf(ctx.bounds()).all()
        r2 = ctx.solve()
        t2 = [t.tolist() for t in ctx.trace()]
        x2, up2 = ctx.primal()
    assert r0.status == spx.SolveStatus.OptimumFound
    for r, t in ((r1, t1), (r2, t2)):
        assert t == t0 and r.pivots == r0.pivots and r.z == r0.z
        assert r.b_ixs.tolist() == r0.b_ixs.tolist() and np.array_equal(r.x_b, r0.x_b)
    assert np.array_equal(x2, x0) and not up2.any()


@pytest.mark.parametrize("rule", RULES)
def test_bound_resolve(spx, golden, rule):
    """Solve, tighten (every 8th finite structural bound halved), loosen (every
    16th finite bound to +inf; see the module text): set_bounds + solve from the
    old basis, against HiGHS on the modified LP."""
    m, n, seed = 256, 1024, 3
    res = golden[1]
    assert (res["m"], res["n"], res["seed"], res["flipc"]) == (m, n, seed, 0)
    At, b, c, u, A = _lp(m, n, seed, 0)
    ns = n - m
    u1 = u.copy()
    u1[np.where(np.isfinite(u[:ns]))[0][::8]] *= 0.5
    u2_all = u1.copy()
    u2_all[np.where(np.isfinite(u1))[0][::16]] = np.inf
    with _ctx(spx, m, n, seed, 0, rule, trace=4096) as ctx:
        r0 = ctx.solve()
        assert r0.status == spx.SolveStatus.OptimumFound
        assert r0.pivots == golden[0][(m, n, seed, 0, rule)]["ref_pivots"]
        # tighten
        ctx.set_bounds(u1)
        s = ctx.state()
        assert s["status"] == spx.SolveStatus.MaxIter and s["pivots"] == r0.pivots
        assert s["b_ixs"].tolist() == r0.b_ixs.tolist()  # the old basis
        x, up = ctx.primal()
        out = (x < -1e-9) | (x > u1 + 1e-9)
        assert out.any()  # ... which the new bounds make primal infeasible
        r1 = ctx.solve()
        tp, tq = ctx.trace()
        z1 = res["tight_highs_z"]
        k1 = r1.pivots - r0.pivots
        fresh1 = res[f"tight_fresh_pivots_{rule}"]
        print(f"{rule}: solve {r0.pivots} pivots; tightened: {k1} more (fresh {fresh1}), z={r1.z:.13g} (HiGHS {z1:.13g})")
        assert r1.status == spx.SolveStatus.OptimumFound
        assert abs(r1.z - z1) <= REL * abs(z1), (r1.z, z1)
        assert 0 < k1 < fresh1
        # the first re-solve pivot leaves a row of the old basis that the tightening pushed out of its bounds
        q = int(tq[r0.pivots])
        assert out[r0.b_ixs[q]]
        x, up = ctx.primal()
        _check_primal(x, up, A, b, u1)
        # loosen, as stated: a column at upper loses its bound and has no dual feasible side left
        kept = np.flatnonzero(up & ~np.isfinite(u2_all))
        assert kept.tolist() == res["loose_kept"]
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_bounds(u2_all)
        assert ei.value.code == -5 and "not dual feasible" in str(ei.value)
        assert "column %d" % res["loose_all_bad_column"] in str(ei.value) and "no upper bound" in str(ei.value)
        # ... and with those bounds kept: nothing the dual method has to repair
        u2 = u2_all.copy()
        u2[kept] = u1[kept]
        ctx.set_bounds(u2)
        assert ctx.state()["b_ixs"].tolist() == r1.b_ixs.tolist()
        r2 = ctx.solve()
        z2 = res["loose_highs_z"]
        k2 = r2.pivots - r1.pivots
        print(f"{rule}: loosened: {k2} more pivots (fresh {res[f'loose_fresh_pivots_{rule}']}), z={r2.z:.13g} "
              f"(HiGHS {z2:.13g})")
        assert r2.status == spx.SolveStatus.OptimumFound
        assert abs(r2.z - z2) <= REL * abs(z2), (r2.z, z2)
        assert k2 < res[f"loose_fresh_pivots_{rule}"]
        x, up = ctx.primal()
        _check_primal(x, up, A, b, u2)


def test_reset_and_rhs_in_a_boxed_context(spx, golden):
    """spx_reset puts every column back at lower (the same solve again), and
    spx_set_rhs takes the caller's b, not the effective one."""
    m, n, seed, flipc = 130, 390, 2, 1
    At, b, c, u, A = _lp(m, n, seed, flipc)
    g = golden[0][(m, n, seed, flipc, ref.DANTZIG)]
    with _ctx(spx, m, n, seed, flipc, ref.DANTZIG) as ctx:
        r = ctx.solve()
        ctx.reset()
        assert not ctx.primal()[1].any()
        r2 = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        _check_against_golden(spx, g, r2, tp.tolist(), tq.tolist(), x, up, _lp(m, n, seed, flipc))
        assert r2.z == r.z
        b2 = b * 1.05
        ctx.set_rhs(b2)
        r3 = ctx.solve()
        x, up = ctx.primal()
    want = ref.dual_simplex_box(A, b2, c, u, rule=ref.DANTZIG, trace_cap=0)
    assert want.status == dual_ref.OPTIMUM and r3.status == spx.SolveStatus.OptimumFound
    assert abs(r3.z - want.z) <= REL * abs(want.z), (r3.z, want.z)
    _check_primal(x, up, A, b2, u)


def test_set_basis_and_reinvert_in_a_boxed_context(spx, golden):
    """spx_set_basis and spx_reinvert called directly: k_box_rhs runs before
    x_b is recomputed.  The basis after 60 pivots is set again at the optimum,
    where 10 of its columns sit non-basic at upper: they become basic with a
    stale flag, which must not count.  x_b is read through spx_get_primal right
    after each call, before any solve."""
    m, n, seed, flipc = 130, 390, 2, 1
    At, b, c, u, A = _lp(m, n, seed, flipc)
    g = golden[0][(m, n, seed, flipc, ref.DANTZIG)]
    bmax = np.max(np.abs(b))
    with _ctx(spx, m, n, seed, flipc, ref.DANTZIG) as ctx:
        ctx.iterate(60)
        mid = ctx.state()["b_ixs"].copy()
        r = ctx.solve()
        x_opt, up_opt = ctx.primal()
        assert r.status == spx.SolveStatus.OptimumFound and np.flatnonzero(up_opt).tolist() == g["ref_at_upper"]
        stale = sorted(set(mid.tolist()) & set(g["ref_at_upper"]))
        assert len(stale) == 10, stale
        # reinvert at the optimum: the same vertex from b_eff
        ctx.reinvert()
        x, up = ctx.primal()
        assert np.array_equal(up, up_opt) and np.max(np.abs(x - x_opt)) <= 1e-9 * bmax
        assert ctx.solve().pivots == r.pivots  # still optimal
        # the mid-solve basis with the optimum's placements
        ctx.set_basis(mid)
        x, up = ctx.primal()
        assert ctx.state()["b_ixs"].tolist() == mid.tolist()
        assert not up[mid].any()  # a basic column has no placement
        want_up = up_opt.copy()
        want_up[mid] = False
        assert np.array_equal(up, want_up)
        assert np.array_equal(x[up], u[up])
        res = float(np.max(np.abs(A @ x - b)))
        print(f"after set_basis: {len(stale)} stale flags, |A x - b| = {res:.2e}")
        assert res <= 1e-9 * bmax, res
        B = np.ascontiguousarray(At[mid].T)
        xb = np.linalg.solve(B, b - A[:, up] @ u[up])
        assert np.max(np.abs(x[mid] - xb)) <= 1e-9 * bmax
        r2 = ctx.solve()
        x, up = ctx.primal()
    assert r2.status == spx.SolveStatus.OptimumFound
    assert abs(r2.z - g["highs_z"]) <= REL * abs(g["highs_z"]), (r2.z, g["highs_z"])
    assert np.flatnonzero(up).tolist() == g["ref_at_upper"]
    _check_primal(x, up, A, b, u)


def test_weights_survive_set_bounds(spx):
    """Steepest-edge weights after set_bounds mid-solve: B^-1 is untouched, so
    they are still the squared row norms of numpy's inverse (1e-9 relative, the
    bound of tests/test_gpu_dual_se.py)."""
    m, n, seed = 256, 1024, 3
    At, b, c, u, _ = _lp(m, n, seed, 0)
    u1 = u.copy()
    u1[np.where(np.isfinite(u[:n - m]))[0][::8]] *= 0.5
    with _ctx(spx, m, n, seed, 0, ref.STEEPEST) as ctx:
        ctx.iterate(60)
        ctx.set_bounds(u1)
        s = ctx.state()
        assert s["pivots"] == 60
        w = ctx.dual_weights()
        B = np.ascontiguousarray(At[np.asarray(s["b_ixs"], dtype=np.int64)].T)
        want = dual_se_ref.row_norms2(np.linalg.inv(B))
        err = float(np.max(np.abs(w - want) / want))
        print(f"largest relative weight error after set_bounds: {err:.2e}")
        assert err <= REL, err
        r = ctx.solve()
        assert r.status == spx.SolveStatus.OptimumFound


def test_infeasible_by_a_bound(spx):
    A, b, c, u = ref.tiny_box_infeasible()
    for rule in (spx.DUAL_PRICING_DANTZIG, spx.DUAL_PRICING_STEEPEST):
        with spx.Context(np.ascontiguousarray(A.T), b, c, window=-1, algorithm=spx.ALGO_DUAL, dual_pricing=rule,
                         upper=u) as ctx:
            r = ctx.solve()
        assert r.status == spx.SolveStatus.Infeasible and r.status == 4 and r.pivots == 2, r


def test_errors(spx):
    m, n, seed = 7, 20, 0
    At, b, c, u, _ = _lp(m, n, seed, 1)
    # a flipc column (c_j > 0) without its bound: not dual feasible on either side
    j = int(np.flatnonzero(c > 0)[0])
    bad = u.copy()
    bad[j] = np.inf
    with pytest.raises(spx.SimplexError) as ei:
        _ctx(spx, m, n, seed, 1, ref.DANTZIG, upper=bad)
    assert ei.value.code == -5 and "not dual feasible" in str(ei.value) and "column %d" % j in str(ei.value)
    assert "no upper bound" in str(ei.value)
    with _ctx(spx, m, n, seed, 1, ref.DANTZIG) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_algorithm(spx.ALGO_PRIMAL)
        assert ei.value.code == -5 and "primal" in str(ei.value)
        for v, word in ((-1.0, "negative"), (np.nan, "NaN")):
            w = u.copy()
            w[3] = v
            with pytest.raises(spx.SimplexError) as ei:
                ctx.set_bounds(w)
            assert ei.value.code == -1 and "column 3" in str(ei.value) and word in str(ei.value)
        with pytest.raises(ValueError):
            ctx.set_bounds(u[:-1])
        assert np.array_equal(ctx.bounds(), u)  # the refused calls changed nothing
        assert ctx.solve().status == spx.SolveStatus.OptimumFound
    # bounds on a context that runs the primal loop: the library's refusal
    A0, b0, c0 = dual_ref.covering(m, n, seed)
    with pytest.raises(spx.SimplexError) as ei:
        spx.Context(np.ascontiguousarray(A0.T), np.abs(b0), c0, window=-1, upper=u)
    assert ei.value.code == -5 and "SPX_ALGO_DUAL" in str(ei.value)


def test_cli_bounds(golden, tmp_path):
    """./solver --dual --bounds FILE, and the refusal without --dual."""
    m, n, seed, flipc = 65, 200, 1, 1
    _, b, c, u, A = _lp(m, n, seed, flipc)
    p = str(tmp_path / "cover.txt")
    with open(p, "w") as f:
        f.write(f"{m} {n}\n")
        for row in A:
            f.write(" ".join("%.17g" % v for v in row) + "\n")
        f.write(" ".join("%.17g" % v for v in b) + "\n")
        f.write(" ".join("%.17g" % v for v in c) + "\n")
    pb = str(tmp_path / "bounds.txt")
    with open(pb, "w") as f:
        f.write("\n".join("inf" if np.isinf(v) else "%.17g" % v for v in u) + "\n")
    solver = os.path.join(ROOT, "solver")
    for rule in RULES:
        r = subprocess.run([solver, "--dual", "--dual-pricing", rule, "--bounds", pb, "--json", "--no-iter-lines", p],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        js = json.loads(r.stdout.splitlines()[-1])
        g = golden[0][(m, n, seed, flipc, rule)]
        assert js["status"] == 1 and js["pivots"] == g["ref_pivots"]
        assert abs(js["z"] - g["highs_z"]) <= REL * abs(g["highs_z"])
    r = subprocess.run([solver, "--bounds", pb, "--json", "--no-iter-lines", p], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "SPX_ALGO_DUAL" in r.stderr
