"""GPU: the bounded primal simplex loop (SPX_ALGO_PRIMAL_BOX) on
the LPs of tests/primal_box_ref.py boxed_primal(m, n, seed), and spx_set_cost.

Golden values (tests/golden/primal_box_optima.json, written by
tests/golden/make_golden_primal_box.py): pivot count, the first 200 (p, q)
pairs, the final basis, the final at-upper set and the flip / to-upper counts of
the numpy restatement tests/primal_box_ref.py, and HiGHS's optimum of the
bounded LP.  The smallest relative gap between the best and the second-best key
of either argmin over those runs is 3.3e-6 at the traced shapes, the smallest
relative distance between u_p and t_q 3.2e-3 (the generator refuses a case below
1e-6), so pass-for-pass equality does not depend on the fp64 summation order.

Shapes: 7 x 20 (m below one wave), 65 x 200 (L = 128, heavy padding), 130 x 390
(L = 256, m no multiple of 64), 256 x 1024 (multi-chunk columns, several update
workgroups, a multi-workgroup pricing grid), 1024 x 4096 (optimum and
certificate).

Cost re-solve: the boxed covering LP of tests/dual_box_ref.py is solved by the
dual loop, spx_set_cost changes the objective (the basis stays primal feasible,
not dual feasible), the bounded primal loop re-optimises from it, and after
spx_set_rhs the dual loop takes the basis back.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import dual_box_ref
import dual_ref
import primal_box_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "primal_box_optima.json")) as f:
        g = json.load(f)
    return {(c["m"], c["n"], c["seed"]): c for c in g["cases"]}, g["resolve"]


_LPS = {}


def _lp(m, n, seed):
    """(A_cols (n, m), b, c, u, A (m, n)) of the bounded LP, built once."""
    k = (m, n, seed)
    if k not in _LPS:
        A, b, c, u = ref.boxed_primal(m, n, seed)
        _LPS[k] = (np.ascontiguousarray(A.T), b, c, u, A)
    return _LPS[k]


def _ctx(spx, m, n, seed, upper="lp", **kw):
    At, b, c, u, _ = _lp(m, n, seed)
    kw.setdefault("trace", 200)
    return spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u if isinstance(upper, str) else upper, **kw)


def _check_primal(x, up, A, b, u):
    res = float(np.max(np.abs(A @ x - b)))
    assert res <= 1e-9 * np.max(np.abs(b)), res
    assert np.min(x) >= -1e-9 and np.max(x - u) <= 1e-9, (np.min(x), np.max(x - u))
    assert np.array_equal(x[up], u[up])  # exactly the bound
    return res


def _check_against_golden(spx, g, r, tp, tq, x, up, flips, lp):
    _, b, c, u, A = lp
    z = g["highs_z"]
    assert r.status == spx.SolveStatus.OptimumFound
    assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
    k = min(g["ref_pivots"], 200)
    assert tp[:k] == g["ref_trace_p"][:k]
    assert tq[:k] == g["ref_trace_q"][:k]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]  # the same pivots: the same basis order
    assert np.flatnonzero(up).tolist() == g["ref_at_upper"]
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    _check_primal(x, up, A, b, u)
    assert abs(float(c @ x) - z) <= REL * abs(z)
    assert flips == (g["flips"], g["to_upper"]), (flips, g["flips"], g["to_upper"])


def _solve(spx, m, n, seed, **kw):
    with _ctx(spx, m, n, seed, **kw) as ctx:
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        flips = ctx.primal_flips()
        assert np.array_equal(ctx.bounds(), _lp(m, n, seed)[3])
    return r, tp.tolist(), tq.tolist(), x, up, flips


@pytest.mark.parametrize("m,n,seed", dual_ref.TRACED)
def test_trace_parity(spx, golden, m, n, seed):
    g = golden[0][(m, n, seed)]
    r, tp, tq, x, up, flips = _solve(spx, m, n, seed)
    print(f"{m}x{n}: z={r.z:.13g} pivots={r.pivots} (golden {g['ref_pivots']}), flips {flips} (golden "
          f"{g['flips']}, {g['to_upper']}), {int(up.sum())} at upper")
    _check_against_golden(spx, g, r, tp, tq, x, up, flips, _lp(m, n, seed))


@pytest.mark.parametrize("kw", [{"global_y": True}, {"price_grid": 3}, {"refactor_every": 50}],
                         ids=["global_y", "price_grid3", "refactor50"])
def test_variants_256(spx, golden, kw):
    """y in global memory, a three-workgroup pricing grid and a reinversion
    every 50 pivots (it lands between flips and pivots; k_box_rhs before it)
    walk the same passes."""
    m, n, seed = 256, 1024, 3
    r, tp, tq, x, up, flips = _solve(spx, m, n, seed, **kw)
    print(f"{kw}: z={r.z:.13g} pivots={r.pivots} flips={flips}")
    _check_against_golden(spx, golden[0][(m, n, seed)], r, tp, tq, x, up, flips, _lp(m, n, seed))


def test_single_steps_256(spx, golden):
    """iterate(1) forty times against one iterate(40): the same trace and the
    same state, B^-1 included (the first flip pass of this LP comes within them
    when the golden trace says so; either way a readback follows every pass)."""
    m, n, seed = 256, 1024, 3
    g = golden[0][(m, n, seed)]
    with _ctx(spx, m, n, seed) as a, _ctx(spx, m, n, seed) as b:
        for i in range(40):
            st, piv = a.iterate(1)
            assert piv == i + 1 and st == spx.SolveStatus.MaxIter
        st, piv = b.iterate(40)
        assert piv == 40
        ta, tb = a.trace(), b.trace()
        assert ta[0].tolist() == tb[0].tolist() == g["ref_trace_p"][:40]
        assert ta[1].tolist() == tb[1].tolist() == g["ref_trace_q"][:40]
        sa, sb = a.state(binv=True), b.state(binv=True)
        for k in ("x_b", "y", "c_B", "binv"):
            assert np.array_equal(sa[k], sb[k]), k
        assert sa["b_ixs"].tolist() == sb["b_ixs"].tolist()
        assert np.array_equal(a.primal()[1], b.primal()[1]) and a.primal_flips() == b.primal_flips()
        # B^-1 as read back is the inverse of the basis columns
        At = _lp(m, n, seed)[0]
        B = np.ascontiguousarray(At[sa["b_ixs"]].T)
        assert np.max(np.abs(sa["binv"] @ B - np.eye(m))) < 1e-8
        ra, rb = a.solve(), b.solve()
        assert ra.pivots == rb.pivots == g["ref_pivots"] and ra.z == rb.z


@pytest.mark.parametrize("m,n,seed", [(257, 771, 2), (512, 2048, 0)])
def test_no_finite_bound_is_the_guarded_primal_loop(spx, m, n, seed):
    """upper=None on the seeded generator's LP: the (p, q) trace and the basis of
    ALGO_PRIMAL with the explicit B^-1 and the guarded ratio test -- the new
    kernels against the old loop, no reference involved."""
    with spx.Context(m=m, n=n, seed=seed, window=-1, ratio_test=spx.RATIO_GUARDED, trace=8192) as ctx:
        r0 = ctx.solve()
        t0 = [t.tolist() for t in ctx.trace()]
    with spx.Context(m=m, n=n, seed=seed, algorithm=spx.ALGO_PRIMAL_BOX, trace=8192) as ctx:
        r1 = ctx.solve()
        t1 = [t.tolist() for t in ctx.trace()]
        x, up = ctx.primal()
        assert ctx.primal_flips() == (0, 0) and not up.any() and np.isinf(ctx.bounds()).all()
    print(f"{m}x{n}: {r0.pivots} pivots (primal), {r1.pivots} (bounded primal), z {r0.z:.13g} / {r1.z:.13g}")
    assert r0.status == r1.status == spx.SolveStatus.OptimumFound
    assert r0.pivots < 8192 and r1.pivots == r0.pivots
    assert t1 == t0
    assert r1.b_ixs.tolist() == r0.b_ixs.tolist()
    assert abs(r1.z - r0.z) <= REL * abs(r0.z)


def test_certificate_1024(spx, golden):
    """1024 x 4096: z against HiGHS and the certificate recomputed on the CPU
    from the returned basis and placements."""
    m, n, seed = dual_ref.SHAPES[4]
    At, b, c, u, A = _lp(m, n, seed)
    g = golden[0][(m, n, seed)]
    z = g["highs_z"]
    with _ctx(spx, m, n, seed, trace=0) as ctx:
        r = ctx.solve()
        x, up = ctx.primal()
        flips = ctx.primal_flips()
    print(f"{m}x{n}: z={r.z:.13g} (HiGHS {z:.13g}) pivots={r.pivots} (reference {g['ref_pivots']}) flips={flips}")
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    assert len(set(r.b_ixs.tolist())) == m
    res = _check_primal(x, up, A, b, u)
    viol, dviol, zc = ref.certificate(A, b, c, u, r.b_ixs, up)
    print(f"primal residual {res:.2e}, bound violation {viol:.2e}, reduced-cost sign violation {dviol:.2e}")
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= REL * abs(z)


@pytest.mark.parametrize("flipc", [0, 1])
def test_cost_resolve(spx, golden, flipc):
    """Dual solve (steepest), set_cost, bounded primal re-solve from that basis;
    then set_rhs and the dual loop takes the basis back."""
    m, n, seed = 256, 1024, 3
    res = golden[1]
    g = res["flipc"][flipc]
    assert (res["m"], res["n"], res["seed"], g["flipc"]) == (m, n, seed, flipc)
    A, b, c, u = dual_box_ref.boxed(m, n, seed, bool(flipc))
    c2 = ref.cost_variant(c, n - m, seed)
    with spx.Context(np.ascontiguousarray(A.T), b, c, window=-1, algorithm=spx.ALGO_DUAL,
                     dual_pricing=spx.DUAL_PRICING_STEEPEST, upper=u) as ctx:
        r0 = ctx.solve()
        assert r0.status == spx.SolveStatus.OptimumFound
        assert abs(r0.z - g["dual_highs_z"]) <= REL * abs(g["dual_highs_z"])
        x0, up0 = ctx.primal()
        ctx.set_cost(c2)
        s = ctx.state()
        assert s["status"] == spx.SolveStatus.MaxIter and s["pivots"] == r0.pivots
        assert s["b_ixs"].tolist() == r0.b_ixs.tolist()  # the old basis
        x, up = ctx.primal()
        assert np.array_equal(up, up0) and np.max(np.abs(x - x0)) <= 1e-9 * np.max(np.abs(b))  # ... and vertex
        ctx.set_algorithm(spx.ALGO_PRIMAL_BOX)
        r1 = ctx.solve()
        x, up = ctx.primal()
        flips = ctx.primal_flips()
        z1 = g["highs_z"]
        k1 = r1.pivots - r0.pivots
        print(f"flipc={flipc}: dual {r0.pivots} pivots; new cost: {k1} primal pivots (reference {g['ref_pivots']}), "
              f"flips {flips} (reference {g['flips']}, {g['to_upper']}), z={r1.z:.13g} (HiGHS {z1:.13g})")
        assert r1.status == spx.SolveStatus.OptimumFound
        assert abs(r1.z - z1) <= REL * abs(z1), (r1.z, z1)
        assert k1 > 0
        _check_primal(x, up, A, b, u)
        viol, dviol, zc = ref.certificate(A, b, c2, u, r1.b_ixs, up)
        assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
        assert abs(zc - z1) <= REL * abs(z1)
        # back: a new right-hand side, the dual loop from the primal loop's basis
        b2 = b * 1.05
        ctx.set_rhs(b2)
        ctx.set_algorithm(spx.ALGO_DUAL)
        r2 = ctx.solve()
        x, up = ctx.primal()
        want = dual_box_ref.dual_simplex_box(A, b2, c2, u, rule=dual_box_ref.STEEPEST, trace_cap=0)
        assert want.status == dual_ref.OPTIMUM and r2.status == spx.SolveStatus.OptimumFound
        assert abs(r2.z - want.z) <= REL * abs(want.z), (r2.z, want.z)
        _check_primal(x, up, A, b2, u)
        viol, dviol, _ = ref.certificate(A, b2, c2, u, r2.b_ixs, up)
        assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)


def test_set_cost_under_the_dual_loop(spx, golden):
    """Every bound finite, so every column has a dual feasible side under the
    new objective: the dual loop's entry normalisation re-places the columns
    whose reduced cost changed sign and re-optimises.  (With the structural
    bounds alone finite, 10 slacks without a bound get a negative reduced cost
    at the old basis, which the dual loop refuses by name.)"""
    m, n, seed = 256, 1024, 3
    g = golden[1]["dual_cost"]
    A, b, c, u = dual_box_ref.boxed(m, n, seed, False)
    ub = ref.all_bounded(u, n - m)
    c3 = ref.cost_variant(c, n - m, seed)
    with spx.Context(np.ascontiguousarray(A.T), b, c, window=-1, algorithm=spx.ALGO_DUAL, upper=ub) as ctx:
        r0 = ctx.solve()
        assert r0.status == spx.SolveStatus.OptimumFound
        assert abs(r0.z - g["first_highs_z"]) <= REL * abs(g["first_highs_z"])
        up0 = ctx.primal()[1]
        ctx.set_cost(c3)
        r1 = ctx.solve()
        x, up = ctx.primal()
    z = g["highs_z"]
    print(f"dual set_cost: {r0.pivots} pivots, then {r1.pivots - r0.pivots}; z={r1.z:.13g} (HiGHS {z:.13g}); "
          f"{int((up != up0).sum())} placements differ")
    assert r1.status == spx.SolveStatus.OptimumFound
    assert abs(r1.z - z) <= REL * abs(z), (r1.z, z)
    _check_primal(x, up, A, b, ub)
    viol, dviol, _ = ref.certificate(A, b, c3, ub, r1.b_ixs, up)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)


def test_entry_check(spx):
    # a covering LP (b < 0): the slack basis is not primal feasible; the dual loop still solves it
    m, n, seed = 65, 200, 1
    A, b, c = dual_ref.covering(m, n, seed)
    with spx.Context(np.ascontiguousarray(A.T), b, c, algorithm=spx.ALGO_PRIMAL_BOX) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.solve()
        assert ei.value.code == -5 and "not primal feasible" in str(ei.value) and "row " in str(ei.value)
        assert "column" in str(ei.value)
        ctx.set_algorithm(spx.ALGO_DUAL)
        r = ctx.solve()
        want = dual_ref.dual_simplex(A, b, c)
        assert r.status == spx.SolveStatus.OptimumFound and abs(r.z - want.z) <= REL * abs(want.z)
    # a slack bound below b_i
    m, n, seed = 7, 20, 0
    At, b, c, u, A = _lp(m, n, seed)
    bad = u.copy()
    bad[n - m + 2] = 0.5 * b[2]
    with _ctx(spx, m, n, seed, upper=bad) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.solve()
        assert ei.value.code == -5 and "not primal feasible" in str(ei.value)
        assert "row 2" in str(ei.value) and "column %d" % (n - m + 2) in str(ei.value)
        ctx.set_bounds(u)  # the context stays usable
        assert ctx.solve().status == spx.SolveStatus.OptimumFound


def test_tightened_bound_is_refused_at_the_next_pass(spx, golden):
    m, n, seed = 130, 390, 2
    At, b, c, u, A = _lp(m, n, seed)
    with _ctx(spx, m, n, seed) as ctx:
        r = ctx.solve()
        x, up = ctx.primal()
        row = int(np.argmax(np.where(r.b_ixs < n - m, r.x_b, 0.0)))  # a basic structural column well above 0
        j = int(r.b_ixs[row])
        assert x[j] > 1e-3
        u2 = u.copy()
        u2[j] = 0.5 * x[j]
        ctx.set_bounds(u2)  # accepted: placements kept
        assert ctx.state()["b_ixs"].tolist() == r.b_ixs.tolist()
        with pytest.raises(spx.SimplexError) as ei:
            ctx.solve()
        assert ei.value.code == -5 and "not primal feasible" in str(ei.value)
        assert "row %d" % row in str(ei.value) and "column %d" % j in str(ei.value)
        # the dual loop repairs it from the same basis
        ctx.set_algorithm(spx.ALGO_DUAL)
        r2 = ctx.solve()
        x2, up2 = ctx.primal()
    assert r2.status == spx.SolveStatus.OptimumFound and r2.pivots > r.pivots
    _check_primal(x2, up2, A, b, u2)
    viol, dviol, _ = ref.certificate(A, b, c, u2, r2.b_ixs, up2)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)


def test_refusals(spx):
    m, n, seed = 7, 20, 0
    At, b, c, u, _ = _lp(m, n, seed)
    for kw, word in (({"window": 8}, "window"), ({"window": 8, "tableau": True}, "tableau"),
                     ({"nranks": 2}, "rank"), ({"ratio_test": spx.RATIO_HARRIS}, "Harris")):
        with pytest.raises(spx.SimplexError) as ei:
            spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, **kw)
        assert ei.value.code == -1 and word in str(ei.value) and "bounded primal" in str(ei.value), (kw, str(ei.value))
    with _ctx(spx, m, n, seed) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.price()
        assert ei.value.code == -5 and "SPX_ALGO_PRIMAL_BOX" in str(ei.value)
        with pytest.raises(spx.SimplexError) as ei:
            ctx.pivot()
        assert ei.value.code == -5
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_algorithm(spx.ALGO_PRIMAL)  # finite bounds: still the plain primal loop's refusal
        assert ei.value.code == -5 and "primal" in str(ei.value)
        assert ctx.solve().status == spx.SolveStatus.OptimumFound


def test_unbounded_and_tiny_flip(spx):
    A, b, c, u = ref.tiny_unbounded()
    with spx.Context(np.ascontiguousarray(A.T), b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, trace=8) as ctx:
        r = ctx.solve()
        s = ctx.state(binv=True)  # (a pass without a pivot leaves a readable state)
    assert r.status == spx.SolveStatus.Unbounded and r.status == 2 and r.pivots == 1
    assert s["binv"].tolist() == [[1.0]] and s["b_ixs"].tolist() == [0]
    A, b, c, u = ref.tiny_flip()
    with spx.Context(np.ascontiguousarray(A.T), b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, trace=8) as ctx:
        st, piv = ctx.iterate(1)  # a flip pass, then the pivot
        assert piv == 1 and ctx.primal_flips() == (1, 0)
        r = ctx.solve()
        x, up = ctx.primal()
    assert r.status == spx.SolveStatus.OptimumFound and r.pivots == 1 and r.z == 5.0
    assert x.tolist() == [1.0, 3.0, 0.0] and up.tolist() == [True, False, False]


def test_reset_clears_placements_and_counters(spx, golden):
    m, n, seed = 65, 200, 1
    g = golden[0][(m, n, seed)]
    with _ctx(spx, m, n, seed) as ctx:
        r = ctx.solve()
        assert ctx.primal_flips() == (g["flips"], g["to_upper"]) and ctx.primal()[1].any()
        ctx.reset()
        assert ctx.primal_flips() == (0, 0) and not ctx.primal()[1].any()
        r2 = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        _check_against_golden(spx, g, r2, tp.tolist(), tq.tolist(), x, up, ctx.primal_flips(), _lp(m, n, seed))
        assert r2.z == r.z


def test_cli_primal_box(golden, tmp_path):
    """./solver --primal-box --bounds FILE, and the refusals."""
    m, n, seed = 65, 200, 1
    _, b, c, u, A = _lp(m, n, seed)
    p = str(tmp_path / "lp.txt")
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
    g = golden[0][(m, n, seed)]
    r = subprocess.run([solver, "--primal-box", "--bounds", pb, "--json", "--no-iter-lines", p], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.splitlines()[-1])
    assert js["status"] == 1 and js["pivots"] == g["ref_pivots"]
    assert abs(js["z"] - g["highs_z"]) <= REL * abs(g["highs_z"])
    assert (js["flip_passes"], js["to_upper"]) == (g["flips"], g["to_upper"])
    r = subprocess.run([solver, "--primal-box", "--dual", "--bounds", pb, p], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--dual" in r.stderr
    r = subprocess.run([solver, "--bounds", pb, "--json", "--no-iter-lines", p], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "SPX_ALGO_DUAL" in r.stderr
