"""GPU: general bounds l <= x <= u (spx_set_bounds_lu) on the LPs
of tests/primal_lu_ref.py: general_lu(m, n, seed) -- finite lower bounds of
either sign, fixed columns and free columns, a slack basis that is feasible on
neither side -- under SPX_ALGO_PRIMAL_BOX with phase 1 (the *_f kernels), and
shift_lp (no free column, every range finite) under both bounded loops (the
existing kernels on the shifted problem, k_box_rhs_lu behind them).

Golden values (tests/golden/primal_lu_optima.json, written by
tests/golden/make_golden_primal_lu.py): pivot count, the first 200 (p, q) pairs,
the final basis and at-upper set, the flip / to-upper counts and the phase-1
counters of the numpy restatement, and HiGHS's optimum with
bounds=list(zip(l, u)).  The generator refuses a case whose smallest relative
gap between the best and the second-best key of either argmin, or between u_p
and t_q, is below 1e-6 (the smallest over the committed cases is 3.8e-6), so
pass-for-pass equality does not depend on the fp64 summation order.

Shapes: 7 x 20, 65 x 200 (two row blocks of k_pbox_vtb), 130 x 390 (three row
blocks, two column chunks), 256 x 1024 (whole solve).
"""
import json
import os
import subprocess

import numpy as np
import pytest

import primal_lu_ref as ref
import primal_phase1_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "primal_lu_optima.json")) as f:
        g = json.load(f)
    g["by_shape"] = {(c["m"], c["n"], c["seed"]): c for c in g["cases"]}
    return g


_LPS = {}


def _lp(m, n, seed, kind="general"):
    """(A_cols (n, m), b, c, l, u, A (m, n)), built once."""
    k = (m, n, seed, kind)
    if k not in _LPS:
        A, b, c, l, u = ref.general_lu(m, n, seed) if kind == "general" else ref.shift_lp(m, n, seed)
        _LPS[k] = (np.ascontiguousarray(A.T), b, c, l, u, A)
    return _LPS[k]


def _ctx(spx, lp, algorithm=None, phase1=True, **kw):
    At, b, c, l, u = lp[:5]
    kw.setdefault("trace", 200)
    algorithm = spx.ALGO_PRIMAL_BOX if algorithm is None else algorithm
    return spx.Context(At, b, c, algorithm=algorithm, lower=l, upper=u,
                       primal_phase1=phase1 and algorithm == spx.ALGO_PRIMAL_BOX, **kw)


def _check_primal(x, up, b_ixs, A, b, l, u):
    res = float(np.max(np.abs(A @ x - b)))
    assert res <= 1e-9 * max(1.0, np.max(np.abs(b))), res
    assert np.max(l - x) <= 1e-9 and np.max(x - u) <= 1e-9, (np.max(l - x), np.max(x - u))
    nb = np.ones(len(x), dtype=bool)
    nb[b_ixs] = False
    want = np.where(up, u, np.where(np.isneginf(l), 0.0, l))
    assert np.array_equal(x[nb], want[nb])  # exactly l_j or u_j (0 for a free column), not l + (u - l)
    assert not np.any(up & ~nb) and not np.any(up & ~np.isfinite(u))


def _check_optimum(spx, r, x, up, A, b, c, l, u, z):
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    _check_primal(x, up, r.b_ixs, A, b, l, u)
    assert abs(float(c @ x) - r.z) <= REL * abs(z), (float(c @ x), r.z)
    assert np.array_equal(x[r.b_ixs], r.x_b)  # x_b comes back in the caller's variables
    viol, dviol, zc = ref.certificate_lu(A, b, c, l, u, r.b_ixs, up)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= REL * abs(z)


def _counters(g):
    return (g["p1_passes"], g["p1_pivots"], g["ninf0"], 0)


def _solve(spx, lp, **kw):
    with _ctx(spx, lp, **kw) as ctx:
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        return r, tp.tolist(), tq.tolist(), x, up, ctx.primal_flips(), ctx.primal_phase1()


def _check_against_golden(spx, g, lp, r, tp, tq, x, up, flips, ph):
    _, b, c, l, u, A = lp
    print(f"{g['m']}x{g['n']}: z={r.z:.13g} pivots={r.pivots} (golden {g['ref_pivots']}) flips={flips} (golden "
          f"{g['flips']}, {g['to_upper']}) phase 1 {ph} (golden {_counters(g)})")
    assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
    k = min(g["ref_pivots"], 200)
    assert tp[:k] == g["ref_trace_p"][:k]
    assert tq[:k] == g["ref_trace_q"][:k]
    assert flips == (g["flips"], g["to_upper"]), flips
    assert ph == _counters(g), ph
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(up).tolist() == g["ref_at_upper"]
    _check_optimum(spx, r, x, up, A, b, c, l, u, g["highs_z"])


@pytest.mark.parametrize("m,n,seed", [(7, 20, 0), (65, 200, 1), (130, 390, 2)])
def test_trace_parity(spx, golden, m, n, seed):
    lp = _lp(m, n, seed)
    g = golden["by_shape"][(m, n, seed)]
    assert g["free_entered"] > 0 and g["free_basic"] > 0  # free columns enter and stay basic
    _check_against_golden(spx, g, lp, *_solve(spx, lp))


@pytest.mark.parametrize("kw", [{"global_y": True}, {"price_grid": 3}, {"refactor_every": 50}],
                         ids=["global_y", "price_grid3", "refactor50"])
def test_variants_65(spx, golden, kw):
    """y in global memory, a three-workgroup pricing grid and a reinversion
    every 50 pivots (it lands inside phase 1: k_pbox_classify_f) walk the same
    passes with the same counters."""
    m, n, seed = 65, 200, 1
    lp = _lp(m, n, seed)
    _check_against_golden(spx, golden["by_shape"][(m, n, seed)], lp, *_solve(spx, lp, **kw))


def test_whole_solve_256(spx, golden):
    m, n, seed = 256, 1024, 3
    lp = _lp(m, n, seed)
    g = golden["by_shape"][(m, n, seed)]
    r, tp, tq, x, up, flips, ph = _solve(spx, lp)
    print(f"{m}x{n}: z={r.z:.13g} (HiGHS {g['highs_z']:.13g}) pivots={r.pivots} (reference {g['ref_pivots']}) "
          f"flips={flips} phase 1 {ph} (golden {_counters(g)})")
    _, b, c, l, u, A = lp
    _check_optimum(spx, r, x, up, A, b, c, l, u, g["highs_z"])


def test_shift_both_loops_65(spx, golden):
    """No free column: the existing kernels on the shifted problem.  Both loops
    solve it from the slack basis to HiGHS's optimum, the bounded primal loop
    along the golden trace; then a new right-hand side and moved lower bounds,
    each re-solved from the old basis."""
    g = golden["shift"]
    m, n, seed = g["m"], g["n"], g["seed"]
    lp = _lp(m, n, seed, "shift")
    _, b, c, l, u, A = lp
    b2 = primal_phase1_ref.rhs_variant(b, seed)
    l2 = ref.moved_lower(l, u, seed)
    zs = {}
    for algo in (spx.ALGO_PRIMAL_BOX, spx.ALGO_DUAL):
        with _ctx(spx, lp, algorithm=algo) as ctx:
            lb, ub = ctx.bounds_lu()
            assert np.array_equal(lb, l) and np.array_equal(ub, u) and np.array_equal(ctx.bounds(), u)
            r = ctx.solve()
            x, up = ctx.primal()
            print(f"shift, algorithm {algo}: z={r.z:.13g} (HiGHS {g['highs_z']:.13g}) pivots={r.pivots}")
            _check_optimum(spx, r, x, up, A, b, c, l, u, g["highs_z"])
            assert abs(ctx.objective() - r.z) <= REL * abs(r.z)
            if algo == spx.ALGO_PRIMAL_BOX:
                tp, tq = ctx.trace()
                k = min(g["ref_pivots"], 200)
                assert r.pivots == g["ref_pivots"] and tp.tolist()[:k] == g["ref_trace_p"][:k]
                assert tq.tolist()[:k] == g["ref_trace_q"][:k] and r.b_ixs.tolist() == g["ref_b_ixs"]
                assert np.flatnonzero(up).tolist() == g["ref_at_upper"]
                assert ctx.primal_phase1() == _counters(g) and ctx.primal_flips() == (g["flips"], g["to_upper"])
            zs[algo] = r.z
            first = r.pivots
            ctx.set_rhs(b2)  # b_eff = b2 - A.l - the at-upper sum: k_box_rhs_lu behind spx_set_rhs
            r = ctx.solve()
            x, up = ctx.primal()
            print(f"  new b: z={r.z:.13g} (HiGHS {g['rhs_highs_z']:.13g}) after {r.pivots - first} more pivots")
            _check_optimum(spx, r, x, up, A, b2, c, l, u, g["rhs_highs_z"])
            second = r.pivots
            ctx.set_bounds_lu(l2, u)
            assert np.array_equal(ctx.bounds_lu()[0], l2)
            r = ctx.solve()
            x, up = ctx.primal()
            print(f"  moved l: z={r.z:.13g} (HiGHS {g['lower_highs_z']:.13g}) after {r.pivots - second} more pivots")
            _check_optimum(spx, r, x, up, A, b2, c, l2, u, g["lower_highs_z"])
            # spx_set_bounds clears the lower bounds: 0 <= x <= u - l now, and get_bounds says so
            ctx.set_bounds(u - l2)
            lb, ub = ctx.bounds_lu()
            assert not lb.any() and np.array_equal(ub, u - l2) and np.array_equal(ctx.bounds(), u - l2)
    assert abs(zs[spx.ALGO_PRIMAL_BOX] - zs[spx.ALGO_DUAL]) <= REL * abs(g["highs_z"])


def test_single_steps_65(spx, golden):
    """iterate(1) until the optimum against one solve(): the same basis, x_b and
    B^-1 bit for bit, the same counters; ninf never increases."""
    m, n, seed = 65, 200, 1
    lp = _lp(m, n, seed)
    g = golden["by_shape"][(m, n, seed)]
    with _ctx(spx, lp) as a, _ctx(spx, lp) as b:
        last = None
        for i in range(g["ref_pivots"]):
            st, piv = a.iterate(1)
            assert piv == i + 1 and st == spx.SolveStatus.MaxIter, (i, piv, st)
            ninf = a.primal_phase1()[3]
            assert last is None or ninf <= last, (i, ninf, last)
            last = ninf
        assert last == 0
        ra = a.solve()
        rb = b.solve()
        assert ra.pivots == rb.pivots == g["ref_pivots"] and ra.z == rb.z
        sa, sb = a.state(binv=True), b.state(binv=True)
        assert sa["b_ixs"].tolist() == sb["b_ixs"].tolist() == g["ref_b_ixs"]
        for k in ("x_b", "c_B", "binv"):
            assert np.array_equal(sa[k], sb[k]), k
        assert a.primal_phase1() == b.primal_phase1() == _counters(g)
        assert a.primal_flips() == b.primal_flips()


def test_unbounded_and_infeasible(spx, golden):
    A, b, c, l, u = ref.tiny_unbounded_free()
    for phase1 in (False, True):
        with spx.Context(np.ascontiguousarray(A.T), b, c, algorithm=spx.ALGO_PRIMAL_BOX, lower=l, upper=u,
                         primal_phase1=phase1) as ctx:
            r = ctx.solve()
            assert r.status == spx.SolveStatus.Unbounded and r.pivots == 0, r
            assert ctx.primal_flips() == (0, 0)
            # bounded from below it stops there: x0 = -3, the slack 4, z = 3
            ctx.set_bounds_lu(np.array([-3.0, 0.0]), u)
            r = ctx.solve()
            x, up = ctx.primal()
            assert r.status == spx.SolveStatus.OptimumFound and r.z == 3.0 and x.tolist() == [-3.0, 4.0], (r, x)
    g = golden["infeasible"]
    m, n, seed = g["m"], g["n"], g["seed"]
    _, b, c, l, u, A = _lp(m, n, seed)
    A2, b2, u2 = primal_phase1_ref.contradict(A, b, u)
    l2 = l.copy()
    l2[n - m], l2[n - m + 1] = 0.0, 0.0
    with _ctx(spx, (np.ascontiguousarray(A2.T), b2, c, l2, u2)) as ctx:
        r = ctx.solve()
        ph = ctx.primal_phase1()
        print(f"contradictory rows: status {r.status} after {r.pivots} pivots (reference {g['ref_pivots']}), phase 1 {ph}")
        assert r.status == spx.SolveStatus.Infeasible
        assert r.pivots == g["ref_pivots"]
        assert ph == (g["p1_passes"], g["p1_pivots"], g["ninf0"], g["ninf_end"])


def test_reset_repeats(spx, golden):
    m, n, seed = 65, 200, 1
    lp = _lp(m, n, seed)
    g = golden["by_shape"][(m, n, seed)]
    with _ctx(spx, lp) as ctx:
        r1 = ctx.solve()
        t1 = [t.tolist() for t in ctx.trace()]
        x1, up1 = ctx.primal()
        c1 = (ctx.primal_flips(), ctx.primal_phase1())
        ctx.reset()
        assert ctx.primal_phase1() == (0, 0, 0, 0) and np.array_equal(ctx.bounds_lu()[0], lp[3])
        r2 = ctx.solve()
        x2, up2 = ctx.primal()
        assert r1.pivots == r2.pivots == g["ref_pivots"] and r1.z == r2.z
        assert t1 == [t.tolist() for t in ctx.trace()] and c1 == (ctx.primal_flips(), ctx.primal_phase1())
        assert np.array_equal(x1, x2) and np.array_equal(up1, up2) and np.array_equal(r1.x_b, r2.x_b)


def test_warm_basis_with_free_columns(spx, golden):
    """The entry check away from the slack basis: lb_B comes from a basis that
    holds free columns, many of them at negative values.  With phase 1 off the
    host's check takes them as feasible (the optimum again, no pivot); after
    spx_set_basis every non-basic column is back at its lower bound, rows are
    out of their bounds, and phase 1 classifies with lb_B on the way back to
    the same optimum."""
    m, n, seed = 65, 200, 1
    lp = _lp(m, n, seed)
    _, b, c, l, u, A = lp
    g = golden["by_shape"][(m, n, seed)]
    free = np.isneginf(l)
    with _ctx(spx, lp) as ctx:
        r = ctx.solve()
        x, up = ctx.primal()
        assert r.pivots == g["ref_pivots"] and np.count_nonzero(free[r.b_ixs]) == g["free_basic"]
        assert np.any(x[free] < -1e-3)  # a free basic column below 0: not "below its bound"
        ctx.set_primal_phase1(False)
        r2 = ctx.solve()
        assert r2.status == spx.SolveStatus.OptimumFound and r2.pivots == r.pivots and r2.z == r.z
        assert np.array_equal(ctx.primal()[0], x)
    with _ctx(spx, lp) as ctx:
        ctx.set_basis(np.array(g["ref_b_ixs"]))
        r3 = ctx.solve()
        x3, up3 = ctx.primal()
        ph = ctx.primal_phase1()
        print(f"warm basis: {r3.pivots} pivots, phase 1 {ph}, z={r3.z:.13g} (HiGHS {g['highs_z']:.13g})")
        assert ph[2] > 0 and ph[3] == 0  # it started out of its bounds
        _check_optimum(spx, r3, x3, up3, A, b, c, l, u, g["highs_z"])
        # the restatement from the same basis: well separated, so the same passes
        w = ref.primal_simplex_lu(A, b, c, l, u, basis=g["ref_b_ixs"], trace_cap=0)
        assert min(w.gap_price, w.gap_ratio, w.gap_flip) >= 1e-6
        assert r3.pivots == w.pivots and ph == (w.p1_passes, w.p1_pivots, w.ninf0, 0), (r3.pivots, w.pivots, ph)
        assert r3.b_ixs.tolist() == w.b_ixs.tolist() and np.array_equal(up3, w.at_upper)


def test_refusals(spx, golden):
    m, n, seed = 7, 20, 0
    At, b, c, l, u, A = _lp(m, n, seed)
    lfin = np.where(np.isneginf(l), -1.0, l)  # no free column
    with spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, lower=lfin, upper=u, primal_phase1=True, trace=64) as ctx:
        def unchanged():
            lb, ub = ctx.bounds_lu()
            return np.array_equal(lb, lfin) and np.array_equal(ub, u)

        def refused(lo, hi, code, *words):
            with pytest.raises(spx.SimplexError) as ei:
                ctx.set_bounds_lu(lo, hi)
            assert ei.value.code == code and all(w in str(ei.value) for w in words), str(ei.value)
            assert unchanged()

        bad = lfin.copy()
        bad[1] = np.nan
        refused(bad, u, -1, "NaN")
        bad = lfin.copy()
        bad[1] = np.inf
        refused(bad, u, -1, "+inf")
        bad = lfin.copy()
        bad[0] = (u[0] if np.isfinite(u[0]) else 5.0) + 1.0
        hi = np.where(np.isfinite(u), u, 5.0)
        refused(bad, hi, -1, "above its upper bound")
        bad = lfin.copy()
        k = int(np.flatnonzero(np.isfinite(u))[0])
        bad[k] = -np.inf
        refused(bad, u, -1, "upper-only")
        # steepest edge first, then a free column
        ctx.set_primal_phase1(False)
        ctx.set_primal_pricing(spx.PRIMAL_PRICING_STEEPEST)
        refused(l, u, -5, "steepest-edge", "free")
        ctx.set_primal_pricing(spx.PRIMAL_PRICING_DANTZIG)
        ctx.set_primal_phase1(True)
        # a free column first, then steepest edge or the dual loop
        ctx.set_bounds_lu(l, u)
        ctx.set_primal_phase1(False)  # (phase 1 has its own refusal of steepest edge, which comes first)
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_pricing(spx.PRIMAL_PRICING_STEEPEST)
        assert ei.value.code == -5 and "free columns" in str(ei.value)
        ctx.set_primal_phase1(True)
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_algorithm(spx.ALGO_DUAL)
        assert ei.value.code == -5 and "free columns" in str(ei.value) and "dual" in str(ei.value)
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_algorithm(spx.ALGO_PRIMAL)
        assert ei.value.code == -5
        lb, ub = ctx.bounds_lu()
        assert np.array_equal(lb, l) and np.array_equal(ub, u)
        r = ctx.solve()  # the refused calls changed nothing: the golden solve
        assert r.status == spx.SolveStatus.OptimumFound and r.pivots == golden["by_shape"][(m, n, seed)]["ref_pivots"]
    # free columns on a context that runs the dual loop; SPX_ALGO_PRIMAL as spx_set_bounds refuses it
    with spx.Context(At, b, c, algorithm=spx.ALGO_DUAL) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_bounds_lu(l, u)
        assert ei.value.code == -5 and "free columns" in str(ei.value) and "dual" in str(ei.value)
        lb, ub = ctx.bounds_lu()
        assert not lb.any() and np.all(np.isposinf(ub))
    with pytest.raises(spx.SimplexError) as ei:
        spx.Context(At, b, c, algorithm=spx.ALGO_DUAL, lower=l, upper=u)
    assert ei.value.code == -5
    with pytest.raises(spx.SimplexError) as ei:
        spx.Context(At, b, c, lower=lfin, upper=u)
    assert ei.value.code == -5 and "SPX_ALGO_PRIMAL_BOX" in str(ei.value)
    with pytest.raises(spx.SimplexError) as ei:
        spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, primal_pricing=spx.PRIMAL_PRICING_STEEPEST, lower=l, upper=u)
    assert ei.value.code == -5 and "steepest-edge" in str(ei.value)


def test_zero_lower_is_todays_context(spx):
    """lower all zero: spx_set_bounds' path, the same trace and the same z bit
    for bit as the context built without `lower`."""
    m, n, seed = 65, 200, 1
    A, b, c, u = primal_phase1_ref.boxed_general(m, n, seed)
    At = np.ascontiguousarray(A.T)
    out = []
    for lower in (None, np.zeros(n)):
        with spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, lower=lower, primal_phase1=True,
                         trace=4096) as ctx:
            r = ctx.solve()
            s = ctx.state(binv=True)
            out.append((r.z, r.pivots, [t.tolist() for t in ctx.trace()], s["x_b"], s["y"], s["binv"], ctx.primal()[0],
                        ctx.primal_flips(), ctx.primal_phase1()))
    a, z = out
    assert a[0] == z[0] and a[1] == z[1] and a[2] == z[2] and a[7:] == z[7:]
    for k in (3, 4, 5, 6):
        assert np.array_equal(a[k], z[k]), k


def test_cli_lower(golden, tmp_path):
    """./solver --primal-box --phase1 --lower F --bounds G --json."""
    m, n, seed = 7, 20, 0
    _, b, c, l, u, A = _lp(m, n, seed)
    g = golden["by_shape"][(m, n, seed)]
    p = str(tmp_path / "lp.txt")
    with open(p, "w") as f:
        f.write(f"{m} {n}\n")
        for row in A:
            f.write(" ".join("%.17g" % v for v in row) + "\n")
        f.write(" ".join("%.17g" % v for v in b) + "\n")
        f.write(" ".join("%.17g" % v for v in c) + "\n")

    def dump(name, v):
        path = str(tmp_path / name)
        with open(path, "w") as f:
            f.write("\n".join(("inf" if x > 0 else "-inf") if np.isinf(x) else "%.17g" % x for x in v) + "\n")
        return path

    pb, pl = dump("bounds.txt", u), dump("lower.txt", l)
    solver = os.path.join(ROOT, "solver")
    r = subprocess.run([solver, "--primal-box", "--phase1", "--lower", pl, "--bounds", pb, "--json", "--no-iter-lines", p],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "Optimum found" in r.stdout
    js = json.loads(r.stdout.splitlines()[-1])
    assert js["status"] == 1 and js["pivots"] == g["ref_pivots"]
    assert abs(js["z"] - g["highs_z"]) <= REL * abs(g["highs_z"])
    assert (js["flip_passes"], js["to_upper"]) == (g["flips"], g["to_upper"])
    assert (js["phase1_passes"], js["phase1_pivots"], js["phase1_rows"]) == (g["p1_passes"], g["p1_pivots"], g["ninf0"])
    r = subprocess.run([solver, "--dual", "--lower", pl, "--bounds", pb, p], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "spx_set_bounds_lu failed" in r.stderr and "free columns" in r.stderr
    r = subprocess.run([solver, "--lower", pl, "--bounds", pb, p], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--lower" in r.stderr and "--primal-box" in r.stderr
