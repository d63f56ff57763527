"""GPU: the bounded primal simplex loop's phase 1 (SPX_FLAG_PRIMAL_PHASE1,
spx_set_primal_phase1) on the LPs of tests/primal_phase1_ref.py
boxed_general(m, n, seed), whose slack basis is neither primal nor dual
feasible.

Golden values (tests/golden/primal_phase1_optima.json, written by
tests/golden/make_golden_primal_phase1.py): pivot count, the first 200 (p, q)
pairs, the final basis and at-upper set, the flip / to-upper counts and the
phase-1 pass / pivot / entry-row counts of the numpy restatement
tests/primal_phase1_ref.py, and HiGHS's optimum.  The generator refuses a case
whose smallest relative gap between the best and the second-best key of either
argmin, or between u_p and t_q, is below 1e-6 (the smallest over the committed
cases is 3.4e-6), so pass-for-pass equality does not depend on the fp64
summation order.

Shapes: 7 x 20 (one partial row block and one column chunk of k_pbox_vtb), 65 x
200 (two row blocks, the second with one row), 130 x 390 (three row blocks, two
column chunks), 256 x 1024 (whole solve).
"""
import json
import os
import subprocess

import numpy as np
import pytest

import dual_box_ref
import dual_ref
import primal_box_ref
import primal_phase1_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "primal_phase1_optima.json")) as f:
        g = json.load(f)
    g["by_shape"] = {(c["m"], c["n"], c["seed"]): c for c in g["cases"]}
    return g


@pytest.fixture(scope="module")
def pbox_golden():
    with open(os.path.join(ROOT, "tests", "golden", "primal_box_optima.json")) as f:
        g = json.load(f)
    return {(c["m"], c["n"], c["seed"]): c for c in g["cases"]}


_LPS = {}


def _lp(m, n, seed):
    """(A_cols (n, m), b, c, u, A (m, n)) of boxed_general, built once."""
    k = (m, n, seed)
    if k not in _LPS:
        A, b, c, u = ref.boxed_general(m, n, seed)
        _LPS[k] = (np.ascontiguousarray(A.T), b, c, u, A)
    return _LPS[k]


def _ctx(spx, lp, phase1=True, **kw):
    At, b, c, u = lp[:4]
    kw.setdefault("trace", 200)
    return spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, primal_phase1=phase1, **kw)


def _check_primal(x, up, A, b, u):
    res = float(np.max(np.abs(A @ x - b)))
    assert res <= 1e-9 * np.max(np.abs(b)), res
    assert np.min(x) >= -1e-9 and np.max(x - u) <= 1e-9, (np.min(x), np.max(x - u))
    assert np.array_equal(x[up], u[up])  # exactly the bound


def _check_optimum(spx, r, x, up, A, b, c, u, z):
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    _check_primal(x, up, A, b, u)
    assert abs(float(c @ x) - z) <= REL * abs(z)
    viol, dviol, zc = ref.certificate(A, b, c, u, r.b_ixs, up)
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
    _, b, c, u, A = lp
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
    _check_optimum(spx, r, x, up, A, b, c, u, g["highs_z"])


@pytest.mark.parametrize("m,n,seed", [(7, 20, 0), (65, 200, 1), (130, 390, 2)])
def test_trace_parity(spx, golden, m, n, seed):
    lp = _lp(m, n, seed)
    _check_against_golden(spx, golden["by_shape"][(m, n, seed)], lp, *_solve(spx, lp))


@pytest.mark.parametrize("kw", [{"global_y": True}, {"price_grid": 3}, {"refactor_every": 50}],
                         ids=["global_y", "price_grid3", "refactor50"])
def test_variants_130(spx, golden, kw):
    """y in global memory, a three-workgroup pricing grid and a reinversion
    every 50 pivots (it lands inside phase 1: the rows are classified again)
    walk the same passes with the same counters."""
    m, n, seed = 130, 390, 2
    lp = _lp(m, n, seed)
    _check_against_golden(spx, golden["by_shape"][(m, n, seed)], lp, *_solve(spx, lp, **kw))


def test_whole_solve_256(spx, golden):
    m, n, seed = 256, 1024, 3
    lp = _lp(m, n, seed)
    g = golden["by_shape"][(m, n, seed)]
    r, tp, tq, x, up, flips, ph = _solve(spx, lp)
    print(f"{m}x{n}: z={r.z:.13g} (HiGHS {g['highs_z']:.13g}) pivots={r.pivots} (reference {g['ref_pivots']}) "
          f"flips={flips} phase 1 {ph} (golden {_counters(g)})")
    assert ph == _counters(g), ph
    _, b, c, u, A = lp
    _check_optimum(spx, r, x, up, A, b, c, u, g["highs_z"])


def test_single_steps_65(spx, golden):
    """iterate(1) until the optimum against one solve(): the same basis, x_b and
    B^-1 (bit for bit); the infeasible-row count never increases; y read in the
    middle of phase 1 is c_B B^-1 although phase 1 does not maintain it."""
    m, n, seed = 65, 200, 1
    lp = _lp(m, n, seed)
    g = golden["by_shape"][(m, n, seed)]
    with _ctx(spx, lp) as a, _ctx(spx, lp) as b, _ctx(spx, lp) as c:
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
        # the stale-y rule, half-way through phase 1
        k = g["p1_pivots"] // 2
        st, piv = c.iterate(k)
        ph = c.primal_phase1()
        assert piv == k and ph[1] == k and ph[3] > 0, (piv, ph)
        sc = c.state(binv=True)
        want = sc["c_B"] @ sc["binv"]
        assert np.max(np.abs(sc["y"] - want)) <= 1e-10, np.max(np.abs(sc["y"] - want))
        assert np.any(sc["c_B"] != 0.0)
        e = c.reduced_costs()
        At = lp[0]
        assert np.max(np.abs(e - (At @ want - lp[2]))) <= 1e-9
        rc = c.solve()  # and the loop goes on from there
        assert rc.pivots == g["ref_pivots"] and rc.b_ixs.tolist() == g["ref_b_ixs"]
        assert abs(rc.z - g["highs_z"]) <= REL * abs(g["highs_z"])


def test_infeasible(spx, golden):
    A, b, c, u = ref.tiny_infeasible()
    with spx.Context(np.ascontiguousarray(A.T), b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, primal_phase1=True) as ctx:
        r = ctx.solve()
        assert r.status == spx.SolveStatus.Infeasible and r.status == 4 and r.pivots == 0
        assert ctx.primal_phase1() == (0, 0, 1, 1)
    g = golden["infeasible"]
    m, n, seed = g["m"], g["n"], g["seed"]
    _, b, c, u, A = _lp(m, n, seed)
    A2, b2, u2 = ref.contradict(A, b, u)
    with _ctx(spx, (np.ascontiguousarray(A2.T), b2, c, u2)) as ctx:
        r = ctx.solve()
        ph = ctx.primal_phase1()
        print(f"contradictory rows: status {r.status} after {r.pivots} pivots (reference {g['ref_pivots']}), phase 1 {ph}")
        assert r.status == spx.SolveStatus.Infeasible
        assert r.pivots == g["ref_pivots"]
        assert ph == (g["p1_passes"], g["p1_pivots"], g["ninf0"], g["ninf_end"])
        # the context stays usable: a feasible right-hand side
        b3 = b2.copy()
        b3[0], b3[1] = g["feasible_b01"]
        ctx.set_rhs(b3)
        r = ctx.solve()
        x, up = ctx.primal()
        _check_optimum(spx, r, x, up, A2, b3, c, u2, g["feasible_highs_z"])


def test_tiny_not_feasible(spx, golden):
    g = golden["tiny_not_feasible"]
    A, b, c, u = primal_box_ref.tiny_not_feasible()
    with spx.Context(np.ascontiguousarray(A.T), b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, primal_phase1=True,
                     trace=8) as ctx:
        r = ctx.solve()
        x, up = ctx.primal()
        ph = ctx.primal_phase1()
        ctx.reset()  # the counters go with the basis, and the same solve follows
        assert ctx.primal_phase1() == (0, 0, 0, 0)
        r2 = ctx.solve()
        assert r2.status == r.status and r2.pivots == r.pivots and r2.z == r.z and ctx.primal_phase1() == ph
    assert r.status == spx.SolveStatus.OptimumFound and r.pivots == g["ref_pivots"]
    assert ph == (g["p1_passes"], 1, g["ninf0"], 0) and g["p1_pivots"] == 1
    assert np.max(np.abs(x - np.array(g["x"]))) <= 1e-12, x
    assert abs(r.z - g["highs_z"]) <= REL * abs(g["highs_z"])


def test_flag_off_and_feasible_entry(spx, golden, pbox_golden):
    m, n, seed = 65, 200, 1
    lp = _lp(m, n, seed)
    with _ctx(spx, lp, phase1=False) as ctx:  # flag off: the refusal, word for word
        with pytest.raises(spx.SimplexError) as ei:
            ctx.solve()
        assert ei.value.code == -5 and "not primal feasible" in str(ei.value) and "no phase 1" in str(ei.value)
        assert ctx.primal_phase1() == (0, 0, 0, 0)
        ctx.set_primal_phase1(True)  # ... on: solved
        r = ctx.solve()
        assert r.status == spx.SolveStatus.OptimumFound and r.pivots == golden["by_shape"][(m, n, seed)]["ref_pivots"]
    with _ctx(spx, lp) as ctx:  # on at create, off before the first pass: the refusal again
        ctx.set_primal_phase1(False)
        with pytest.raises(spx.SimplexError) as ei:
            ctx.solve()
        assert ei.value.code == -5 and "not primal feasible" in str(ei.value)
    # flag on, feasible entry: the bounded primal loop's own golden trace, and no phase-1 pass
    m, n, seed = 130, 390, 2
    g = pbox_golden[(m, n, seed)]
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    with _ctx(spx, (np.ascontiguousarray(A.T), b, c, u)) as ctx:
        r = ctx.solve()
        tp, tq = ctx.trace()
        assert ctx.primal_phase1() == (0, 0, 0, 0)
        assert ctx.primal_flips() == (g["flips"], g["to_upper"])
        up = ctx.primal()[1]
    assert r.status == spx.SolveStatus.OptimumFound and r.pivots == g["ref_pivots"]
    k = min(g["ref_pivots"], 200)
    assert tp.tolist()[:k] == g["ref_trace_p"][:k] and tq.tolist()[:k] == g["ref_trace_q"][:k]
    assert r.b_ixs.tolist() == g["ref_b_ixs"] and np.flatnonzero(up).tolist() == g["ref_at_upper"]
    assert abs(r.z - g["highs_z"]) <= REL * abs(g["highs_z"])


def test_stuck_warm_start(spx, golden):
    """An optimal basis after set_cost and set_rhs together is neither primal
    nor dual feasible: both bounded loops refuse it; phase 1 solves from it."""
    g = golden["stuck"]
    m, n, seed = g["m"], g["n"], g["seed"]
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    c2 = primal_box_ref.cost_variant(c, n - m, seed)
    b2 = ref.rhs_variant(b, seed)
    with _ctx(spx, (np.ascontiguousarray(A.T), b, c, u), phase1=False) as ctx:
        r0 = ctx.solve()
        assert r0.status == spx.SolveStatus.OptimumFound and r0.pivots == g["first_pivots"]
        ctx.set_cost(c2)
        ctx.set_rhs(b2)
        with pytest.raises(spx.SimplexError) as ei:
            ctx.solve()
        assert ei.value.code == -5 and "not primal feasible" in str(ei.value)
        ctx.set_algorithm(spx.ALGO_DUAL)
        with pytest.raises(spx.SimplexError) as ei:
            ctx.solve()
        assert ei.value.code == -5 and "not dual feasible" in str(ei.value)
        ctx.set_algorithm(spx.ALGO_PRIMAL_BOX)
        ctx.set_primal_phase1(True)
        r = ctx.solve()
        x, up = ctx.primal()
        ph = ctx.primal_phase1()
    print(f"stuck warm start: {r.pivots - r0.pivots} pivots (reference {g['ref_pivots']}), phase 1 {ph} (reference "
          f"{g['p1_passes']}, {g['p1_pivots']}, {g['ninf0']}), z={r.z:.13g} (HiGHS {g['highs_z']:.13g})")
    # the golden stuck case passed the generator's gap check: the same passes as the reference
    assert r.pivots - r0.pivots == g["ref_pivots"], (r.pivots - r0.pivots, g["ref_pivots"])
    assert ph == (g["p1_passes"], g["p1_pivots"], g["ninf0"], 0), ph
    _check_optimum(spx, r, x, up, A, b2, c2, u, g["highs_z"])


# Hand-offs through spx_set_algorithm in the middle of phase 1 (half of its
# pivots made) and exactly at ninf == 0 (the last pass was a phase-1 pivot, so y
# is stale on the device).  Context `a` reads y back after the hand-off; context
# `h` hands off and goes on without any readback in between, so the loop that
# takes the basis must have been given y = c_B B^-1 by the hand-off itself: its
# pivots are compared with the numpy reference started from the same basis.
_HANDOFF = {}


def _handoff_case(kind, where):
    key = (kind, where)
    if key not in _HANDOFF:
        m, n, seed = 65, 200, 1
        if kind == "dual":  # every bound finite: the dual loop's normalisation takes any basis
            A, b, c, u = ref.boxed_general(m, n, seed)
            u = primal_box_ref.all_bounded(u, n - m)
        else:  # no bound at all (the primal loop refuses one): a covering LP, b < 0 at the slack basis
            A, b, c = dual_ref.covering(m, n, seed)
            u = np.full(n, np.inf)
        full = ref.primal_simplex_phase1(A, b, c, u, trace_cap=0)
        assert full.status == dual_ref.OPTIMUM and full.p1_pivots > 2
        k = full.p1_pivots // 2 if where == "mid" else full.p1_pivots
        at = ref.primal_simplex_phase1(A, b, c, u, max_iter=k, trace_cap=0)
        assert at.p1_pivots == k and (at.ninf > 0) == (where == "mid")
        assert min(full.gap_price, full.gap_ratio, full.gap_flip) >= 1e-6
        _HANDOFF[key] = (A, b, c, u, k, at, full)
    return _HANDOFF[key]


def _to_handoff_point(spx, ctx, where, k):
    if where == "mid":
        st, piv = ctx.iterate(k)
    else:
        piv = 0
        while piv == 0 or ctx.primal_phase1()[3] > 0:
            st, piv = ctx.iterate(1)
            assert piv <= k
    ph = ctx.primal_phase1()
    assert piv == k and st == spx.SolveStatus.MaxIter and ph[1] == k and (ph[3] > 0) == (where == "mid"), (piv, ph)


def _check_y_after_handoff(ctx, at):
    s = ctx.state(binv=True)
    assert s["b_ixs"].tolist() == at.b_ixs.tolist()
    assert np.any(s["c_B"] != 0.0)
    want = s["c_B"] @ s["binv"]
    assert np.max(np.abs(s["y"] - want)) <= 1e-10, np.max(np.abs(s["y"] - want))


@pytest.mark.parametrize("where", ["mid", "switch"])
def test_handoff_to_dual(spx, where):
    A, b, c, u, k, at, full = _handoff_case("dual", where)
    want = dual_box_ref.dual_simplex_box(A, b, c, u, basis=at.b_ixs, at_upper=at.at_upper, trace_cap=4096)
    assert want.status == dual_ref.OPTIMUM and min(want.gap_row, want.gap_ratio) >= 1e-6
    lp = (np.ascontiguousarray(A.T), b, c, u)
    with _ctx(spx, lp, trace=4096) as a, _ctx(spx, lp, trace=4096) as h:
        _to_handoff_point(spx, a, where, k)
        a.set_algorithm(spx.ALGO_DUAL)
        _check_y_after_handoff(a, at)
        _to_handoff_point(spx, h, where, k)
        h.set_algorithm(spx.ALGO_DUAL)
        r = h.solve()
        tp, tq = h.trace()
        x, up = h.primal()
    print(f"{where} -> dual: {r.pivots - k} dual pivots after {k} (reference {want.pivots}), z={r.z:.13g} ({want.z:.13g})")
    assert r.status == spx.SolveStatus.OptimumFound and r.pivots - k == want.pivots
    assert list(zip(tp.tolist()[k:], tq.tolist()[k:])) == want.trace
    assert r.b_ixs.tolist() == want.b_ixs.tolist() and np.array_equal(up.astype(bool), want.at_upper)
    assert abs(r.z - want.z) <= REL * abs(want.z) and abs(r.z - full.z) <= REL * abs(full.z)
    _check_primal(x, up.astype(bool), A, b, u)


@pytest.mark.parametrize("where", ["mid", "switch"])
def test_handoff_to_primal(spx, where):
    """No finite bound, so SPX_ALGO_PRIMAL accepts the context (explicit B^-1,
    guarded ratio test: primal_box_ref's loop with every bound +inf).  At
    ninf == 0 the primal loop's whole solve is compared with the reference from
    the same basis.  From the middle of phase 1 the basis is still out of its
    bounds, which the primal loop does not check: rows clamped at 0 tie at t = 0
    and after a degenerate pivot the sign of a rounding error in x_b picks the
    row, so only the first pivot is compared with the reference (run without
    its entry check), after checking that it is well separated: the pricing gap,
    no candidate row with x_b or alpha near its threshold.  That pivot needs the
    whole of y, and y is read back after it."""
    A, b, c, u, k, at, full = _handoff_case("primal", where)
    if where == "mid":
        steps = 1
        want = primal_box_ref.primal_simplex_box(A, b, c, u, basis=at.b_ixs, feas_tol=np.inf, max_iter=1, trace_cap=8)
        assert want.pivots == 1 and want.gap_price >= 1e-6
        Binv = np.linalg.inv(A[:, at.b_ixs])
        alpha = Binv @ A[:, want.trace[0][0]]
        cand = alpha > 1e-9
        assert np.min(np.abs(alpha - 1e-9)) > 1e-7 and np.min(np.abs(at.x_b[cand])) > 1e-7
        below = np.flatnonzero(cand & (at.x_b < 0))  # they tie at t = 0 exactly: the first one leaves
        assert len(below) > 0 and want.trace[0][1] == below[0]
    else:
        steps = 1 << 62
        want = primal_box_ref.primal_simplex_box(A, b, c, u, basis=at.b_ixs, trace_cap=4096)
        assert want.status == dual_ref.OPTIMUM and min(want.gap_price, want.gap_ratio) >= 1e-6
    At = np.ascontiguousarray(A.T)

    def ctx():
        return spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, primal_phase1=True, window=-1,
                           ratio_test=spx.RATIO_GUARDED, trace=4096)

    with ctx() as a, ctx() as h:
        _to_handoff_point(spx, a, where, k)
        a.set_algorithm(spx.ALGO_PRIMAL)
        _check_y_after_handoff(a, at)
        _to_handoff_point(spx, h, where, k)
        h.set_algorithm(spx.ALGO_PRIMAL)
        if where == "mid":
            st, piv = h.iterate(steps)
            assert piv == k + steps
        else:
            r = h.solve()
            piv = r.pivots
            assert r.status == spx.SolveStatus.OptimumFound and r.b_ixs.tolist() == want.b_ixs.tolist()
            assert abs(r.z - want.z) <= REL * abs(want.z) and abs(r.z - full.z) <= REL * abs(full.z)
        tp, tq = h.trace()
        s = h.state(binv=True)  # and y is still c_B B^-1 after the primal loop's own updates
        assert np.max(np.abs(s["y"] - s["c_B"] @ s["binv"])) <= 1e-9
    print(f"{where} -> primal: {piv - k} primal pivots after {k} (reference {want.pivots})")
    assert piv - k == want.pivots
    assert list(zip(tp.tolist()[k:], tq.tolist()[k:])) == want.trace


def test_cli_phase1(golden, tmp_path):
    """./solver --primal-box --phase1 --bounds FILE, and --phase1 alone."""
    m, n, seed = 7, 20, 0
    _, b, c, u, A = _lp(m, n, seed)
    g = golden["by_shape"][(m, n, seed)]
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
    r = subprocess.run([solver, "--primal-box", "--phase1", "--bounds", pb, "--json", "--no-iter-lines", p],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "Optimum found" in r.stdout
    js = json.loads(r.stdout.splitlines()[-1])
    assert js["status"] == 1 and js["pivots"] == g["ref_pivots"]
    assert abs(js["z"] - g["highs_z"]) <= REL * abs(g["highs_z"])
    assert (js["flip_passes"], js["to_upper"]) == (g["flips"], g["to_upper"])
    assert (js["phase1_passes"], js["phase1_pivots"], js["phase1_rows"]) == (g["p1_passes"], g["p1_pivots"], g["ninf0"])
    r = subprocess.run([solver, "--phase1", "--bounds", pb, p], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--phase1" in r.stderr and "--primal-box" in r.stderr
    r = subprocess.run([solver, "--primal-box", "--bounds", pb, p], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not primal feasible" in r.stderr
