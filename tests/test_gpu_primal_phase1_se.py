"""GPU: steepest-edge pricing through phase 1 of the bounded primal loop
(SPX_FLAG_PRIMAL_PHASE1_STEEPEST, spx_set_primal_phase_one_pricing; DESIGN.md
§7l) on the LPs of tests/primal_phase1_ref.py boxed_general(m, n, seed), whose
slack basis is neither primal nor dual feasible.

Golden values (tests/golden/primal_phase1_se_optima.json, written by
tests/golden/make_golden_primal_phase1_se.py): pivot count, the first 200 (p, q)
pairs, the final basis and at-upper set, the flip / to-upper counts and the
phase-1 pass / pivot / entry-row counts of the numpy restatement
tests/primal_phase1_se_ref.py, the recurrence's drift there, and HiGHS's
optimum.  A case is compared pass for pass only where the golden file marks it
`traced`: its smallest relative gap between the best and the second-best key of
either argmin, or between u_p and t_q, is >= 1e-6, so the pass sequence does not
depend on the fp64 summation order.  256 x 1024 is not (a pricing gap of 7.6e-7)
and is compared by optimum, certificate and pivot count against Dantzig's.

Weights against 1 + ||B^-1 A_j||^2 recomputed in numpy: within max(100 x the
restatement's recorded drift of the case, 1e-12), tests/test_gpu_primal_box_se.py's
convention; the drift is the golden file's, not a value of the code under test.

Shapes: 7 x 20 (one partial row block and column chunk of k_pbox_vtb / k_pbox_tau),
65 x 200 (two row blocks, the second with one row), 130 x 390 (three row blocks,
two column chunks, a pricing grid of more than one workgroup), 256 x 1024 and
1024 x 4096 (whole solves).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dual_ref
import primal_box_ref
import primal_box_se_ref
import primal_phase1_se_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "primal_phase1_se_optima.json")) as f:
        g = json.load(f)
    g["by_shape"] = {(c["m"], c["n"], c["seed"]): c for c in g["cases"]}
    return g


_LPS = {}


def _lp(m, n, seed):
    """(A_cols (n, m), b, c, u, A (m, n)) of boxed_general, built once."""
    k = (m, n, seed)
    if k not in _LPS:
        A, b, c, u = ref.boxed_general(m, n, seed)
        _LPS[k] = (np.ascontiguousarray(A.T), b, c, u, A)
    return _LPS[k]


def _ctx(spx, lp, **kw):
    At, b, c, u = lp[:4]
    kw.setdefault("trace", 200)
    kw.setdefault("primal_phase1", True)
    kw.setdefault("primal_pricing", spx.PRIMAL_PRICING_STEEPEST)
    kw.setdefault("primal_phase1_pricing", spx.PRIMAL_PRICING_STEEPEST)
    return spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, **kw)


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
    viol, dviol, zc = ref.certificate(A, b, c, u, r.b_ixs, up)  # primal_box_ref.certificate
    print(f"certificate: bound violation {viol:.2e}, reduced-cost sign violation {dviol:.2e}")
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= REL * abs(z)


def _counters(g):
    return (g["p1_passes"], g["p1_pivots"], g["ninf0"], 0)


def _solve(spx, lp, **kw):
    with _ctx(spx, lp, **kw) as ctx:
        cfg = ctx.config()
        assert cfg["primal_pricing"] == cfg["primal_phase1_pricing"] == spx.PRIMAL_PRICING_STEEPEST
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        return r, tp.tolist(), tq.tolist(), x, up, ctx.primal_flips(), ctx.primal_phase1()


def _check_against_golden(spx, g, lp, r, tp, tq, x, up, flips, ph):
    _, b, c, u, A = lp
    print(f"{g['m']}x{g['n']}: z={r.z:.13g} pivots={r.pivots} (golden {g['ref_pivots']}, Dantzig {g['dantzig_pivots']}) "
          f"flips={flips} (golden {g['flips']}, {g['to_upper']}) phase 1 {ph} (golden {_counters(g)})")
    assert g["traced"]
    assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
    k = min(g["ref_pivots"], 200)
    assert tp[:k] == g["ref_trace_p"][:k]
    assert tq[:k] == g["ref_trace_q"][:k]
    assert flips == (g["flips"], g["to_upper"]), flips
    assert ph == _counters(g), ph
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(up).tolist() == g["ref_at_upper"]
    _check_optimum(spx, r, x, up, A, b, c, u, g["highs_z"])


def _weight_error(A, b_ixs, w):
    """Largest relative difference between the non-basic entries of w and 1 +
    ||B^-1 A_j||^2 recomputed from the basis."""
    n = A.shape[1]
    basic = np.zeros(n, dtype=bool)
    basic[b_ixs] = True
    ex = primal_box_se_ref.exact_weights(A, np.linalg.inv(A[:, b_ixs]), basic)
    return float(np.max(np.abs(w[~basic] - ex[~basic]) / ex[~basic]))


@pytest.mark.parametrize("m,n,seed", [(7, 20, 0), (65, 200, 1), (130, 390, 2)])
def test_trace_parity(spx, golden, m, n, seed):
    lp = _lp(m, n, seed)
    _check_against_golden(spx, golden["by_shape"][(m, n, seed)], lp, *_solve(spx, lp))


@pytest.mark.parametrize("kw", [{"global_y": True}, {"price_grid": 3}, {"refactor_every": 50}],
                         ids=["global_y", "price_grid3", "refactor50"])
def test_variants_65(spx, golden, kw):
    """The vectors in global memory, a three-workgroup pricing grid and a
    reinversion every 50 pivots (the first lands inside phase 1, with a weight
    update pending: the rows are classified again and the update is not lost)
    walk the same passes with the same counters."""
    m, n, seed = 65, 200, 1
    g = golden["by_shape"][(m, n, seed)]
    assert g["p1_pivots"] > 50
    lp = _lp(m, n, seed)
    _check_against_golden(spx, g, lp, *_solve(spx, lp, **kw))


def test_lds_layouts_65(spx, golden, tmp_path):
    """SPX_PBOX_SE_LDS = 3, 1, 0 (k_pbox_price_se1<3> / <1> / <0>), each in a
    fresh process: the golden passes, and final states that are the same bits."""
    m, n, seed = 65, 200, 1
    g = golden["by_shape"][(m, n, seed)]
    got = {}
    for vecs in ("3", "1", "0"):
        out = str(tmp_path / f"lds{vecs}.npz")
        env = dict(os.environ, SPX_PBOX_SE_LDS=vecs)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "phase1_se_child.py"), out, str(m), str(n),
                            str(seed)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        d = dict(np.load(out))
        assert int(d["lds_vecs"]) == int(vecs)
        assert int(d["status"]) == int(spx.SolveStatus.OptimumFound) and int(d["pivots"]) == g["ref_pivots"]
        assert d["tp"].tolist()[:195] == g["ref_trace_p"][:195] and d["tq"].tolist()[:195] == g["ref_trace_q"][:195]
        assert d["b_ixs"].tolist() == g["ref_b_ixs"] and np.flatnonzero(d["up"]).tolist() == g["ref_at_upper"]
        assert tuple(d["flips"].tolist()) == (g["flips"], g["to_upper"]) and tuple(d["ph"].tolist()) == _counters(g)
        got[vecs] = d
    nb = np.ones(n, dtype=bool)
    nb[got["3"]["b_ixs"]] = False
    for vecs in ("1", "0"):
        for k in ("x_b", "y", "binv", "z"):
            assert np.array_equal(got["3"][k], got[vecs][k]), (vecs, k)
        assert np.array_equal(got["3"]["w"][nb], got[vecs]["w"][nb]), vecs


def test_whole_solve_256(spx, golden):
    """Not traced (a pricing gap below 1e-6): the optimum to 1e-9 relative, a
    clean certificate, and fewer pivots than Dantzig's 17,473."""
    m, n, seed = 256, 1024, 3
    lp = _lp(m, n, seed)
    g = golden["by_shape"][(m, n, seed)]
    assert not g["traced"] and g["dantzig_pivots"] == 17473
    r, tp, tq, x, up, flips, ph = _solve(spx, lp)
    print(f"{m}x{n}: z={r.z:.13g} (HiGHS {g['highs_z']:.13g}) pivots={r.pivots} (restatement {g['ref_pivots']}, Dantzig "
          f"{g['dantzig_pivots']}) flips={flips} phase 1 {ph} (restatement {_counters(g)})")
    _, b, c, u, A = lp
    _check_optimum(spx, r, x, up, A, b, c, u, g["highs_z"])
    assert r.pivots < g["dantzig_pivots"]
    assert ph[2] == g["ninf0"] and ph[3] == 0 and 0 < ph[1] <= ph[0]


def test_certificate_1024(spx, golden):
    m, n, seed = 1024, 4096, 4
    lp = _lp(m, n, seed)
    g = golden["by_shape"][(m, n, seed)]
    assert g["traced"]
    with _ctx(spx, lp, trace=0) as ctx:
        r = ctx.solve()
        x, up = ctx.primal()
        flips, ph = ctx.primal_flips(), ctx.primal_phase1()
    print(f"{m}x{n}: z={r.z:.13g} (HiGHS {g['highs_z']:.13g}) pivots={r.pivots} (golden {g['ref_pivots']}) flips={flips} "
          f"(golden {g['flips']}, {g['to_upper']}) phase 1 {ph} (golden {_counters(g)})")
    assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
    assert ph == _counters(g), ph
    assert flips == (g["flips"], g["to_upper"]), flips
    assert len(set(r.b_ixs.tolist())) == m
    _, b, c, u, A = lp
    _check_optimum(spx, r, x, up, A, b, c, u, g["highs_z"])


def test_single_steps_130(spx, golden):
    """iterate(1) forty times, weight readbacks in between (each applies the
    pending update outside a pass), against one iterate(40): the same trace,
    x_b, B^-1 and weights bit for bit; all forty pivots are phase-1 pivots."""
    m, n, seed = 130, 390, 2
    lp = _lp(m, n, seed)
    g = golden["by_shape"][(m, n, seed)]
    assert g["p1_pivots"] > 40
    with _ctx(spx, lp) as a, _ctx(spx, lp) as b:
        for i in range(40):
            st, piv = a.iterate(1)
            assert piv == i + 1 and st == spx.SolveStatus.MaxIter, (i, piv, st)
            if i % 8 == 3:
                a.primal_weights()
        st, piv = b.iterate(40)
        assert piv == 40
        pa, pb = a.primal_phase1(), b.primal_phase1()
        assert pa == pb and pa[1] == 40 and pa[3] > 0, (pa, pb)  # inside phase 1
        ta, tb = a.trace(), b.trace()
        assert ta[0].tolist() == tb[0].tolist() == g["ref_trace_p"][:40]
        assert ta[1].tolist() == tb[1].tolist() == g["ref_trace_q"][:40]
        wa, wb = a.primal_weights(), b.primal_weights()
        sa, sb = a.state(binv=True), b.state(binv=True)
        assert sa["b_ixs"].tolist() == sb["b_ixs"].tolist()
        for k in ("x_b", "c_B", "binv"):
            assert np.array_equal(sa[k], sb[k]), k
        nb = np.ones(n, dtype=bool)
        nb[sa["b_ixs"]] = False
        assert np.array_equal(wa[nb], wb[nb])
        assert np.array_equal(a.primal_weights()[nb], wa[nb])  # a second readback applies nothing
        assert np.array_equal(a.primal()[1], b.primal()[1]) and a.primal_flips() == b.primal_flips()
        ra, rb = a.solve(), b.solve()  # and both go on to the golden end
        assert ra.pivots == rb.pivots == g["ref_pivots"] and ra.z == rb.z
        assert a.primal_phase1() == b.primal_phase1() == _counters(g)


def test_weights_and_y_130(spx, golden):
    """Half-way through phase 1: the weights against 1 + ||B^-1 A_j||^2
    recomputed from the basis, and y = c_B B^-1 although phase 1 does not
    maintain it; the weights again at the optimum (the switch kept them)."""
    m, n, seed = 130, 390, 2
    lp = _lp(m, n, seed)
    A = lp[4]
    g = golden["by_shape"][(m, n, seed)]
    tol = max(100.0 * max(g["drift_enter"], g["drift_final"]), 1e-12)
    k = g["p1_pivots"] // 2
    with _ctx(spx, lp) as ctx:
        w0 = ctx.primal_weights()
        assert np.allclose(w0, primal_box_se_ref.reference_weights(A), rtol=1e-13, atol=0.0)  # exact at the slack basis
        st, piv = ctx.iterate(k)
        ph = ctx.primal_phase1()
        assert piv == k and ph[1] == k and ph[3] > 0, (piv, ph)
        w = ctx.primal_weights()
        s = ctx.state(binv=True)
        emid = _weight_error(A, s["b_ixs"], w)
        want = s["c_B"] @ s["binv"]
        ey = float(np.max(np.abs(s["y"] - want)))
        assert np.any(s["c_B"] != 0.0)
        r = ctx.solve()
        tp, tq = ctx.trace()
        wo = ctx.primal_weights()
        eopt = _weight_error(A, r.b_ixs, wo)
        ph = ctx.primal_phase1()
    print(f"weights against exact: {emid:.2e} after {k} phase-1 pivots, {eopt:.2e} at the optimum (tolerance {tol:.2e}, "
          f"restatement drift {g['drift_enter']:.2e} / {g['drift_final']:.2e}); y against c_B B^-1: {ey:.2e}")
    assert emid <= tol and eopt <= tol, (emid, eopt, tol)
    assert ey <= 1e-10, ey
    # the readbacks in the middle changed no pass
    assert r.pivots == g["ref_pivots"] and ph == _counters(g)
    assert tp.tolist()[:200] == g["ref_trace_p"][:200] and tq.tolist()[:200] == g["ref_trace_q"][:200]


def test_infeasible(spx, golden):
    A, b, c, u = ref.tiny_infeasible()
    with _ctx(spx, (np.ascontiguousarray(A.T), b, c, u)) as ctx:
        r = ctx.solve()
        assert r.status == spx.SolveStatus.Infeasible and r.pivots == golden["tiny_infeasible"]["ref_pivots"] == 0
        assert ctx.primal_phase1() == (0, 0, 1, 1)
    g = golden["infeasible"]
    m, n, seed = g["m"], g["n"], g["seed"]
    _, b, c, u, A = _lp(m, n, seed)
    A2, b2, u2 = ref.contradict(A, b, u)
    assert g["traced"]
    with _ctx(spx, (np.ascontiguousarray(A2.T), b2, c, u2)) as ctx:
        r = ctx.solve()
        ph = ctx.primal_phase1()
        print(f"contradictory rows: status {r.status} after {r.pivots} pivots (golden {g['ref_pivots']}, Dantzig "
              f"{g['dantzig_pivots']}), phase 1 {ph}")
        assert r.status == spx.SolveStatus.Infeasible
        assert r.pivots == g["ref_pivots"]
        assert ph == (g["p1_passes"], g["p1_pivots"], g["ninf0"], g["ninf_end"])
        assert ctx.primal_flips() == (g["flips"], g["to_upper"])
        # the context stays usable: a feasible right-hand side, the weights kept
        b3 = b2.copy()
        b3[0], b3[1] = g["feasible_b01"]
        ctx.set_rhs(b3)
        r = ctx.solve()
        x, up = ctx.primal()
        _check_optimum(spx, r, x, up, A2, b3, c, u2, g["feasible_highs_z"])


def test_stuck_warm_start(spx, golden):
    """An optimal basis after set_cost and set_rhs together is neither primal nor
    dual feasible; both calls keep the weights of the first solve, and phase 1
    under steepest edge solves from there in the restatement's pivots."""
    g = golden["stuck"]
    assert g["traced"]
    m, n, seed = g["m"], g["n"], g["seed"]
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    c2 = primal_box_ref.cost_variant(c, n - m, seed)
    b2 = ref.rhs_variant(b, seed)
    with _ctx(spx, (np.ascontiguousarray(A.T), b, c, u)) as ctx:
        r0 = ctx.solve()
        assert r0.status == spx.SolveStatus.OptimumFound and r0.pivots == g["first_pivots"]
        assert ctx.primal_phase1() == (0, 0, 0, 0)  # a feasible entry: the plain steepest-edge passes
        ctx.set_cost(c2)
        ctx.set_rhs(b2)
        r = ctx.solve()
        x, up = ctx.primal()
        ph = ctx.primal_phase1()
        flips = ctx.primal_flips()
    print(f"stuck warm start: {r.pivots - r0.pivots} pivots (golden {g['ref_pivots']}, Dantzig {g['dantzig_pivots']}), "
          f"phase 1 {ph} (golden {_counters(g)}), z={r.z:.13g} (HiGHS {g['highs_z']:.13g})")
    assert r.pivots - r0.pivots == g["ref_pivots"], (r.pivots - r0.pivots, g["ref_pivots"])
    assert ph == _counters(g), ph
    _check_optimum(spx, r, x, up, A, b2, c2, u, g["highs_z"])


def _trace_of(ctx):
    r = ctx.solve()
    tp, tq = ctx.trace()
    return r.pivots, tp.tolist(), tq.tolist(), ctx.primal_phase1()


def test_setter_orders(spx, golden):
    m, n, seed = 65, 200, 1
    lp = _lp(m, n, seed)
    g = golden["by_shape"][(m, n, seed)]
    S, D = spx.PRIMAL_PRICING_STEEPEST, spx.PRIMAL_PRICING_DANTZIG
    want = (g["ref_pivots"], g["ref_trace_p"], g["ref_trace_q"], _counters(g))

    def reached(ctx):
        piv, tp, tq, ph = _trace_of(ctx)
        return (piv, tp[:200], tq[:200], ph) == (want[0], want[1][:200], want[2][:200], want[3])

    # accepted: the three flags at create, and every order of the setters that names phase 1's rule first
    with _ctx(spx, lp) as ctx:
        assert reached(ctx)
    plain = dict(primal_phase1=False, primal_pricing=D, primal_phase1_pricing=D)
    with _ctx(spx, lp, **plain) as ctx:
        ctx.set_primal_phase1_pricing(S)  # inert so far
        ctx.set_primal_phase1(True)
        ctx.set_primal_pricing(S)
        assert reached(ctx)
    with _ctx(spx, lp, **plain) as ctx:
        ctx.set_primal_phase1_pricing(S)
        ctx.set_primal_pricing(S)
        ctx.set_primal_phase1(True)
        assert reached(ctx)
    with _ctx(spx, lp, primal_pricing=D) as ctx:  # phase 1 and its rule at create (the rule inert), the loop's rule later
        ctx.set_primal_pricing(S)
        assert reached(ctx)
    with _ctx(spx, lp, primal_phase1=False) as ctx:
        ctx.set_primal_phase1(True)
        assert reached(ctx)
    # refused, by name, and nothing changed
    with _ctx(spx, lp) as ctx:
        before = ctx.config()
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_phase1_pricing(D)
        assert ei.value.code == -5 and "spx_set_primal_phase_one_pricing" in str(ei.value)
        assert "phase 1" in str(ei.value) and "steepest" in str(ei.value)
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_phase1_pricing(7)
        assert ei.value.code == -1 and "rule" in str(ei.value)
        assert ctx.config() == before
        assert reached(ctx)
        ctx.set_primal_phase1(False)  # with phase 1 off the setting is inert again: accepted
        ctx.set_primal_phase1_pricing(D)
        with pytest.raises(spx.SimplexError) as ei:  # ... and the default refusal is back
            ctx.set_primal_phase1(True)
        assert ei.value.code == -5 and "steepest" in str(ei.value)
        assert ctx.config()["primal_phase1_pricing"] == D
    with _ctx(spx, lp, primal_pricing=D, primal_phase1_pricing=D) as ctx:
        before = ctx.config()
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_pricing(S)
        assert ei.value.code == -5 and "phase 1" in str(ei.value)
        assert ctx.config() == before
    # free columns stay refused under steepest edge
    lo = np.zeros(n)
    lo[0] = -np.inf
    with _ctx(spx, lp) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_bounds_lu(lo, lp[3])
        assert ei.value.code == -5 and "free columns" in str(ei.value)


def test_default_still_refuses(spx):
    """With the new setting at its default the combination is refused with the
    message it always had, at create and in both setters."""
    lp = _lp(7, 20, 0)
    D = spx.PRIMAL_PRICING_DANTZIG
    with pytest.raises(spx.SimplexError) as ei:
        _ctx(spx, lp, primal_phase1_pricing=D)
    assert ei.value.code == -1
    assert ("SPX_FLAG_PRIMAL_STEEPEST with SPX_FLAG_PRIMAL_PHASE1: steepest-edge pricing does not run during the bounded "
            "primal loop's phase 1") in str(ei.value)
    with _ctx(spx, lp, primal_phase1=False, primal_phase1_pricing=D) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_phase1(True)
        assert ei.value.code == -5 and "set SPX_PRIMAL_PRICING_DANTZIG first" in str(ei.value)
    with _ctx(spx, lp, primal_pricing=D, primal_phase1_pricing=D) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_pricing(spx.PRIMAL_PRICING_STEEPEST)
        assert ei.value.code == -5 and "switch phase 1 off first" in str(ei.value)


def test_cli(golden, tmp_path):
    """./solver --primal-box --phase1 --primal-pricing steepest --phase1-pricing steepest."""
    m, n, seed = 65, 200, 1
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
    base = [solver, "--primal-box", "--phase1", "--bounds", pb, "--primal-pricing", "steepest"]
    r = subprocess.run(base + ["--phase1-pricing", "steepest", "--json", "--no-iter-lines", p], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "Optimum found" in r.stdout
    js = json.loads(r.stdout.splitlines()[-1])
    assert js["status"] == 1 and js["pivots"] == g["ref_pivots"]
    assert abs(js["z"] - g["highs_z"]) <= REL * abs(g["highs_z"])
    assert (js["flip_passes"], js["to_upper"]) == (g["flips"], g["to_upper"])
    assert (js["phase1_passes"], js["phase1_pivots"], js["phase1_rows"]) == (g["p1_passes"], g["p1_pivots"], g["ninf0"])
    r = subprocess.run(base + [p], capture_output=True, text=True, timeout=120)  # without it: today's refusal
    assert r.returncode == 1 and "SPX_FLAG_PRIMAL_STEEPEST with SPX_FLAG_PRIMAL_PHASE1" in r.stderr
