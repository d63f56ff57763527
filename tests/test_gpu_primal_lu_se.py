"""GPU: steepest-edge pricing with free columns in the bounded primal loop
(SPX_FLAG_PRIMAL_FREE_STEEPEST, spx_set_primal_free_pricing; k_pbox_price_se_f,
k_pbox_step_se_f) on two families of LPs with a fifth of the
structural columns free: tests/primal_lu_ref.py general_lu(m, n, seed), whose
slack basis is infeasible on both sides (phase 1, then phase 2), and
tests/primal_lu_se_ref.py free_feasible(m, n, seed), whose slack basis is feasible
(phase 1 off: the phase word stays 0).

Golden values (tests/golden/primal_lu_se_optima.json, written by
tests/golden/make_golden_primal_lu_se.py): pivot count, the first 200 (p, q)
pairs, the final basis and at-upper set, the flip / to-upper counts and the
phase-1 counters of the numpy restatement tests/primal_lu_se_ref.py, its drift,
and HiGHS's optimum with bounds=list(zip(l, u)).  The generator refuses a case
whose smallest relative gap between the best and the second-best key of either
argmin, or between u_p and t_q, is below 1e-6 (the smallest over the committed
cases is 1.4e-5), so pass-for-pass equality does not depend on the fp64
summation order.

Weights against 1 + ||B^-1 A_j||^2 recomputed in numpy: within max(100 x the
restatement's recorded drift of the case, 1e-12), tests/test_gpu_primal_phase1_se.py's
convention; the drift is the golden file's, not a value of the code under test.
Weights restarted exactly (k_pbox_wexact) against numpy: the a-priori bound of
tests/test_gpu_primal_box_wexact.py, 8 m 2^-53 (1 + || |S| |A_j| ||^2) absolute.

Shapes: 7 x 20 (one partial row block and column chunk), 65 x 200 (two row blocks
of k_pbox_vtb / k_pbox_tau, the second with one row), 130 x 390 (three row blocks,
two column chunks, a pricing grid of more than one workgroup), 256 x 1024 (whole
solve).
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
import primal_lu_se_ref as ref
import test_gpu_ranging as ranging_checks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9
KINDS = ("general", "feasible")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "primal_lu_se_optima.json")) as f:
        g = json.load(f)
    g["by_shape"] = {(k, c["m"], c["n"], c["seed"]): c for k in KINDS for c in g[k]}
    return g


_LPS = {}


def _lp(kind, m, n, seed):
    """(A_cols (n, m), b, c, l, u, A (m, n)), built once."""
    k = (kind, m, n, seed)
    if k not in _LPS:
        A, b, c, l, u = (ref.general_lu if kind == "general" else ref.free_feasible)(m, n, seed)
        _LPS[k] = (np.ascontiguousarray(A.T), b, c, l, u, A)
    return _LPS[k]


def _ctx(spx, lp, phase1, **kw):
    At, b, c, l, u = lp[:5]
    S = spx.PRIMAL_PRICING_STEEPEST
    kw.setdefault("trace", 200)
    kw.setdefault("primal_pricing", S)
    kw.setdefault("primal_phase1_pricing", S)
    kw.setdefault("primal_free_pricing", S)
    return spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, lower=l, upper=u, primal_phase1=phase1, **kw)


def _check_primal(x, up, b_ixs, A, b, l, u):
    res = float(np.max(np.abs(A @ x - b)))
    assert res <= 1e-9 * max(1.0, np.max(np.abs(b))), res
    assert np.max(l - x) <= 1e-9 and np.max(x - u) <= 1e-9, (np.max(l - x), np.max(x - u))
    nb = np.ones(len(x), dtype=bool)
    nb[b_ixs] = False
    want = np.where(up, u, np.where(np.isneginf(l), 0.0, l))
    assert np.array_equal(x[nb], want[nb])  # exactly l_j or u_j (0 for a free column)
    assert not np.any(up & ~nb) and not np.any(up & ~np.isfinite(u))


def _check_optimum(spx, r, x, up, A, b, c, l, u, z):
    """tests/test_gpu_primal_lu.py's: certificate_lu plus HiGHS's z within 1e-9 relative."""
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    _check_primal(x, up, r.b_ixs, A, b, l, u)
    assert abs(float(c @ x) - r.z) <= REL * abs(z), (float(c @ x), r.z)
    assert np.array_equal(x[r.b_ixs], r.x_b)
    viol, dviol, zc = ref.certificate_lu(A, b, c, l, u, r.b_ixs, up)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= REL * abs(z)


def _counters(g):
    return (g["p1_passes"], g["p1_pivots"], g["ninf0"], 0)


def _solve(spx, lp, phase1, **kw):
    with _ctx(spx, lp, phase1, **kw) as ctx:
        cfg = ctx.config()
        assert cfg["primal_pricing"] == cfg["primal_free_pricing"] == spx.PRIMAL_PRICING_STEEPEST
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        return r, tp.tolist(), tq.tolist(), x, up, ctx.primal_flips(), ctx.primal_phase1()


def _check_against_golden(spx, g, lp, r, tp, tq, x, up, flips, ph):
    _, b, c, l, u, A = lp
    print(f"{g['m']}x{g['n']}: z={r.z:.13g} pivots={r.pivots} (golden {g['ref_pivots']}, Dantzig {g['dantzig_pivots']}) "
          f"flips={flips} (golden {g['flips']}, {g['to_upper']}) phase 1 {ph} (golden {_counters(g)})")
    assert g["free_entered"] > 0 and g["free_basic"] > 0 and g["ref_pivots"] < g["dantzig_pivots"]
    assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
    k = min(g["ref_pivots"], 200)
    assert tp[:k] == g["ref_trace_p"][:k]
    assert tq[:k] == g["ref_trace_q"][:k]
    assert flips == (g["flips"], g["to_upper"]), flips
    assert ph == _counters(g), ph
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(up).tolist() == g["ref_at_upper"]
    assert np.count_nonzero(np.isneginf(l)[r.b_ixs]) == g["free_basic"]
    _check_optimum(spx, r, x, up, A, b, c, l, u, g["highs_z"])


def _weight_error(A, b_ixs, w):
    """Largest relative difference between the non-basic entries of w and 1 +
    ||B^-1 A_j||^2 recomputed from the basis."""
    n = A.shape[1]
    basic = np.zeros(n, dtype=bool)
    basic[b_ixs] = True
    ex = primal_box_se_ref.exact_weights(A, np.linalg.inv(A[:, b_ixs]), basic)
    return float(np.max(np.abs(w[~basic] - ex[~basic]) / ex[~basic]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n,seed", [(7, 20, 0), (65, 200, 1), (130, 390, 2)])
def test_trace_parity(spx, golden, kind, m, n, seed):
    """Through phase 1 (`general`: vtb -> price_se_f -> update_f -> step_se_f ->
    tau) and with phase 1 off (`feasible`: the same pass without vtb)."""
    lp = _lp(kind, m, n, seed)
    g = golden["by_shape"][(kind, m, n, seed)]
    assert (g["p1_pivots"] > 0) == (kind == "general")
    _check_against_golden(spx, g, lp, *_solve(spx, lp, kind == "general"))


LAYOUTS = [("lds3", {"SPX_PBOX_SE_LDS": "3"}, []), ("lds1", {"SPX_PBOX_SE_LDS": "1"}, []),
           ("lds0", {"SPX_PBOX_SE_LDS": "0"}, []), ("global_y", {}, ["global_y"]),
           ("price_grid3", {}, ["price_grid=3"]), ("refactor50", {}, ["refactor_every=50"])]


def _child(tmp_path, name, env, extra, kind, m, n, seed, k):
    out = str(tmp_path / f"{name}_{kind}_{k}.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lu_se_child.py"), out, kind, str(m), str(n),
                        str(seed), str(k)] + extra, env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    return dict(np.load(out))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,env,extra", LAYOUTS, ids=[v[0] for v in LAYOUTS])
def test_layouts_65(spx, golden, tmp_path, kind, name, env, extra):
    """k_pbox_price_se_f<3> / <1> / <0> (SPX_PBOX_SE_LDS), the vectors in global
    memory, a three-workgroup pricing grid and a reinversion every 50 pivots
    (`general`: the first lands inside phase 1 with a weight update pending; the
    rows are classified again by k_pbox_classify_f and the update is not lost),
    each in a fresh process: the golden passes, counters and final basis."""
    m, n, seed = 65, 200, 1
    g = golden["by_shape"][(kind, m, n, seed)]
    if kind == "general":
        assert g["p1_pivots"] > 50
    d = _child(tmp_path, name, env, extra, kind, m, n, seed, 0)
    if "SPX_PBOX_SE_LDS" in env:
        assert int(d["lds_vecs"]) == int(env["SPX_PBOX_SE_LDS"])
    if name == "global_y":
        assert int(d["lds_vecs"]) == 0
    if name == "price_grid3":
        assert int(d["price_grid"]) == 3
    assert int(d["status"]) == int(spx.SolveStatus.OptimumFound) and int(d["pivots"]) == g["ref_pivots"]
    k = min(g["ref_pivots"], 200)
    assert d["tp"].tolist()[:k] == g["ref_trace_p"][:k] and d["tq"].tolist()[:k] == g["ref_trace_q"][:k]
    assert d["b_ixs"].tolist() == g["ref_b_ixs"] and np.flatnonzero(d["up"]).tolist() == g["ref_at_upper"]
    assert tuple(d["flips"].tolist()) == (g["flips"], g["to_upper"]) and tuple(d["ph"].tolist()) == _counters(g)
    assert abs(float(d["z"]) - g["highs_z"]) <= REL * abs(g["highs_z"])


@pytest.mark.parametrize("kind", KINDS)
def test_bitwise_across_layouts_65(spx, golden, tmp_path, kind):
    """After 40 pivots (`general`: all inside phase 1) x_b, B^-1 and the weights
    are the same bits with all three vectors in LDS on the default grid, and with
    none of them there on a three-workgroup grid: a column's d_j and gamma_j do
    not depend on NL, on the grid or on the wave that prices it."""
    m, n, seed = 65, 200, 1
    g = golden["by_shape"][(kind, m, n, seed)]
    a = _child(tmp_path, "a", {"SPX_PBOX_SE_LDS": "3"}, [], kind, m, n, seed, 40)
    b = _child(tmp_path, "b", {"SPX_PBOX_SE_LDS": "0"}, ["price_grid=3"], kind, m, n, seed, 40)
    assert int(a["lds_vecs"]) == 3 and int(b["lds_vecs"]) == 0 and int(b["price_grid"]) == 3 != int(a["price_grid"])
    assert int(a["pivots"]) == int(b["pivots"]) == 40
    if kind == "general":
        assert g["p1_pivots"] > 40 and a["ph"][1] == 40 and a["ph"][3] > 0
    assert a["tp"].tolist() == b["tp"].tolist() == g["ref_trace_p"][:40]
    assert a["tq"].tolist() == b["tq"].tolist() == g["ref_trace_q"][:40]
    assert a["b_ixs"].tolist() == b["b_ixs"].tolist()
    nb = np.ones(n, dtype=bool)
    nb[a["b_ixs"]] = False
    for k in ("x_b", "binv", "x"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["w"][nb], b["w"][nb])


@pytest.mark.parametrize("kind", KINDS)
def test_whole_solve_256(spx, golden, kind):
    m, n, seed = 256, 1024, 3
    lp = _lp(kind, m, n, seed)
    g = golden["by_shape"][(kind, m, n, seed)]
    r, tp, tq, x, up, flips, ph = _solve(spx, lp, kind == "general")
    print(f"{kind} {m}x{n}: z={r.z:.13g} (HiGHS {g['highs_z']:.13g}) pivots={r.pivots} (golden {g['ref_pivots']}, Dantzig "
          f"{g['dantzig_pivots']}) flips={flips} phase 1 {ph} (golden {_counters(g)})")
    _, b, c, l, u, A = lp
    _check_optimum(spx, r, x, up, A, b, c, l, u, g["highs_z"])
    assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])


@pytest.mark.parametrize("kind", KINDS)
def test_weights_130(spx, golden, kind):
    """Exact at the slack basis, then half-way (`general`: half-way through
    phase 1) and at the optimum against 1 + ||B^-1 A_j||^2 from the basis."""
    m, n, seed = 130, 390, 2
    lp = _lp(kind, m, n, seed)
    A = lp[5]
    g = golden["by_shape"][(kind, m, n, seed)]
    tol = max(100.0 * max(g["drift_enter"], g["drift_final"]), 1e-12)
    k = (g["p1_pivots"] if kind == "general" else g["ref_pivots"]) // 2
    with _ctx(spx, lp, kind == "general") as ctx:
        w0 = ctx.primal_weights()
        assert np.allclose(w0, primal_box_se_ref.reference_weights(A), rtol=1e-13, atol=0.0)  # exact at the slack basis
        st, piv = ctx.iterate(k)
        ph = ctx.primal_phase1()
        assert piv == k and (kind != "general" or (ph[1] == k and ph[3] > 0)), (piv, ph)
        s = ctx.state(binv=True)
        emid = _weight_error(A, s["b_ixs"], ctx.primal_weights())
        r = ctx.solve()
        tp, tq = ctx.trace()
        eopt = _weight_error(A, r.b_ixs, ctx.primal_weights())
        ph = ctx.primal_phase1()
    print(f"{kind}: weights against exact: {emid:.2e} after {k} pivots, {eopt:.2e} at the optimum (tolerance {tol:.2e}, "
          f"restatement drift {g['drift_enter']:.2e} / {g['drift_final']:.2e})")
    assert emid <= tol and eopt <= tol, (emid, eopt, tol)
    # the readbacks in the middle changed no pass
    assert r.pivots == g["ref_pivots"] and ph == _counters(g)
    assert tp.tolist()[:200] == g["ref_trace_p"][:200] and tq.tolist()[:200] == g["ref_trace_q"][:200]


def test_warm_start_exact_weights(spx):
    """free_feasible at 65 x 200 solved under Dantzig (the *_f kernels), a new
    cost on that basis, which holds free columns, then steepest edge with the
    weights restarted exactly: they are 1 + ||B^-1 A_j||^2 at entry, and the
    re-solve walks the restatement's passes from that basis with those weights."""
    m, n, seed = 65, 200, 1
    lp = _lp("feasible", m, n, seed)
    _, b, c, l, u, A = lp
    c2 = primal_box_ref.cost_variant(c, n - m, seed)
    S, D = spx.PRIMAL_PRICING_STEEPEST, spx.PRIMAL_PRICING_DANTZIG
    with _ctx(spx, lp, False, primal_pricing=D, primal_weights=spx.PRIMAL_WEIGHTS_EXACT, trace=4096) as ctx:
        r0 = ctx.solve()
        assert r0.status == spx.SolveStatus.OptimumFound
        _, up0 = ctx.primal()
        assert np.count_nonzero(np.isneginf(l)[r0.b_ixs]) > 0  # free columns in the warm basis
        ctx.set_cost(c2)
        ctx.set_primal_pricing(S)
        w = ctx.primal_weights()
        s = ctx.state(binv=True)
        assert s["b_ixs"].tolist() == r0.b_ixs.tolist()
        nb = np.ones(n, dtype=bool)
        nb[s["b_ixs"]] = False
        V = s["binv"] @ A[:, nb]
        bound = 8.0 * m * 2.0 ** -53 * (1.0 + np.einsum("ij,ij->j", np.abs(s["binv"]) @ np.abs(A[:, nb]),
                                                           np.abs(s["binv"]) @ np.abs(A[:, nb])))
        err = np.abs(w[nb] - (1.0 + np.einsum("ij,ij->j", V, V)))
        print(f"exact weights at entry: worst error / bound = {float(np.max(err / bound)):.3g}")
        assert np.all(err <= bound)
        w_in = np.where(nb, w, 2.0)  # (a basic column's entry is unspecified on the device; exact_weights' filler)
        want = ref.primal_simplex_lu_se(A, b, c2, l, u, basis=r0.b_ixs, at_upper=up0, weights=w_in, trace_cap=4096)
        assert want.status == dual_ref.OPTIMUM and min(want.gap_price, want.gap_ratio, want.gap_flip) >= 1e-6
        f0 = ctx.primal_flips()
        r = ctx.solve()
        x, up = ctx.primal()
        tp, tq = ctx.trace()
        f1 = ctx.primal_flips()
    print(f"warm start: Dantzig {r0.pivots} pivots, then {r.pivots - r0.pivots} under steepest edge (restatement "
          f"{want.pivots}), z={r.z:.13g} (restatement {want.z:.13g})")
    assert want.pivots > 0 and r.pivots - r0.pivots == want.pivots
    assert list(zip(tp.tolist()[r0.pivots:], tq.tolist()[r0.pivots:])) == [(int(p), int(q)) for p, q in want.trace]
    assert (f1[0] - f0[0], f1[1] - f0[1]) == (want.flips, want.to_upper)
    assert r.b_ixs.tolist() == want.b_ixs.tolist() and np.array_equal(up, want.at_upper)
    _check_optimum(spx, r, x, up, A, b, c2, l, u, want.z)


def test_exact_tie(spx):
    """The 7 x 20 free_feasible LP with free column 2 duplicated in position 3:
    whenever both are candidates their d_j and gamma_j, so their keys, are the
    same bits, and the smaller index enters, as in the restatement."""
    A, b, c, l, u = ref.free_tie()
    want = ref.primal_simplex_lu_se(A, b, c, l, u)
    assert want.status == dual_ref.OPTIMUM and want.ties["free_price"] > 0 and want.gap_price == 0.0
    assert 2 in [p for p, _ in want.trace] and 3 not in [p for p, _ in want.trace]
    lp = (np.ascontiguousarray(A.T), b, c, l, u, A)
    with _ctx(spx, lp, False) as ctx:
        w0 = ctx.primal_weights()
        assert w0[2] == w0[3]
        k = [p for p, _ in want.trace].index(2)
        ctx.iterate(k)  # the pass in front of the tie: the recurrence has kept the two weights equal
        w = ctx.primal_weights()
        assert w[2] == w[3] and w[2] != w0[2]
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
    assert r.pivots == want.pivots and list(zip(tp.tolist(), tq.tolist())) == [(int(p), int(q)) for p, q in want.trace]
    assert r.b_ixs.tolist() == want.b_ixs.tolist() and np.array_equal(up, want.at_upper)
    _check_optimum(spx, r, x, up, A, b, c, l, u, want.z)


def test_unbounded(spx):
    """tiny_unbounded_free: x0 free falls without a bound.  Column 0 is the LP's
    only non-basic column, so it is the restatement's ray column and the device's."""
    A, b, c, l, u = ref.tiny_unbounded_free()
    want = ref.primal_simplex_lu_se(A, b, c, l, u)
    assert want.status == primal_box_ref.UNBOUNDED and want.ray_col == 0 and want.pivots == 0
    lp = (np.ascontiguousarray(A.T), b, c, l, u, A)
    for phase1 in (False, True):
        with _ctx(spx, lp, phase1) as ctx:
            r = ctx.solve()
            assert r.status == spx.SolveStatus.Unbounded and r.pivots == 0, r
            assert r.b_ixs.tolist() == [1] and ctx.primal_flips() == (0, 0)
            # bounded from below it stops there: x0 = -3, the slack 4, z = 3
            ctx.set_bounds_lu(np.array([-3.0, 0.0]), u)
            r = ctx.solve()
            x, up = ctx.primal()
            assert r.status == spx.SolveStatus.OptimumFound and r.z == 3.0 and x.tolist() == [-3.0, 4.0], (r, x)


def test_setter_orders(spx, golden):
    kind, m, n, seed = "feasible", 65, 200, 1
    lp = _lp(kind, m, n, seed)
    At, b, c, l, u, A = lp
    g = golden["by_shape"][(kind, m, n, seed)]
    gg = golden["by_shape"][("general", m, n, seed)]
    glp = _lp("general", m, n, seed)
    S, D = spx.PRIMAL_PRICING_STEEPEST, spx.PRIMAL_PRICING_DANTZIG

    def reached(ctx, g):
        r = ctx.solve()
        tp, tq = ctx.trace()
        k = min(g["ref_pivots"], 200)
        return (r.status == spx.SolveStatus.OptimumFound and r.pivots == g["ref_pivots"]
                and tp.tolist()[:k] == g["ref_trace_p"][:k] and tq.tolist()[:k] == g["ref_trace_q"][:k]
                and ctx.primal_phase1() == _counters(g))

    def plain(lp, **kw):
        return spx.Context(lp[0], lp[1], lp[2], algorithm=spx.ALGO_PRIMAL_BOX, trace=200, **kw)

    # accepted: the flags at create; the free rule first, then bounds and the loop's rule in either order
    with _ctx(spx, lp, False) as ctx:
        assert reached(ctx, g)
    with plain(lp) as ctx:
        assert ctx.config()["primal_free_pricing"] == D
        ctx.set_primal_free_pricing(S)  # inert so far
        ctx.set_primal_pricing(S)
        ctx.set_bounds_lu(l, u)  # free columns under steepest edge
        assert ctx.config()["primal_free_pricing"] == S
        assert reached(ctx, g)
    with plain(lp) as ctx:
        ctx.set_bounds_lu(l, u)
        ctx.set_primal_free_pricing(S)
        ctx.set_primal_pricing(S)  # steepest edge on a context that holds free columns
        assert reached(ctx, g)
    # with phase 1 on, phase 1's own opt-in is still required and still refuses as it does
    with plain(glp, primal_phase1=True, primal_free_pricing=S) as ctx:
        ctx.set_bounds_lu(glp[3], glp[4])
        before = ctx.config()
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_pricing(S)
        assert ei.value.code == -5 and "switch phase 1 off first" in str(ei.value)
        assert ctx.config() == before
        ctx.set_primal_phase1_pricing(S)
        ctx.set_primal_pricing(S)
        assert reached(ctx, gg)
    with pytest.raises(spx.SimplexError) as ei:
        _ctx(spx, glp, True, primal_phase1_pricing=D)
    assert ei.value.code == -1 and "SPX_FLAG_PRIMAL_STEEPEST with SPX_FLAG_PRIMAL_PHASE1" in str(ei.value)
    # refused by name, and nothing changed: back to DANTZIG while the context holds a free column under steepest edge
    with _ctx(spx, lp, False) as ctx:
        before = ctx.config()
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_free_pricing(D)
        assert ei.value.code == -5 and "spx_set_primal_free_pricing" in str(ei.value)
        assert "free columns" in str(ei.value) and "steepest" in str(ei.value)
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_free_pricing(7)
        assert ei.value.code == -1 and "rule" in str(ei.value)
        assert ctx.config() == before
        with pytest.raises(spx.SimplexError) as ei:  # the dual loop still takes no free column
            ctx.set_algorithm(spx.ALGO_DUAL)
        assert ei.value.code == -5 and "free columns" in str(ei.value) and "dual" in str(ei.value)
        bad = l.copy()
        bad[int(np.flatnonzero(np.isfinite(u))[0])] = -np.inf
        with pytest.raises(spx.SimplexError) as ei:  # ... and upper-only columns stay out
            ctx.set_bounds_lu(bad, u)
        assert ei.value.code == -1 and "upper-only" in str(ei.value)
        assert ctx.config() == before and np.array_equal(ctx.bounds_lu()[0], l)
        assert reached(ctx, g)
        # under Dantzig the setting is inert again: accepted, and the default refusal is back
        ctx.set_primal_pricing(D)
        ctx.set_primal_free_pricing(D)
        assert ctx.config()["primal_free_pricing"] == D
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_pricing(S)
        assert ei.value.code == -5 and "steepest-edge pricing does not run with free columns" in str(ei.value)
    # a context without free columns: inert, every value of the two accepted, the §7h passes
    with plain(lp, upper=np.where(np.isfinite(l), u, 1.0), primal_pricing=S, primal_free_pricing=S) as ctx:
        ctx.set_primal_free_pricing(D)
        ctx.set_primal_free_pricing(S)
        ctx.set_primal_free_pricing(D)
        assert ctx.solve().status == spx.SolveStatus.OptimumFound


def test_default_still_refuses(spx):
    """With the new setting at its default the combination is refused with the
    messages it always had: spx_set_bounds_lu under steepest edge,
    spx_set_primal_pricing on a context with free columns, and at create."""
    At, b, c, l, u, A = _lp("feasible", 7, 20, 0)
    S = spx.PRIMAL_PRICING_STEEPEST
    with spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, primal_pricing=S) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_bounds_lu(l, u)
        assert ei.value.code == -5
        assert ("do not run with steepest-edge pricing (spx_set_primal_pricing); set SPX_PRIMAL_PRICING_DANTZIG first"
                in str(ei.value)) and "free columns (3 of them)" in str(ei.value)
        lb, ub = ctx.bounds_lu()
        assert not lb.any() and np.all(np.isposinf(ub))
    with spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, lower=l, upper=u) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_pricing(S)
        assert ei.value.code == -5
        assert ("spx_set_primal_pricing: steepest-edge pricing does not run with free columns (3 of them, "
                "spx_set_bounds_lu)") in str(ei.value)
        assert ctx.config()["primal_pricing"] == spx.PRIMAL_PRICING_DANTZIG
    with pytest.raises(spx.SimplexError) as ei:
        spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, primal_pricing=S, lower=l, upper=u)
    assert ei.value.code == -5 and "steepest-edge" in str(ei.value)
    with pytest.raises(spx.SimplexError) as ei:  # the opt-in does not reach the dual loop
        spx.Context(At, b, c, algorithm=spx.ALGO_DUAL, primal_free_pricing=S, lower=l, upper=u)
    assert ei.value.code == -5 and "dual" in str(ei.value)


def test_cli(golden, tmp_path):
    """./solver --primal-box --lower F --bounds G [--phase1 --phase1-pricing steepest]
    --primal-pricing steepest, with and without --free-pricing steepest."""
    solver = os.path.join(ROOT, "solver")

    def dump(name, v):
        path = str(tmp_path / name)
        with open(path, "w") as f:
            f.write("\n".join(("inf" if x > 0 else "-inf") if np.isinf(x) else "%.17g" % x for x in v) + "\n")
        return path

    for kind in KINDS:
        m, n, seed = 65, 200, 1
        _, b, c, l, u, A = _lp(kind, m, n, seed)
        g = golden["by_shape"][(kind, m, n, seed)]
        p = str(tmp_path / f"{kind}.txt")
        with open(p, "w") as f:
            f.write(f"{m} {n}\n")
            for row in A:
                f.write(" ".join("%.17g" % v for v in row) + "\n")
            f.write(" ".join("%.17g" % v for v in b) + "\n")
            f.write(" ".join("%.17g" % v for v in c) + "\n")
        base = [solver, "--primal-box", "--lower", dump(f"{kind}_l.txt", l), "--bounds", dump(f"{kind}_u.txt", u),
                "--primal-pricing", "steepest"]
        if kind == "general":
            base += ["--phase1", "--phase1-pricing", "steepest"]
        r = subprocess.run(base + ["--free-pricing", "steepest", "--json", "--no-iter-lines", p], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "Optimum found" in r.stdout
        js = json.loads(r.stdout.splitlines()[-1])
        assert js["status"] == 1 and js["pivots"] == g["ref_pivots"]
        assert abs(js["z"] - g["highs_z"]) <= REL * abs(g["highs_z"])
        assert (js["flip_passes"], js["to_upper"]) == (g["flips"], g["to_upper"])
        if kind == "general":
            assert (js["phase1_passes"], js["phase1_pivots"], js["phase1_rows"]) == (g["p1_passes"], g["p1_pivots"],
                                                                                      g["ninf0"])
        for extra in ([], ["--free-pricing", "dantzig"]):  # without it: today's refusal and exit code
            r = subprocess.run(base + extra + [p], capture_output=True, text=True, timeout=120)
            assert r.returncode == 1 and "spx_set_bounds_lu failed" in r.stderr
            assert "do not run with steepest-edge pricing" in r.stderr and "free columns" in r.stderr


def test_ranging_65(spx, golden):
    """At the 65 x 200 optimum reached under the new rule, cost and right-hand-side
    ranging against tests/ranging_ref.py on that basis, with
    tests/test_gpu_ranging.py's comparison and error bounds."""
    kind, m, n, seed = "general", 65, 200, 1
    _, b, c, l, u, A = _lp(kind, m, n, seed)
    g = golden["by_shape"][(kind, m, n, seed)]
    rlp = (A, b, c, l, u)
    with _ctx(spx, _lp(kind, m, n, seed), True) as ctx:
        r = ctx.solve()
        assert r.status == spx.SolveStatus.OptimumFound and r.pivots == g["ref_pivots"]
        gc = ctx.cost_ranging()
        gr = ctx.rhs_ranging()
        s, up, fr, cost, rhs, e_x = ranging_checks._device_ref(ctx, rlp)
    assert ranging_checks.rr.refuse_case(cost, rhs, s["binv"], ranging_checks.TOL) == []
    wc, cc, sc = ranging_checks._compare_cost(A, s, cost, gc)
    wr, cr, sr = ranging_checks._compare_rhs(s, rhs, gr, e_x)
    print(f"ranging at the steepest-edge optimum: cost worst error / bound = {wc:.3g} ({cc} indices compared, {sc} exempt); "
          f"rhs {wr:.3g} ({cr} compared, {sr} exempt); {int(fr.sum())} free columns")
    assert cc > 0 and cr > 0 and wc <= 1.0 and wr <= 1.0, (wc, wr)
