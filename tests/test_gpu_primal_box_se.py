"""GPU: exact primal steepest-edge pricing for the bounded primal simplex loop
(SPX_PRIMAL_PRICING_STEEPEST, spx_set_primal_pricing, spx_get_primal_weights;
DESIGN.md §7h) on the LPs of tests/primal_box_ref.py boxed_primal(m, n, seed).

Golden values (tests/golden/primal_box_se_optima.json, written by
tests/golden/make_golden_primal_box_se.py): pivot count, the first 200 (p, q)
pairs, the final basis and at-upper set and the flip / to-upper counts of the
numpy restatement tests/primal_box_se_ref.py, its weight drift, and HiGHS's
optimum.  The smallest relative gap between the best and the second-best key of
either argmin over those runs is 2.7e-6 (the steepest-edge key at 130 x 390; the
generator refuses a case below 1e-6), so pass-for-pass equality does not depend
on the fp64 summation order.

Shapes: 7 x 20 (m below one wave), 65 x 200 (L = 128, heavy padding), 130 x 390
(m no multiple of 64), 256 x 1024 (multi-chunk columns, several update
workgroups and row blocks for tau), 1024 x 4096 (pivot count, optimum and
certificate).

Weights against exact: the tolerance is 100 x the restatement's own recorded
drift at 256 x 1024 (the larger of its two measures, 2.3e-11, so 2.3e-9) with a
floor of 1e-12.  The GPU sums in another order, so its error is of the same
order, and 100 x the drift is still orders of magnitude below the 1e-6 gap that
decides a pivot.
"""
import json
import os

import numpy as np
import pytest

import dual_box_ref
import dual_ref
import primal_box_ref
import primal_box_se_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "primal_box_se_optima.json")) as f:
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


def _ctx(spx, m, n, seed, **kw):
    At, b, c, u, _ = _lp(m, n, seed)
    kw.setdefault("trace", 200)
    kw.setdefault("primal_pricing", spx.PRIMAL_PRICING_STEEPEST)
    return spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, **kw)


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
        assert ctx.config()["primal_pricing"] == spx.PRIMAL_PRICING_STEEPEST
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        flips = ctx.primal_flips()
    return r, tp.tolist(), tq.tolist(), x, up, flips


def _weight_error(A, b_ixs, w):
    """Largest relative difference between the non-basic entries of w and 1 +
    ||B^-1 A_j||^2 recomputed from the basis."""
    n = A.shape[1]
    basic = np.zeros(n, dtype=bool)
    basic[b_ixs] = True
    ex = ref.exact_weights(A, np.linalg.inv(A[:, b_ixs]), basic)
    return float(np.max(np.abs(w[~basic] - ex[~basic]) / ex[~basic]))


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
    """The three vectors in global memory, a three-workgroup pricing grid and a
    reinversion every 50 pivots (it lands with a weight update pending) walk the
    same passes."""
    m, n, seed = 256, 1024, 3
    r, tp, tq, x, up, flips = _solve(spx, m, n, seed, **kw)
    print(f"{kw}: z={r.z:.13g} pivots={r.pivots} flips={flips}")
    _check_against_golden(spx, golden[0][(m, n, seed)], r, tp, tq, x, up, flips, _lp(m, n, seed))


@pytest.mark.parametrize("vecs", ["1", "0"])
def test_lds_layouts_256(spx, golden, monkeypatch, vecs):
    """The pricing kernel's other LDS layouts (the default stages all three
    vectors; y alone is what a context takes whose vectors do not fit three
    times, none is global_y's): the arithmetic does not depend on the layout,
    so the state after 40 pivots is the default's bit for bit."""
    m, n, seed = 256, 1024, 3
    g = golden[0][(m, n, seed)]
    with _ctx(spx, m, n, seed) as a:
        a.iterate(40)
        wa, sa = a.primal_weights(), a.state(binv=True)
    monkeypatch.setenv("SPX_PBOX_SE_LDS", vecs)
    with _ctx(spx, m, n, seed) as b:
        b.iterate(40)
        wb, sb = b.primal_weights(), b.state(binv=True)
        r = b.solve()
    assert sa["b_ixs"].tolist() == sb["b_ixs"].tolist()
    for k in ("x_b", "y", "binv"):
        assert np.array_equal(sa[k], sb[k]), k
    nb = np.ones(n, dtype=bool)
    nb[sa["b_ixs"]] = False
    assert np.array_equal(wa[nb], wb[nb])
    assert r.status == spx.SolveStatus.OptimumFound and r.pivots == g["ref_pivots"]


def test_single_steps_and_weights_256(spx, golden):
    """iterate(1) forty times against one iterate(40): the same trace and the
    same state bit for bit, B^-1 and the weights included (a readback after every
    pass, the limit cut-off with an update pending, a flip pass right after a
    pivot where the golden trace has one).  Then the weights against 1 + ||B^-1
    A_j||^2 recomputed from the basis, here and at the optimum."""
    m, n, seed = 256, 1024, 3
    g = golden[0][(m, n, seed)]
    A = _lp(m, n, seed)[4]
    tol = max(100.0 * g["drift"], 1e-12)
    with _ctx(spx, m, n, seed) as a, _ctx(spx, m, n, seed) as b:
        for i in range(40):
            st, piv = a.iterate(1)
            assert piv == i + 1 and st == spx.SolveStatus.MaxIter
            if i % 8 == 3:
                a.primal_weights()  # a weight readback between passes applies the pending update
        st, piv = b.iterate(40)
        assert piv == 40
        ta, tb = a.trace(), b.trace()
        assert ta[0].tolist() == tb[0].tolist() == g["ref_trace_p"][:40]
        assert ta[1].tolist() == tb[1].tolist() == g["ref_trace_q"][:40]
        wa, wb = a.primal_weights(), b.primal_weights()
        sa, sb = a.state(binv=True), b.state(binv=True)
        for k in ("x_b", "y", "c_B", "binv"):
            assert np.array_equal(sa[k], sb[k]), k
        assert sa["b_ixs"].tolist() == sb["b_ixs"].tolist()
        nb = np.ones(n, dtype=bool)
        nb[sa["b_ixs"]] = False
        assert np.array_equal(wa[nb], wb[nb])
        assert np.array_equal(a.primal_weights()[nb], wa[nb])  # a second readback applies nothing
        assert np.array_equal(a.primal()[1], b.primal()[1]) and a.primal_flips() == b.primal_flips()
        e40 = _weight_error(A, sa["b_ixs"], wa)
        ra, rb = a.solve(), b.solve()
        assert ra.pivots == rb.pivots == g["ref_pivots"] and ra.z == rb.z
        wo = a.primal_weights()
        assert np.array_equal(wo[~np.isin(np.arange(n), ra.b_ixs)], b.primal_weights()[~np.isin(np.arange(n), rb.b_ixs)])
        eopt = _weight_error(A, ra.b_ixs, wo)
    print(f"weights against exact: {e40:.2e} after 40 pivots, {eopt:.2e} at the optimum (tolerance {tol:.2e}, "
          f"reference drift {g['drift']:.2e})")
    assert e40 <= tol and eopt <= tol, (e40, eopt, tol)


def test_certificate_1024(spx, golden):
    """1024 x 4096: the golden pivot count, z against HiGHS and the certificate
    recomputed on the CPU from the returned basis and placements."""
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
    assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    assert len(set(r.b_ixs.tolist())) == m
    res = _check_primal(x, up, A, b, u)
    viol, dviol, zc = primal_box_ref.certificate(A, b, c, u, r.b_ixs, up)
    print(f"primal residual {res:.2e}, bound violation {viol:.2e}, reduced-cost sign violation {dviol:.2e}")
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= REL * abs(z)


def test_rule_change_mid_solve(spx, golden):
    """30 Dantzig pivots, then steepest edge: the trace of the restatement
    started from that basis and those placements with restarted weights.  Back
    to Dantzig, the weights are refused."""
    m, n, seed = 256, 1024, 3
    At, b, c, u, A = _lp(m, n, seed)
    head = primal_box_ref.primal_simplex_box(A, b, c, u, max_iter=30)
    want = ref.primal_simplex_box_se(A, b, c, u, basis=head.b_ixs, at_upper=head.at_upper, trace_cap=170)
    assert want.status == dual_ref.OPTIMUM and min(want.gap_price, want.gap_ratio, want.gap_flip) >= 1e-6
    with _ctx(spx, m, n, seed, primal_pricing=spx.PRIMAL_PRICING_DANTZIG) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.primal_weights()
        assert ei.value.code == -5 and "Dantzig" in str(ei.value)
        st, piv = ctx.iterate(30)
        assert piv == 30
        s = ctx.state()
        assert s["b_ixs"].tolist() == head.b_ixs.tolist() and np.array_equal(ctx.primal()[1], head.at_upper)
        ctx.set_primal_pricing(spx.PRIMAL_PRICING_STEEPEST)
        assert ctx.config()["primal_pricing"] == spx.PRIMAL_PRICING_STEEPEST
        w0 = ctx.primal_weights()
        assert np.allclose(w0, ref.reference_weights(A), rtol=1e-13, atol=0.0)  # restarted
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        flips = ctx.primal_flips()
        print(f"rule change: 30 Dantzig pivots + {r.pivots - 30} steepest-edge pivots (reference {want.pivots}), "
              f"flips {flips} (reference {head.flips + want.flips}, {head.to_upper + want.to_upper})")
        assert r.status == spx.SolveStatus.OptimumFound and r.pivots == 30 + want.pivots
        k = len(want.trace)
        assert tp.tolist()[30:30 + k] == [p for p, _ in want.trace]
        assert tq.tolist()[30:30 + k] == [q for _, q in want.trace]
        assert r.b_ixs.tolist() == want.b_ixs.tolist() and np.array_equal(up, want.at_upper)
        assert flips == (head.flips + want.flips, head.to_upper + want.to_upper)
        z = golden[0][(m, n, seed)]["highs_z"]
        assert abs(r.z - z) <= REL * abs(z)
        _check_primal(x, up, A, b, u)
        ctx.set_primal_pricing(spx.PRIMAL_PRICING_DANTZIG)
        with pytest.raises(spx.SimplexError) as ei:
            ctx.primal_weights()
        assert ei.value.code == -5


@pytest.mark.parametrize("flipc", [0, 1])
def test_cost_resolve(spx, golden, flipc):
    """Boxed dual solve (steepest), set_cost, then the steepest-edge bounded
    primal loop from that basis: HiGHS's optimum of the new LP in the
    restatement's pivot count."""
    m, n, seed = 256, 1024, 3
    with open(os.path.join(ROOT, "tests", "golden", "primal_box_optima.json")) as f:
        dz = json.load(f)["resolve"]
    res = golden[1]
    g = res["flipc"][flipc]
    assert (res["m"], res["n"], res["seed"], g["flipc"]) == (m, n, seed, flipc)
    z1 = dz["flipc"][flipc]["highs_z"]
    assert g["highs_z"] == z1
    A, b, c, u = dual_box_ref.boxed(m, n, seed, bool(flipc))
    c2 = primal_box_ref.cost_variant(c, n - m, seed)
    with spx.Context(np.ascontiguousarray(A.T), b, c, window=-1, algorithm=spx.ALGO_DUAL,
                     dual_pricing=spx.DUAL_PRICING_STEEPEST, upper=u,
                     primal_pricing=spx.PRIMAL_PRICING_STEEPEST) as ctx:  # (inert under the dual loop)
        r0 = ctx.solve()
        assert r0.status == spx.SolveStatus.OptimumFound
        with pytest.raises(spx.SimplexError) as ei:
            ctx.primal_weights()
        assert ei.value.code == -5 and "SPX_ALGO_PRIMAL_BOX" in str(ei.value)
        ctx.set_cost(c2)
        ctx.set_algorithm(spx.ALGO_PRIMAL_BOX)
        r1 = ctx.solve()
        x, up = ctx.primal()
        k1 = r1.pivots - r0.pivots
        print(f"flipc={flipc}: dual {r0.pivots} pivots; new cost: {k1} steepest-edge pivots (reference "
              f"{g['ref_pivots']}), z={r1.z:.13g} (HiGHS {z1:.13g})")
        assert r1.status == spx.SolveStatus.OptimumFound
        assert abs(r1.z - z1) <= REL * abs(z1), (r1.z, z1)
        assert k1 == g["ref_pivots"], (k1, g["ref_pivots"])
        _check_primal(x, up, A, b, u)
        viol, dviol, zc = primal_box_ref.certificate(A, b, c2, u, r1.b_ixs, up)
        assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
        assert abs(zc - z1) <= REL * abs(z1)


def test_refusals(spx):
    m, n, seed = 7, 20, 0
    At, b, c, u, _ = _lp(m, n, seed)
    # steepest edge with phase 1, in either order
    with pytest.raises(spx.SimplexError) as ei:
        _ctx(spx, m, n, seed, primal_phase1=True)
    assert ei.value.code == -1 and "SPX_FLAG_PRIMAL_PHASE1" in str(ei.value) and "SPX_FLAG_PRIMAL_STEEPEST" in str(ei.value)
    with _ctx(spx, m, n, seed) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_phase1(True)
        assert ei.value.code == -5 and "steepest" in str(ei.value)
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_pricing(7)
        assert ei.value.code == -1 and "rule" in str(ei.value)
        assert ctx.config()["primal_pricing"] == spx.PRIMAL_PRICING_STEEPEST  # the refused calls changed nothing
        assert ctx.solve().status == spx.SolveStatus.OptimumFound
    with _ctx(spx, m, n, seed, primal_pricing=spx.PRIMAL_PRICING_DANTZIG, primal_phase1=True) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_pricing(spx.PRIMAL_PRICING_STEEPEST)
        assert ei.value.code == -5 and "phase 1" in str(ei.value)
        ctx.set_primal_phase1(False)
        ctx.set_primal_pricing(spx.PRIMAL_PRICING_STEEPEST)
        assert ctx.solve().status == spx.SolveStatus.OptimumFound
    # opts.pricing stays the windowed loop's field
    with pytest.raises(spx.SimplexError) as ei:
        spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, pricing=spx.PRICING_STEEPEST)
    assert ei.value.code == -1 and "bounded primal" in str(ei.value)
    # the flag is accepted and inert under the primal loop
    with spx.Context(m=64, n=256, seed=0, primal_pricing=spx.PRIMAL_PRICING_STEEPEST) as ctx:
        assert ctx.solve().status == spx.SolveStatus.OptimumFound
        with pytest.raises(spx.SimplexError) as ei:
            ctx.primal_weights()
        assert ei.value.code == -5


def test_reset_and_set_basis_restart_the_weights(spx, golden):
    m, n, seed = 65, 200, 1
    g = golden[0][(m, n, seed)]
    A = _lp(m, n, seed)[4]
    with _ctx(spx, m, n, seed) as ctx:
        r = ctx.solve()
        ctx.reset()
        assert np.allclose(ctx.primal_weights(), ref.reference_weights(A), rtol=1e-13, atol=0.0)
        r2 = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        _check_against_golden(spx, g, r2, tp.tolist(), tq.tolist(), x, up, ctx.primal_flips(), _lp(m, n, seed))
        assert r2.z == r.z
        ctx.set_basis(r2.b_ixs)  # a warm basis: the reference framework, not the exact norm
        assert np.allclose(ctx.primal_weights(), ref.reference_weights(A), rtol=1e-13, atol=0.0)


def test_cli_primal_pricing(golden, tmp_path):
    """./solver --primal-box --bounds FILE --primal-pricing steepest."""
    import subprocess

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
    r = subprocess.run([solver, "--primal-box", "--bounds", pb, "--primal-pricing", "steepest", "--json",
                        "--no-iter-lines", p], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.splitlines()[-1])
    assert js["status"] == 1 and js["pivots"] == g["ref_pivots"]
    assert abs(js["z"] - g["highs_z"]) <= REL * abs(g["highs_z"])
    assert (js["flip_passes"], js["to_upper"]) == (g["flips"], g["to_upper"])
    r = subprocess.run([solver, "--primal-box", "--phase1", "--bounds", pb, "--primal-pricing", "steepest", p],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "SPX_FLAG_PRIMAL_PHASE1" in r.stderr
