"""GPU: exact steepest-edge weights for a warm basis in the bounded primal loop
(SPX_PRIMAL_WEIGHTS_EXACT, spx_set_primal_weight_init, spx_refresh_primal_weights,
spx_pbox_wexact_times; k_pbox_wexact, k_pbox_wexact_slack, k_pbox_wexact_sum;
DESIGN.md §7i).

Weights against numpy: gamma_j = 1 + ||S A_j||^2 with S = B^-1 read back from the
device (spx_get_state), for every non-basic column, structural and slack; basic
entries are not compared.  The tolerance is the a-priori bound

    8 m 2^-53 (1 + || |S| |A_j| ||^2)   (absolute, per column)

Each dot (S A_j)_i carries at most m 2^-53 (|S| |A_j|)_i in any summation order,
fused or not; squaring at most doubles that relative to a_i^2; the sum of the m
squares and the 1 adds another m 2^-53; both sides carry it: 6, rounded up to 8.
The bound is derived, not tuned.

A recurrence step on top of a refresh: within 100 x the restatement's own error
one pivot after an exact start (tests/golden/primal_box_wexact_optima.json
`one_step`: 2.0e-15 at 65 x 200, 1.2e-15 at 130 x 390), relative.

Warm re-solve: the pivot, flip and to-upper counts (at 130 x 390 also the first
200 (p, q)) of the numpy restatement started from the exact weights; its
smallest gap over those runs is 2.2e-4 (the generator refuses a case below
1e-6), so pass-for-pass equality does not depend on the fp64 summation order.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import dual_box_ref
import primal_box_ref
import primal_box_se_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9
SHAPES = [(7, 20, 0), (65, 200, 1), (130, 390, 2), (256, 1024, 3)]


def _json(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden():
    return _json("primal_box_wexact_optima.json")


@pytest.fixture(scope="module")
def golden_se():
    g = _json("primal_box_se_optima.json")
    return {(c["m"], c["n"], c["seed"]): c for c in g["cases"]}, g["resolve"]


@pytest.fixture(scope="module")
def golden_dantzig():
    return {(c["m"], c["n"], c["seed"]): c for c in _json("primal_box_optima.json")["cases"]}


_LPS = {}


def _lp(m, n, seed):
    """(A_cols (n, m), b, c, u, A (m, n)) of the bounded LP, built once."""
    k = (m, n, seed)
    if k not in _LPS:
        A, b, c, u = ref.boxed_primal(m, n, seed)
        _LPS[k] = (np.ascontiguousarray(A.T), b, c, u, A)
    return _LPS[k]


def _ctx(spx, m, n, seed, c=None, **kw):
    At, b, c0, u, _ = _lp(m, n, seed)
    kw.setdefault("trace", 200)
    kw.setdefault("primal_pricing", spx.PRIMAL_PRICING_STEEPEST)
    return spx.Context(At, b, c0 if c is None else c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, **kw)


def _against_numpy(A, s, w):
    """(largest |w_j - gamma_j| / bound_j over the non-basic columns, how many),
    gamma and the a-priori bound from the device's own B^-1."""
    m, n = A.shape
    S = s["binv"]
    nb = np.ones(n, dtype=bool)
    nb[s["b_ixs"]] = False
    V = S @ A[:, nb]
    gam = 1.0 + np.einsum("ij,ij->j", V, V)
    Va = np.abs(S) @ np.abs(A[:, nb])
    bound = 8.0 * m * 2.0 ** -53 * (1.0 + np.einsum("ij,ij->j", Va, Va))
    return float(np.max(np.abs(w[nb] - gam) / bound)), int(nb.sum())


def _exact_rel_error(A, s, w):
    n = A.shape[1]
    nb = np.ones(n, dtype=bool)
    nb[s["b_ixs"]] = False
    V = s["binv"] @ A[:, nb]
    gam = 1.0 + np.einsum("ij,ij->j", V, V)
    return float(np.max(np.abs(w[nb] - gam) / gam))


def _head(m):
    return 5 if m == 7 else 40


@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_kernel_against_numpy(spx, m, n, seed):
    """m < 16, one row past 64, two past 128 and an aligned case; Dantzig pivots
    first, so slack columns are non-basic and columns sit at their upper bounds."""
    A = _lp(m, n, seed)[4]
    with _ctx(spx, m, n, seed, primal_pricing=spx.PRIMAL_PRICING_DANTZIG) as ctx:
        st, piv = ctx.iterate(_head(m))
        assert piv == _head(m)
        ctx.set_primal_pricing(spx.PRIMAL_PRICING_STEEPEST)
        ctx.refresh_primal_weights()
        w = ctx.primal_weights()
        s = ctx.state(binv=True)
    worst, cnt = _against_numpy(A, s, w)
    nslack = int(np.sum(~np.isin(np.arange(n - m, n), s["b_ixs"])))
    print(f"{m}x{n}: {cnt} non-basic columns ({nslack} slacks), worst error / bound = {worst:.3g}")
    assert cnt == n - m and nslack > 0
    assert worst <= 1.0, worst


def test_determinism_130(spx):
    """Two refreshes in a row, a three-workgroup pricing grid and y in global
    memory: the same bits."""
    m, n, seed = 130, 390, 2
    ws = []
    for kw in ({}, {"price_grid": 3}, {"global_y": True}):
        with _ctx(spx, m, n, seed, primal_pricing=spx.PRIMAL_PRICING_DANTZIG, **kw) as ctx:
            ctx.iterate(40)
            ctx.set_primal_pricing(spx.PRIMAL_PRICING_STEEPEST)
            ctx.refresh_primal_weights()
            w1 = ctx.primal_weights()
            ctx.refresh_primal_weights()
            w2 = ctx.primal_weights()
            nb = np.ones(n, dtype=bool)
            nb[ctx.state()["b_ixs"]] = False
        assert np.array_equal(w1[nb], w2[nb]), kw
        ws.append(w1[nb])
    assert np.array_equal(ws[0], ws[1]) and np.array_equal(ws[0], ws[2])


@pytest.mark.parametrize("k", [0, 1])
def test_refresh_with_a_pivot_pending(spx, golden, golden_se, k):
    """iterate(40) under steepest edge leaves a recurrence and a rank-1 update
    pending: the refresh gives the weights of the current basis and drops the
    record (applied on top of the refresh it would spoil the next readback)."""
    g1 = golden["one_step"][k]
    m, n, seed = g1["m"], g1["n"], g1["seed"]
    _, b, c, u, A = _lp(m, n, seed)
    g = golden_se[0][(m, n, seed)]
    with _ctx(spx, m, n, seed) as ctx:
        st, piv = ctx.iterate(40)
        assert piv == 40 and st == spx.SolveStatus.MaxIter
        ctx.refresh_primal_weights()
        w = ctx.primal_weights()
        s = ctx.state(binv=True)
        assert s["pivots"] == 40 and s["status"] == spx.SolveStatus.MaxIter
        worst, _ = _against_numpy(A, s, w)
        st, piv = ctx.iterate(1)
        assert piv == 41
        w1 = ctx.primal_weights()
        s1 = ctx.state(binv=True)
        e1 = _exact_rel_error(A, s1, w1)
        r = ctx.solve()
        x, up = ctx.primal()
    tol = 100.0 * g1["error"]
    print(f"{m}x{n}: refresh with a pivot pending: error / bound = {worst:.3g}; one pivot later {e1:.2e} relative "
          f"(tolerance {tol:.2e}); solve: {r.pivots} pivots (golden {g['ref_pivots']}), z={r.z:.13g}")
    assert worst <= 1.0, worst
    assert e1 <= tol, (e1, tol)
    z = g["highs_z"]
    assert r.status == spx.SolveStatus.OptimumFound and abs(r.z - z) <= REL * abs(z), (r.z, z)
    assert sorted(r.b_ixs.tolist()) == sorted(g["ref_b_ixs"])
    viol, dviol, zc = primal_box_ref.certificate(A, b, c, u, r.b_ixs, up)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= REL * abs(z)


def test_slack_basis_is_the_same_in_both_modes(spx, golden_se):
    m, n, seed = 130, 390, 2
    g = golden_se[0][(m, n, seed)]
    got = []
    for mode in (spx.PRIMAL_WEIGHTS_REFERENCE, spx.PRIMAL_WEIGHTS_EXACT):
        with _ctx(spx, m, n, seed, primal_weights=mode, timing=True) as ctx:
            assert ctx.config()["primal_weights"] == mode
            w0 = ctx.primal_weights()
            ctx.iterate(40)
            w40 = ctx.primal_weights()
            s40 = ctx.state(binv=True)
            r = ctx.solve()
            tp, tq = ctx.trace()
            got.append((w0, w40, s40, r, tp.tolist(), tq.tolist(), ctx.primal_weights(), ctx.state(binv=True)))
            assert ctx.wexact_times() == (0.0, 0)
    a, b = got
    assert a[3].pivots == b[3].pivots == g["ref_pivots"] and a[3].z == b[3].z
    assert a[4] == b[4] == g["ref_trace_p"][:200] and a[5] == b[5] == g["ref_trace_q"][:200]
    for i in (0, 1, 6):
        assert np.array_equal(a[i], b[i]), i
    for i in (2, 7):
        assert a[i]["b_ixs"].tolist() == b[i]["b_ixs"].tolist()
        for key in ("x_b", "y", "binv"):
            assert np.array_equal(a[i][key], b[i][key]), (i, key)


@pytest.mark.parametrize("flipc", [0, 1])
@pytest.mark.parametrize("shape", [(130, 390, 2), (256, 1024, 3)])
def test_warm_resolve(spx, golden, golden_se, shape, flipc):
    """Boxed dual steepest-edge solve, set_cost, then the bounded primal loop
    under steepest edge from that basis with the weights started exactly: the
    restatement's passes.  In REFERENCE mode the same sequence takes the
    reference framework's count."""
    m, n, seed = shape
    g = {(c["m"], c["n"], c["seed"]): c for c in golden["resolve"]}[shape]["flipc"][flipc]
    assert g["flipc"] == flipc and min(g["gap_price"], g["gap_ratio"], g["gap_flip"]) >= 1e-6
    z1 = g["highs_z"]
    A, b, c, u = dual_box_ref.boxed(m, n, seed, bool(flipc))
    c2 = primal_box_ref.cost_variant(c, n - m, seed)
    At = np.ascontiguousarray(A.T)

    def run(mode):
        with spx.Context(At, b, c, window=-1, algorithm=spx.ALGO_DUAL, dual_pricing=spx.DUAL_PRICING_STEEPEST, upper=u,
                         primal_pricing=spx.PRIMAL_PRICING_STEEPEST, primal_weights=spx.PRIMAL_WEIGHTS_EXACT,
                         trace=4096, timing=True) as ctx:
            ctx.set_primal_weight_init(mode)
            assert ctx.config()["primal_weights"] == mode
            r0 = ctx.solve()
            assert r0.status == spx.SolveStatus.OptimumFound
            ctx.set_cost(c2)
            ctx.set_algorithm(spx.ALGO_PRIMAL_BOX)
            r1 = ctx.solve()
            x, up = ctx.primal()
            tp, tq = ctx.trace()
            return r0, r1, x, up, tp.tolist(), tq.tolist(), ctx.primal_flips(), ctx.wexact_times()

    r0, r1, x, up, tp, tq, flips, (ms, launches) = run(spx.PRIMAL_WEIGHTS_EXACT)
    k1 = r1.pivots - r0.pivots
    print(f"{m}x{n} flipc={flipc}: dual {r0.pivots} pivots; new cost, exact start ({ms * 1e3:.0f} us): {k1} pivots "
          f"(golden {g['ref_pivots']}, reference framework {g['reference_framework_pivots']}), flips {flips}, "
          f"z={r1.z:.13g} (HiGHS {z1:.13g})")
    assert launches == 1
    assert r1.status == spx.SolveStatus.OptimumFound
    assert abs(r1.z - z1) <= REL * abs(z1), (r1.z, z1)
    viol, dviol, zc = primal_box_ref.certificate(A, b, c2, u, r1.b_ixs, up)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z1) <= REL * abs(z1)
    assert k1 == g["ref_pivots"], (k1, g["ref_pivots"])
    assert flips == (g["flips"], g["to_upper"]), (flips, g["flips"], g["to_upper"])
    if "ref_trace_p" in g:
        k = len(g["ref_trace_p"])
        assert k == min(200, g["ref_pivots"]) and r0.pivots + k <= 4096
        assert tp[r0.pivots:r0.pivots + k] == g["ref_trace_p"]
        assert tq[r0.pivots:r0.pivots + k] == g["ref_trace_q"]
    if shape == (256, 1024, 3):
        se = golden_se[1]["flipc"][flipc]
        assert se["ref_pivots"] == [583, 370][flipc] == g["reference_framework_pivots"]
        q0, q1, _, _, _, _, _, (_, launches) = run(spx.PRIMAL_WEIGHTS_REFERENCE)
        assert launches == 0
        assert q1.status == spx.SolveStatus.OptimumFound and q1.pivots - q0.pivots == se["ref_pivots"]


def test_set_basis_under_exact(spx, golden_dantzig):
    """A warm basis from spx_set_basis (the Dantzig golden optimum of the LP's
    first cost, in a context that holds another cost): the restart is exact."""
    m, n, seed = 65, 200, 1
    _, b, c, u, A = _lp(m, n, seed)
    basis = golden_dantzig[(m, n, seed)]["ref_b_ixs"]
    c2 = primal_box_ref.cost_variant(c, n - m, seed)
    with _ctx(spx, m, n, seed, c=c2, primal_weights=spx.PRIMAL_WEIGHTS_EXACT, timing=True) as ctx:
        ctx.set_basis(basis)
        w = ctx.primal_weights()
        s = ctx.state(binv=True)
        assert ctx.wexact_times()[1] == 1
    assert sorted(s["b_ixs"].tolist()) == sorted(basis)
    worst, cnt = _against_numpy(A, s, w)
    print(f"set_basis under EXACT: {cnt} non-basic columns, worst error / bound = {worst:.3g}")
    assert worst <= 1.0, worst


def test_refusals_and_inertness(spx, golden_dantzig):
    m, n, seed = 65, 200, 1
    At, b, c, u, A = _lp(m, n, seed)
    g = golden_dantzig[(m, n, seed)]
    # a Dantzig context with the flag set: the Dantzig golden trace, no exact launch, no weights
    with _ctx(spx, m, n, seed, primal_pricing=spx.PRIMAL_PRICING_DANTZIG, primal_weights=spx.PRIMAL_WEIGHTS_EXACT,
              timing=True) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.refresh_primal_weights()
        assert ei.value.code == -5 and "Dantzig" in str(ei.value)
        rc = ctx._L.spx_set_primal_weight_init(ctx._h, 7)
        assert rc == -1 and b"mode" in ctx._L.spx_last_error()
        with pytest.raises(spx.SimplexError) as ei:
            ctx.set_primal_weight_init(7)
        assert ei.value.code == -1
        assert ctx.config()["primal_weights"] == spx.PRIMAL_WEIGHTS_EXACT  # the refused calls changed nothing
        r = ctx.solve()
        tp, tq = ctx.trace()
        assert r.status == spx.SolveStatus.OptimumFound and r.pivots == g["ref_pivots"]
        k = min(200, g["ref_pivots"])
        assert tp.tolist()[:k] == g["ref_trace_p"][:k] and tq.tolist()[:k] == g["ref_trace_q"][:k]
        assert ctx.primal_flips() == (g["flips"], g["to_upper"])
        assert ctx.wexact_times() == (0.0, 0)
    # the dual loop has no primal pricing weights to refresh
    A2, b2, c2, u2 = dual_box_ref.boxed(m, n, seed, False)
    with spx.Context(np.ascontiguousarray(A2.T), b2, c2, window=-1, algorithm=spx.ALGO_DUAL, upper=u2,
                     primal_pricing=spx.PRIMAL_PRICING_STEEPEST, primal_weights=spx.PRIMAL_WEIGHTS_EXACT) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.refresh_primal_weights()
        assert ei.value.code == -5 and "SPX_ALGO_PRIMAL_BOX" in str(ei.value)
        assert ctx.solve().status == spx.SolveStatus.OptimumFound


def test_cli_primal_weights(golden_se, tmp_path):
    """./solver --primal-box --primal-pricing steepest --primal-weights exact: from
    the slack basis, the steepest-edge golden pivots; an unknown word is refused."""
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
    g = golden_se[0][(m, n, seed)]
    r = subprocess.run([solver, "--primal-box", "--bounds", pb, "--primal-pricing", "steepest", "--primal-weights",
                        "exact", "--json", "--no-iter-lines", p], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.splitlines()[-1])
    assert js["status"] == 1 and js["pivots"] == g["ref_pivots"] and js["primal_weights"] == "exact"
    assert abs(js["z"] - g["highs_z"]) <= REL * abs(g["highs_z"])
    assert (js["flip_passes"], js["to_upper"]) == (g["flips"], g["to_upper"])
    r = subprocess.run([solver, "--primal-box", "--bounds", pb, "--primal-pricing", "steepest", "--primal-weights",
                        "sometimes", p], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--primal-weights" in r.stderr and "sometimes" in r.stderr
