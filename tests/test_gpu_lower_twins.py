"""GPU: non-zero lower bounds under every rule of the dual and the bounded primal
loop ("nothing else on the device knows l").

The LPs are the lower-bound twins of tests/lower_twins.py: a neighbouring golden
case moved by primal_lu_ref.lower_twin (l on about 40 % of all columns, slacks
included, b2 = b + A.l, u2 = u + l), given to the library as Context(..., b2,
lower=l, upper=u2).  Its shifted problem is the neighbour's LP up to rounding
of order 1e-14, and tests/test_lower_twins_cpu.py shows that the neighbour's
numpy restatement walks the golden passes on it with every gap >= 1e-6.  So
each loop must reproduce the neighbour's golden record under l: the boxed dual
loop under Dantzig and steepest-edge rows (flipc 0 and 1), the long-step ratio
test under both (its flips update b_eff in the kernels while box_sync rebuilds
it with k_box_rhs_lu), the bounded primal loop under Dantzig and steepest-edge
columns, and phase 1; at 65 x 200 and 130 x 390.

What comes back is in the caller's variables: z = HiGHS's optimum of the
neighbour + sum_j c_j l_j (the sum in np.longdouble) within the neighbour's
REL = 1e-9 of max(|z|, sum_j |c_j l_j|) -- the second term because the shift
cancels --, a non-basic column exactly l_j or u2_j, x[b_ixs] == x_b, and the
certificate of the basis on the unshifted problem (primal_lu_ref.certificate_lu)
within the neighbouring files' limits, 1e-9 and 1e-7.
"""
import numpy as np
import pytest

import dual_box_ref
import lower_twins as lt
import primal_box_ref
import primal_lu_ref

pytestmark = pytest.mark.gpu

REL = 1e-9
CASES = lt.cases()
AT_130 = [k for k in CASES if k[1] == 130]
DUAL_130 = [k for k in AT_130 if lt.FAMILIES[k[0]].dual]
LONG_130 = [k for k in AT_130 if k[0] == "long"]


def _ids(ks):
    return [lt.case_id(k) for k in ks]


def _ctx(spx, k, **kw):
    name, m, n, seed, flipc, rule = k
    A, b, c, u, l, b2, u2 = lt.twin(name, m, n, seed, flipc)
    kw.setdefault("trace", 200)
    if lt.FAMILIES[name].dual:
        kw.update(window=-1, algorithm=spx.ALGO_DUAL,
                  dual_pricing=spx.DUAL_PRICING_STEEPEST if rule == dual_box_ref.STEEPEST else spx.DUAL_PRICING_DANTZIG)
        if name == "long":
            kw.update(dual_ratio=spx.DUAL_RATIO_LONG_STEP)
    else:
        kw.update(algorithm=spx.ALGO_PRIMAL_BOX, primal_phase1=name == "phase1")
        if name == "pbox_se":
            kw.update(primal_pricing=spx.PRIMAL_PRICING_STEEPEST)
    return spx.Context(np.ascontiguousarray(A.T), b2, c, lower=l, upper=u2, **kw)


def _check_solution(spx, r, x, up, A, b2, c, l, u2, z, zl, zabs):
    """The optimum in the caller's variables."""
    assert r.status == spx.SolveStatus.OptimumFound
    tol = REL * max(abs(z), zabs)
    assert abs(r.z - (z + zl)) <= tol, (r.z, z + zl, tol)
    nb = np.ones(len(x), dtype=bool)
    nb[r.b_ixs] = False
    assert not np.any(up & ~nb)
    assert np.array_equal(x[nb], np.where(up, u2, l)[nb])  # exactly l_j or u2_j
    assert np.array_equal(x[r.b_ixs], r.x_b)
    assert abs(float(c @ x) - (z + zl)) <= tol
    viol, dviol, zc = primal_lu_ref.certificate_lu(A, b2, c, l, u2, r.b_ixs, up)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - (z + zl)) <= tol
    return viol, dviol


def _run_and_check(spx, k, **kw):
    name, m, n, seed, flipc, rule = k
    fam = lt.FAMILIES[name]
    g = lt.golden_case(fam, m, n, seed, flipc, rule)
    A, b, c, u, l, b2, u2 = lt.twin(name, m, n, seed, flipc)
    with _ctx(spx, k, **kw) as ctx:
        lb, ub = ctx.bounds_lu()
        assert np.array_equal(lb, l) and np.array_equal(ub, u2)
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        dflips, pflips, ph = ctx.dual_flips(), ctx.primal_flips(), ctx.primal_phase1()
    zl, zabs = lt.shift_sum(c, l)
    print(f"{lt.case_id(k)} {kw}: z={r.z:.13g} (HiGHS {g['highs_z']:.13g} + c.l {zl:.13g}) pivots={r.pivots} (golden "
          f"{g['ref_pivots']}) dual flips {dflips} primal flips {pflips} phase 1 {ph}; {np.count_nonzero(l)} lower "
          f"bounds, {int(up.sum())} at upper")
    assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
    n200 = min(g["ref_pivots"], 200)
    assert tp.tolist()[:n200] == g["ref_trace_p"][:n200]
    assert tq.tolist()[:n200] == g["ref_trace_q"][:n200]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(up).tolist() == g["ref_at_upper"]
    if name == "long":
        assert dflips == (g["flips"], g["flip_passes"], g["max_flips"]) and g["flips"] > 0, dflips
    else:
        assert dflips == (0, 0, 0), dflips
    assert pflips == ((0, 0) if fam.dual else (g["flips"], g["to_upper"])), pflips
    assert ph == ((g["p1_passes"], g["p1_pivots"], g["ninf0"], 0) if name == "phase1" else (0, 0, 0, 0)), ph
    _check_solution(spx, r, x, up, A, b2, c, l, u2, g["highs_z"], zl, zabs)


@pytest.mark.parametrize("k", CASES, ids=_ids(CASES))
def test_twin_walks_the_golden_passes(spx, k):
    _run_and_check(spx, k)


@pytest.mark.parametrize("kw", [{"price_grid": 3}, {"global_y": True}], ids=["price_grid3", "global_y"])
@pytest.mark.parametrize("k", AT_130, ids=_ids(AT_130))
def test_variants_130(spx, k, kw):
    """A three-workgroup pricing grid and y in global memory: the same passes."""
    _run_and_check(spx, k, **kw)


@pytest.mark.parametrize("k", DUAL_130, ids=_ids(DUAL_130))
def test_reinversion_between_flips_130(spx, k):
    """refactor_every=7 in the dual loops: a reinversion lands in the middle of a
    boxed solve, so box_sync runs k_box_rhs_lu with columns at their upper bound
    (both of its terms) and x_b is recomputed from that b_eff."""
    g = lt.golden_case(lt.FAMILIES[k[0]], *k[1:])
    assert g["ref_pivots"] > 14 and len(g["ref_at_upper"]) > 0
    _run_and_check(spx, k, refactor_every=7)


@pytest.mark.parametrize("k", LONG_130, ids=_ids(LONG_130))
def test_long_step_from_global_memory_130(spx, monkeypatch, k):
    """k_dual_long's path that reads the keys from global memory in every round."""
    monkeypatch.setenv("SPX_DUAL_LONG_GLOBAL", "1")
    _run_and_check(spx, k)


@pytest.mark.parametrize("flipc", [0, 1])
def test_warm_resolve_twin(spx, flipc):
    """tests/test_gpu_primal_box_wexact.py::test_warm_resolve's sequence under
    the twin's bounds: dual steepest-edge solve, set_cost(c2), the bounded
    primal loop under steepest edge with exact weights.  The hand-off's z shift
    sum_j c_j l_j must use the new cost."""
    m, n, seed = lt.RESOLVE_SHAPE
    g = lt.resolve_golden(flipc)
    assert min(g["gap_price"], g["gap_ratio"], g["gap_flip"]) >= 1e-6
    k = ("box", m, n, seed, flipc, dual_box_ref.STEEPEST)
    g0 = lt.golden_case(lt.FAMILIES["box"], *k[1:])
    A, b, c, u, l, b2, u2 = lt.twin("box", m, n, seed, flipc)
    c2 = primal_box_ref.cost_variant(c, n - m, seed)
    zl1, zabs1 = lt.shift_sum(c, l)
    zl2, zabs2 = lt.shift_sum(c2, l)
    assert abs(zl2 - zl1) > 1e-3  # the two shifts differ far beyond the tolerance: the old one would fail
    with _ctx(spx, k, primal_pricing=spx.PRIMAL_PRICING_STEEPEST, primal_weights=spx.PRIMAL_WEIGHTS_EXACT, trace=4096,
              timing=True) as ctx:
        r0 = ctx.solve()
        x0, up0 = ctx.primal()
        assert r0.pivots == g0["ref_pivots"]
        _check_solution(spx, r0, x0, up0, A, b2, c, l, u2, g0["highs_z"], zl1, zabs1)
        ctx.set_cost(c2)
        ctx.set_algorithm(spx.ALGO_PRIMAL_BOX)
        r1 = ctx.solve()
        x, up = ctx.primal()
        tp, tq = ctx.trace()
        flips, (ms, launches) = ctx.primal_flips(), ctx.wexact_times()
        obj = ctx.objective()
    k1 = r1.pivots - r0.pivots
    print(f"re-solve twin {m}x{n} flipc={flipc}: dual {r0.pivots} pivots; new cost, exact start: {k1} pivots (golden "
          f"{g['ref_pivots']}), flips {flips}, z={r1.z:.13g} (HiGHS {g['highs_z']:.13g} + c2.l {zl2:.13g}; c.l "
          f"{zl1:.13g})")
    assert launches == 1
    assert k1 == g["ref_pivots"], (k1, g["ref_pivots"])
    assert flips == (g["flips"], g["to_upper"]), flips
    n200 = len(g["ref_trace_p"])
    assert n200 == min(200, g["ref_pivots"]) and r0.pivots + n200 <= 4096
    assert tp.tolist()[r0.pivots:r0.pivots + n200] == g["ref_trace_p"]
    assert tq.tolist()[r0.pivots:r0.pivots + n200] == g["ref_trace_q"]
    _check_solution(spx, r1, x, up, A, b2, c2, l, u2, g["highs_z"], zl2, zabs2)
    tol = REL * max(abs(g["highs_z"]), zabs2)
    assert abs(obj - float(c2 @ x)) <= tol and abs(obj - r1.z) <= tol, (obj, float(c2 @ x), r1.z)
