"""GPU: exact ties in the dual loop (Dantzig and steepest-edge rows), the boxed
dual loop, the long-step ratio test, the bounded primal loop, its phase 1 and
the free-column rules of general bounds (the *_f kernels: the key -|d_j| of a
free column under the common argmin, sigma_p from the sign of d_p, a row whose
basic column is free never blocks, a fixed column flips at once; tied_lp.tied_lu
has integer lower bounds, fixed columns and free columns of both cost signs).

The LPs are the integer interval-matrix LPs of tests/tied_lp.py: A = [+-U | I]
is totally unimodular and b, c, u are integers, so every x_b, y, B^-1 entry,
reduced cost, ratio key, slope and steepest-edge weight is a small integer
(the steepest-edge key is one fp64 division of two of them) and no order of
summation, reduction or reinversion can change a bit.  What is left to decide a
pass is the first-index tie rule of every argmin ("smallest column on ties",
"first row wins ties through every reduction", the (key, column) order of the
long-step walk, `u_p <= t_q`: flip, `slope' <= 0`: enter), and the golden cases
(tests/golden/tied_optima.json, written by tests/golden/make_golden_tied.py)
meet such ties in most passes: their `ties` counters say how often.  So the
kernels must agree with the numpy references exactly: status, pivot count, (p,
q) trace, basis, at-upper set, every counter, z against HiGHS with ==, and x_b,
y and B^-1 with np.array_equal.  No tolerance appears in this file.

Every solve is bounded by the reference's pivot count plus a margin, so a
kernel that leaves the reference's path ends in MaxIter instead of cycling.
"""
import json
import os

import numpy as np
import pytest

import tied_lp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "tied_optima.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
IDS = [f"{g['variant']}-{g['m']}x{g['n']}" for g in GOLDEN]
AT_130 = [g for g in GOLDEN if g["m"] == 130]
LONG_130 = [g for g in AT_130 if g["variant"].startswith("long_")]
MARGIN = 64  # pivots allowed beyond the reference's count before a solve gives up

_REFS = {}


def _case(g):
    """((A_cols (n, m), b, c, u), the reference's result), computed once per
    case; (A_cols, b, c, l, u) for the general-bounds variants."""
    k = (g["variant"], g["m"])
    if k not in _REFS:
        lp = tied_lp.case_lp(g["variant"], g["m"], g["n"], g["seed"], bool(g["mixed"]))
        r = tied_lp.case_ref(g["variant"], lp, trace_cap=200)
        _REFS[k] = ((np.ascontiguousarray(lp[0].T), *lp[1:]), r)
    return _REFS[k]


def _ctx(spx, variant, lp, **kw):
    """The arguments the sibling files use for the variant's loop."""
    kw.setdefault("trace", 200)
    if variant in tied_lp.LU_VARIANTS:
        At, b, c, l, u = lp
        return spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, lower=l, upper=u, primal_phase1=True, **kw)
    At, b, c, u = lp
    rule = spx.DUAL_PRICING_STEEPEST if variant.endswith("steepest") else spx.DUAL_PRICING_DANTZIG
    if variant.startswith("dual_"):
        return spx.Context(At, b, c, window=-1, algorithm=spx.ALGO_DUAL, dual_pricing=rule, **kw)
    if variant.startswith("box_"):
        return spx.Context(At, b, c, window=-1, algorithm=spx.ALGO_DUAL, dual_pricing=rule, upper=u, **kw)
    if variant.startswith("long_"):
        return spx.Context(At, b, c, window=-1, algorithm=spx.ALGO_DUAL, dual_pricing=rule,
                           dual_ratio=spx.DUAL_RATIO_LONG_STEP, upper=u, **kw)
    return spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, primal_phase1=variant.startswith("phase1"), **kw)


def _run_and_check(spx, g, **kw):
    variant = g["variant"]
    lp, ref = _case(g)
    boxed = not variant.startswith("dual_")
    with _ctx(spx, variant, lp, **kw) as ctx:
        r = ctx.solve(g["ref_pivots"] + MARGIN)
        tp, tq = ctx.trace()
        s = ctx.state(binv=True)
        x, up = ctx.primal() if boxed else (None, np.zeros(g["n"], dtype=bool))
        dflips, pflips, ph = ctx.dual_flips(), ctx.primal_flips(), ctx.primal_phase1()
    print(f"{variant} {g['m']}x{g['n']} {kw}: status {int(r.status)} z={r.z} (HiGHS {g['highs_z']}) pivots={r.pivots} "
          f"(reference {g['ref_pivots']}) dual flips {dflips} primal flips {pflips} phase 1 {ph}; ties {g['ties']}")
    # the golden record, the live reference and the run agree on what is compared
    assert ref.status == g["ref_status"] and ref.pivots == g["ref_pivots"] and ref.integral
    want = {"infeasible": spx.SolveStatus.Infeasible, "unbounded": spx.SolveStatus.Unbounded,
            "optimum": spx.SolveStatus.OptimumFound}[g["ref_status"]]
    assert r.status == want, r.status
    assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
    k = min(g["ref_pivots"], 200)
    assert tp.tolist()[:k] == g["ref_trace_p"][:k]
    assert tq.tolist()[:k] == g["ref_trace_q"][:k]
    assert r.b_ixs.tolist() == g["ref_b_ixs"] and s["b_ixs"].tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(up).tolist() == g["ref_at_upper"]
    if variant.startswith("long_"):
        assert dflips == (g["flips"], g["flip_passes"], g["max_flips"]), dflips
    else:
        assert dflips == (0, 0, 0), dflips
    lu = variant in tied_lp.LU_VARIANTS
    if variant in ("pbox", "phase1", "phase1_infeasible") or lu:
        assert pflips == (g["flips"], g["to_upper"]), pflips
    else:
        assert pflips == (0, 0), pflips
    if variant.startswith("phase1") or lu:
        assert ph == (g["p1_passes"], g["p1_pivots"], g["ninf0"], g["ninf"]), ph
    else:
        assert ph == (0, 0, 0, 0), ph
    if g["highs_z"] is not None:
        assert r.z == g["highs_z"], (r.z, g["highs_z"])
    for name, got, exp in (("x_b", s["x_b"], ref.x_b), ("y", s["y"], ref.y), ("binv", s["binv"], ref.Binv)):
        assert np.array_equal(got, np.rint(got)), name  # integral
        assert np.array_equal(got, exp), (name, float(np.max(np.abs(got - exp))))
    assert np.array_equal(r.x_b, ref.x_b)  # (general bounds: both in the caller's variables, l included)
    if lu:
        assert np.array_equal(x, ref.primal_lu(lp[3], lp[4]))  # a non-basic column exactly l_j, u_j or 0 (free)


@pytest.mark.parametrize("g", GOLDEN, ids=IDS)
def test_tied_parity(spx, g):
    _run_and_check(spx, g)


@pytest.mark.parametrize("kw", [{"price_grid": 3}, {"global_y": True}, {"refactor_every": 7}],
                         ids=["price_grid3", "global_y", "refactor7"])
@pytest.mark.parametrize("g", AT_130, ids=[g["variant"] for g in AT_130])
def test_variants_130(spx, g, kw):
    """Ties that straddle the workgroups of a three-workgroup pricing grid, y in
    global memory and a reinversion every 7 pivots (pivoting keeps the basis
    unimodular, so the reinverted B^-1 holds the same integers): the same exact
    results."""
    _run_and_check(spx, g, **kw)


@pytest.mark.parametrize("g", LONG_130, ids=[g["variant"] for g in LONG_130])
def test_walk_from_global_memory(spx, monkeypatch, g):
    """k_dual_long's path that reads the keys from global memory in every round
    walks the same tied keys in the same (key, column) order."""
    monkeypatch.setenv("SPX_DUAL_LONG_GLOBAL", "1")
    _run_and_check(spx, g)


FREE_130 = [g for g in AT_130 if g["variant"] == "free"]


@pytest.mark.parametrize("g", FREE_130, ids=[g["variant"] for g in FREE_130])
def test_free_from_global_memory(spx, monkeypatch, g):
    """SPX_PBOX_LDS_CAP=1000 at L = 256 (vectors of 2048 and 4096 bytes): y and
    the update's pending row and A_p are read from global memory, so the exact
    ties go through k_pbox_price_f<false> and k_pbox_update_f<false>
    (loop_layout()'s pbox_* fields govern the *_f launches too)."""
    monkeypatch.setenv("SPX_PBOX_LDS_CAP", "1000")
    lp, _ = _case(g)
    with _ctx(spx, g["variant"], lp) as ctx:
        ctx.iterate(1)
        lay = ctx.loop_layout()
    print(f"free 130x390 under SPX_PBOX_LDS_CAP=1000: layout {lay}")
    assert lay["pbox_price_lds"] == 0 and lay["pbox_update_lds"] == 0, lay
    _run_and_check(spx, g)


def _tiny(spx, lp, **kw):
    A, b, c, u = lp
    return spx.Context(np.ascontiguousarray(A.T), b, c, upper=u, trace=8, **kw)


def test_exact_capacity(spx):
    """x1 + x2 >= 3, u = (1, 2): the walk's slope goes 3 -> 2 -> 0; at exactly 0
    x2 enters at its bound after the one flip of x1.  OptimumFound, x = (1, 2)."""
    lp = tied_lp.exact_capacity()
    for rule in (spx.DUAL_PRICING_DANTZIG, spx.DUAL_PRICING_STEEPEST):
        with _tiny(spx, lp, window=-1, algorithm=spx.ALGO_DUAL, dual_pricing=rule,
                   dual_ratio=spx.DUAL_RATIO_LONG_STEP) as ctx:
            r = ctx.solve(8)
            x, up = ctx.primal()
            tp, tq = ctx.trace()
            assert r.status == spx.SolveStatus.OptimumFound and r.pivots == 1 and r.z == -5.0, r
            assert x.tolist() == [1.0, 2.0, 0.0] and up.tolist() == [True, False, False]
            assert ctx.dual_flips() == (1, 1, 1)
            assert (tp.tolist(), tq.tolist()) == ([1], [0]) and r.b_ixs.tolist() == [1]


def test_short_capacity(spx):
    """x1 + x2 >= 4 with the same bounds: Infeasible, nothing flipped, no counter moved."""
    lp = tied_lp.short_capacity()
    for rule in (spx.DUAL_PRICING_DANTZIG, spx.DUAL_PRICING_STEEPEST):
        with _tiny(spx, lp, window=-1, algorithm=spx.ALGO_DUAL, dual_pricing=rule,
                   dual_ratio=spx.DUAL_RATIO_LONG_STEP) as ctx:
            r = ctx.solve(8)
            x, up = ctx.primal()
            assert r.status == spx.SolveStatus.Infeasible and r.pivots == 0, r
            assert not up.any() and ctx.dual_flips() == (0, 0, 0)
            assert r.b_ixs.tolist() == [2] and x.tolist() == [0.0, 0.0, -4.0]


@pytest.mark.parametrize("phase1", [False, True])
def test_flip_tie(spx, phase1):
    """u_p == t_q exactly (3 == 3): the pass is a flip, then a degenerate pivot."""
    lp = tied_lp.flip_tie()
    with _tiny(spx, lp, algorithm=spx.ALGO_PRIMAL_BOX, primal_phase1=phase1) as ctx:
        r = ctx.solve(8)
        x, up = ctx.primal()
        tp, tq = ctx.trace()
        assert r.status == spx.SolveStatus.OptimumFound and r.pivots == 1 and r.z == 6.0, r
        assert ctx.primal_flips() == (1, 0)
        assert x.tolist() == [3.0, 0.0, 0.0] and up.tolist() == [True, False, False]
        assert (tp.tolist(), tq.tolist()) == ([1], [0]) and r.b_ixs.tolist() == [1]
