"""GPU: the long-step ratio test of the bounded primal loop's phase 1
(SPX_PRIMAL_RATIO_LONG_STEP, spx_set_primal_phase_one_ratio; k_pbox_long1;
DESIGN.md §7o) on tests/primal_phase1_ref.py boxed_general (upper bounds only:
k_pbox_long1<false> behind k_pbox_update1) and tests/primal_lu_ref.py general_lu
(general bounds, a fifth of the structural columns free: k_pbox_long1<true>
behind k_pbox_update_f), under Dantzig and steepest-edge pricing.

Golden values (tests/golden/primal_phase1_long_optima.json, written by
tests/golden/make_golden_primal_phase1_long.py): pivot count, the first 200 (p, q)
pairs, the final basis and at-upper set, the flip / to-upper counts, the phase-1
counters and the walk's counters of the numpy restatement
tests/primal_phase1_long_ref.py, and HiGHS's optimum.  The generator refuses a
case whose smallest relative gap of an argmin, between u_p and t_q, or between
the leaving breakpoint and its neighbours is below 1e-6, or whose slope comes
within 1e-10 (relative to the terms summed) of the threshold -eps, so
pass-for-pass equality does not depend on the fp64 summation order.

Shapes: 7 x 20, 65 x 200, 130 x 390 (a pricing grid and an update grid of more
than one workgroup: the slots of rparts beyond the first are overwritten), 256 x
1024 (whole solves, up to 75 rows passed in one pass), 1100 x 2300 cut at 30
pivots (more rows than k_pbox_long1 has threads, 258 rows passed in one pass).
SPX_PBOX_LONG_CAP=4 sends every walk with more than four soft breakpoints to the
rounds over global memory.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import phase1_long_child as child
import primal_phase1_long_ref as ref
import primal_phase1_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9
FAMILIES = ("boxed_general", "general_lu")
RULES = ("dantzig", "steepest")
SHAPES = [(7, 20, 0), (65, 200, 1), (130, 390, 2), (256, 1024, 3)]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "primal_phase1_long_optima.json")) as f:
        g = json.load(f)
    g["by_case"] = {(c["family"], c["pricing"], c["m"], c["n"], c["seed"]): c for c in g["cases"]}
    return g


_LPS = {}


def _lp(family, m, n, seed):
    k = (family, m, n, seed)
    if k not in _LPS:
        _LPS[k] = ref.lp_of(family, m, n, seed)
    return _LPS[k]


def _check_optimum(spx, lp, r, x, up, z):
    A, b, c, l, u = lp
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    assert abs(float(c @ x) - r.z) <= REL * abs(z)
    res = float(np.max(np.abs(A @ x - b)))
    assert res <= 1e-9 * max(1.0, np.max(np.abs(b))), res
    viol, dviol, zc = ref.certificate_lu(A, b, c, l, u, r.b_ixs, up)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= REL * abs(z)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("pricing", RULES)
@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_golden_parity(spx, golden, family, pricing, m, n, seed):
    g = golden["by_case"][(family, pricing, m, n, seed)]
    lp = _lp(family, m, n, seed)
    with child.context(family, pricing, lp) as ctx:
        ctx.set_primal_phase1_ratio(spx.PRIMAL_RATIO_LONG_STEP)
        assert ctx.config()["primal_phase1_ratio"] == spx.PRIMAL_RATIO_LONG_STEP
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        flips, ph, ls = ctx.primal_flips(), ctx.primal_phase1(), ctx.primal_long_steps()
    print(f"{family} {pricing} {m}x{n}: z={r.z:.13g} pivots={r.pivots} (golden {g['ref_pivots']}, textbook "
          f"{g['textbook_pivots']}) flips={flips} phase 1 {ph} (textbook passes {g['textbook_p1_passes']}) walk {ls}")
    assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
    k = min(g["ref_pivots"], 200)
    assert tp.tolist()[:k] == g["ref_trace_p"][:k] and tq.tolist()[:k] == g["ref_trace_q"][:k]
    assert r.b_ixs.tolist() == g["ref_b_ixs"] and np.flatnonzero(up).tolist() == g["ref_at_upper"]
    assert flips == (g["flips"], g["to_upper"]), flips
    assert ph == (g["p1_passes"], g["p1_pivots"], g["ninf0"], 0), ph
    assert ls == (g["long_passed"], g["long_passes"], g["long_max"], spx.PRIMAL_RATIO_LONG_STEP), ls
    _check_optimum(spx, lp, r, x, up, g["highs_z"])


def test_more_rows_than_threads(spx, golden):
    """1100 x 2300, the first 30 pivots: every thread of k_pbox_long1 owns two
    rows, 734 rows start out of their bounds and one walk passes 258."""
    g = golden["cut"]
    m, n, seed, k = g["m"], g["n"], g["seed"], g["pivots"]
    assert m > 1024 and g["long_max"] > 200
    lp = _lp(g["family"], m, n, seed)
    with child.context(g["family"], g["pricing"], lp) as ctx:
        ctx.set_primal_phase1_ratio(spx.PRIMAL_RATIO_LONG_STEP)
        st, piv = ctx.iterate(k)
        tp, tq = ctx.trace()
        s = ctx.state()
        flips, ph, ls = ctx.primal_flips(), ctx.primal_phase1(), ctx.primal_long_steps()
    print(f"{m}x{n}: {piv} pivots, flips {flips}, phase 1 {ph}, walk {ls}")
    assert st == spx.SolveStatus.MaxIter and piv == k
    assert tp.tolist()[:k] == g["ref_trace_p"] and tq.tolist()[:k] == g["ref_trace_q"]
    assert flips == (g["flips"], g["to_upper"])
    assert ph == (g["p1_passes"], g["p1_pivots"], g["ninf0"], g["ninf"])
    assert ls == (g["long_passed"], g["long_passes"], g["long_max"], 1)
    xr = np.array(g["ref_x_b"])
    assert np.max(np.abs(s["x_b"][:m] - xr)) <= REL * np.max(np.abs(xr))


def _child(tmp_path, name, env, family, pricing, m, n, seed, k):
    out = str(tmp_path / f"{name}_{family}_{pricing}_{m}_{k}.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "phase1_long_child.py"), out, family, pricing, str(m),
                        str(n), str(seed), str(k)], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    return dict(np.load(out))


@pytest.mark.parametrize("family,pricing,m,n,seed,k", [("boxed_general", "dantzig", 65, 200, 1, 0),
                                                        ("general_lu", "steepest", 65, 200, 1, 0),
                                                        ("boxed_general", "steepest", 130, 390, 2, 40),
                                                        ("general_lu", "dantzig", 130, 390, 2, 40)])
def test_fallback_path_bitwise(spx, golden, tmp_path, family, pricing, m, n, seed, k):
    """SPX_PBOX_LONG_CAP=4: a walk with more than four soft breakpoints goes by
    rounds of argmin over global memory.  The same passes as the sort path, and
    x_b, y and B^-1 the same bits (whole solves at 65 x 200, and after 40 pivots,
    inside phase 1, at 130 x 390)."""
    g = golden["by_case"][(family, pricing, m, n, seed)]
    assert g["long_max"] > 4
    a = _child(tmp_path, "sort", {}, family, pricing, m, n, seed, k)
    b = _child(tmp_path, "rounds", {"SPX_PBOX_LONG_CAP": "4"}, family, pricing, m, n, seed, k)
    want = g["ref_pivots"] if k == 0 else k
    assert int(a["pivots"]) == int(b["pivots"]) == want
    kk = min(want, 200)
    assert a["tp"].tolist()[:kk] == b["tp"].tolist()[:kk] == g["ref_trace_p"][:kk]
    assert a["tq"].tolist()[:kk] == b["tq"].tolist()[:kk] == g["ref_trace_q"][:kk]
    assert a["ls"].tolist() == b["ls"].tolist() and a["ph"].tolist() == b["ph"].tolist()
    assert a["flips"].tolist() == b["flips"].tolist()
    if k == 0:
        assert a["ls"].tolist() == [g["long_passed"], g["long_passes"], g["long_max"], 1]
    else:
        assert a["ph"][3] > 0 and a["ls"][2] > 4  # still in phase 1, and a walk went by rounds
    for key in ("b_ixs", "x_b", "y", "binv", "x", "up"):
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("pricing", RULES)
def test_long_tie(spx, pricing):
    """Exact ties in the walk (tests/primal_phase1_long_ref.py long_tie): the
    smaller 2 row + side goes first, on the device as in the restatement."""
    lp = ref.long_tie()
    rr = ref.primal_simplex_long(*lp, pricing=pricing, ratio="long")
    assert rr.ties["p1_walk"] >= 2
    with child.context("boxed_general", pricing, lp) as ctx:
        ctx.set_primal_phase1_ratio(spx.PRIMAL_RATIO_LONG_STEP)
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        ph, ls = ctx.primal_phase1(), ctx.primal_long_steps()
    assert r.status == spx.SolveStatus.OptimumFound and r.pivots == rr.pivots
    assert list(zip(tp.tolist(), tq.tolist())) == rr.trace and rr.trace[:2] == [(0, 1), (1, 5)]
    assert r.z == rr.z == -31.0
    assert r.b_ixs.tolist() == rr.b_ixs.tolist() and np.array_equal(up, rr.at_upper)
    assert ph == (rr.p1_passes, rr.p1_pivots, rr.ninf0, 0) and ls == rr.long_counters(1)
    assert np.array_equal(r.x_b, rr.x_b)


def test_set_and_unset_is_textbook(spx):
    """Long, then textbook again before the first pass: the golden passes of
    tests/golden/primal_phase1_optima.json, and nothing counted."""
    with open(os.path.join(ROOT, "tests", "golden", "primal_phase1_optima.json")) as f:
        g = {(c["m"], c["n"], c["seed"]): c for c in json.load(f)["cases"]}[(65, 200, 1)]
    lp = _lp("boxed_general", 65, 200, 1)
    with child.context("boxed_general", "dantzig", lp) as ctx:
        ctx.set_primal_phase1_ratio(spx.PRIMAL_RATIO_LONG_STEP)
        ctx.set_primal_phase1_ratio(spx.PRIMAL_RATIO_TEXTBOOK)
        assert ctx.config()["primal_phase1_ratio"] == spx.PRIMAL_RATIO_TEXTBOOK
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        assert ctx.primal_long_steps() == (0, 0, 0, 0)
        assert ctx.primal_phase1() == (g["p1_passes"], g["p1_pivots"], g["ninf0"], 0)
        with pytest.raises(spx.SimplexError):
            ctx.set_primal_phase1_ratio(2)
    assert r.pivots == g["ref_pivots"]
    k = min(r.pivots, 200)
    assert tp.tolist()[:k] == g["ref_trace_p"][:k] and tq.tolist()[:k] == g["ref_trace_q"][:k]
    assert r.b_ixs.tolist() == g["ref_b_ixs"] and np.flatnonzero(up).tolist() == g["ref_at_upper"]
    _check_optimum(spx, lp, r, x, up, g["highs_z"])


def test_switch_after_20_pivots(spx, golden):
    """Textbook for 20 pivots, then long, at 130 x 390: the setter restarts
    nothing, the solve ends at the optimum and the walk has counted."""
    m, n, seed = 130, 390, 2
    g = golden["by_case"][("boxed_general", "dantzig", m, n, seed)]
    lp = _lp("boxed_general", m, n, seed)
    rr = ref.primal_simplex_long(*lp, ratio="long", switch_at=20, trace_cap=200)
    with child.context("boxed_general", "dantzig", lp) as ctx:
        st, piv = ctx.iterate(20)
        assert piv == 20 and ctx.primal_long_steps() == (0, 0, 0, 0) and ctx.primal_phase1()[3] > 0
        ctx.set_primal_phase1_ratio(spx.PRIMAL_RATIO_LONG_STEP)
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        ls = ctx.primal_long_steps()
    print(f"switch at 20: pivots {r.pivots} (restatement {rr.pivots}), walk {ls} (restatement {rr.long_counters(1)})")
    assert ls[0] > 0 and ls[1] > 0 and ls[2] > 0 and ls[3] == 1
    _check_optimum(spx, lp, r, x, up, g["highs_z"])
    if min(rr.gap_price, rr.gap_ratio, rr.gap_flip, rr.gap_walk) >= 1e-6 and rr.gap_slope >= 1e-10:
        k = min(rr.pivots, 200)
        assert r.pivots == rr.pivots and list(zip(tp.tolist()[:k], tq.tolist()[:k])) == rr.trace[:k]
        assert ls == rr.long_counters(1)


def test_refactor_every_7(spx, golden):
    """A reinversion every 7 pivots at 65 x 200 under long: the rows are
    classified again between walks; the optimum and its certificate."""
    m, n, seed = 65, 200, 1
    for family, pricing in (("boxed_general", "dantzig"), ("general_lu", "steepest")):
        g = golden["by_case"][(family, pricing, m, n, seed)]
        lp = _lp(family, m, n, seed)
        with child.context(family, pricing, lp, refactor_every=7) as ctx:
            ctx.set_primal_phase1_ratio(spx.PRIMAL_RATIO_LONG_STEP)
            r = ctx.solve()
            x, up = ctx.primal()
            ls = ctx.primal_long_steps()
        print(f"{family} {pricing} refactor_every=7: pivots {r.pivots} (golden {g['ref_pivots']}), walk {ls}")
        assert ls[0] > 0
        _check_optimum(spx, lp, r, x, up, g["highs_z"])


def test_infeasible(spx):
    """tests/primal_phase1_ref.py contradict at 65 x 200: no column lowers the
    sum of violations any further, with rows still out of their bounds."""
    A, b, c, l, u = _lp("boxed_general", 65, 200, 1)
    A2, b2, u2 = primal_phase1_ref.contradict(A, b, u)
    rr = ref.primal_simplex_long(A2, b2, c, l, u2, ratio="long")
    assert rr.status == ref.INFEASIBLE and rr.ninf > 0
    with child.context("boxed_general", "dantzig", (A2, b2, c, l, u2)) as ctx:
        ctx.set_primal_phase1_ratio(spx.PRIMAL_RATIO_LONG_STEP)
        r = ctx.solve()
        ph, ls = ctx.primal_phase1(), ctx.primal_long_steps()
    print(f"contradictory rows: {r.status} after {r.pivots} pivots (restatement {rr.pivots}), phase 1 {ph}, walk {ls}")
    assert r.status == spx.SolveStatus.Infeasible and ph[3] > 0
    if min(rr.gap_price, rr.gap_ratio, rr.gap_flip, rr.gap_walk) >= 1e-6 and rr.gap_slope >= 1e-10:
        assert r.pivots == rr.pivots and ph == (rr.p1_passes, rr.p1_pivots, rr.ninf0, rr.ninf)
        assert ls == rr.long_counters(1)
