"""GPU: the dual and the bounded primal loop where their vectors outgrow LDS
(DESIGN.md §7d/§7e), and their dense-slack branches.

Both loops choose their kernels from L = round_up(m, 128) against 150 KiB of
LDS: 24 L bytes fit up to L = 6400 (steepest edge stages everything), 16 L up
to L = 9600 (the update kernels stage the pending row and A_p), above that both
are read from global memory.  Every other GPU test of these loops runs at m <=
1024, so three things are checked here, each test first asserting through
Context.loop_layout() that it runs the layout it means to run:

1. Small-shape twins.  SPX_DUAL_LDS_CAP / SPX_PBOX_LDS_CAP lower the cap (bytes)
   so that 256 x 1024 (L = 256: vectors of 2048, 4096 and 6144 bytes) takes the
   layouts of a large m: 5000 turns the steepest-edge update's staging off and
   leaves one vector of the bounded steepest-edge pricing in LDS (LDS pricing
   with a global steepest-edge update), 3000 also turns both updates' and the
   dual pricing's staging off, 1000 puts everything in global memory.  The
   arithmetic order does not depend on where an operand is read from, so after
   40 pivots and again after solve() everything equals the default layout's bit
   for bit; the solve also meets the golden files.  The pricing grids need no
   pinning: 768 non-basic columns ask for 96 workgroups, below any occupancy
   limit, with or without LDS.  The `pbox_free` case (general bounds with free
   columns, tests/test_gpu_primal_lu.py's LPs) runs the *_f kernels: the library
   cannot report which instantiation of them it launched, but loop_layout()'s
   pbox_* fields govern the *_f launches too (pbox_free_prepare,
   launch_pbox_price_f and launch_pbox_update_f read the two flags that
   pbox_prepare set), so pbox_update_lds == 0 is k_pbox_update_f<false> and
   pbox_price_lds == 0 is k_pbox_price_f<false>.
2. Dense slacks.  SPX_DENSE_SLACKS=1 streams a slack column like any other; a
   unit column streamed densely contributes exact zeros, so the same equality
   holds at 130 x 390.  The exception is refresh_primal_weights(): the slack
   weights then come from the MFMA product instead of k_pbox_wexact_slack, in
   another summation order; they are checked with the a-priori bound of
   tests/test_gpu_primal_box_wexact.py.
3. The real thresholds with nothing forced: m = 6401 (L = 6528) and m = 9601 (L =
   9728), n = m + 64, against tests/block_ref.py (np.longdouble, the block
   structure of a basis with at most 64 structural columns) and
   tests/golden/lds_cap_optima.json (tests/golden/make_golden_lds_cap.py: the
   numpy restatements' traces, counters and own residuals, HiGHS's optimum; the
   smallest gap over the seven runs is 5.2e-6, the generator refuses a case
   below 1e-6).  The LPs are the neighbouring tests' generators at (m, m + 64),
   with two exceptions: dual_box_ref.boxed is infeasible this far from square
   (64 columns cannot keep thousands of ranged rows inside their ranges), so
   the boxed dual LP is boxed_tall (the same draws, 16 x the slack bounds); and
   primal_phase1_ref.boxed_general would start phase 1 with thousands of rows
   out of their bounds, so the phase-1 LP is boxed_general_tall (65 such rows).
   The device state may be 100 x the restatement's own residual away from the
   longdouble reference, the margin of primal_box_wexact_optima.json's
   `one_step`: it allows for another summation order and nothing else (measured:
   0.15 % to 2.1 % of what is allowed).  Each of the seven takes 0.4 to 1.5 s,
   the longest solve 851 pivots.
"""
import json
import os
import time

import numpy as np
import pytest

import block_ref
import dual_box_ref
import dual_ref
import primal_box_ref
import primal_phase1_ref
import test_gpu_dual as t_dual
import test_gpu_dual_box as t_box
import test_gpu_dual_long as t_long
import test_gpu_dual_se as t_se
import test_gpu_primal_box as t_pbox
import test_gpu_primal_box_se as t_pse
import test_gpu_primal_box_wexact as t_wx
import test_gpu_primal_lu as t_lu
import test_gpu_primal_phase1 as t_p1

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9
HEAD = 40
ENVS = ("SPX_DUAL_LDS_CAP", "SPX_PBOX_LDS_CAP", "SPX_DENSE_SLACKS")


def _json(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


_GOLD = {}


def _gold(name):
    if name not in _GOLD:
        _GOLD[name] = _json(name)
    return _GOLD[name]


# ---------------------------------------------------------------------------
# The loops as cases: how to make the context, which weights and counters it
# keeps, and the neighbouring file's golden check of a whole solve
# ---------------------------------------------------------------------------
class Case:
    """loop ("dual" / "pbox") and steep say which loop_layout() fields the case's setup fills in."""

    def __init__(self, name, loop, steep, make, check, weights=None, counters=(), boxed=True):
        self.name, self.loop, self.steep, self.make, self.check = name, loop, steep, make, check
        self.weights, self.counters, self.boxed = weights, counters, boxed


def _by_shape(name, key=lambda c: (c["m"], c["n"], c["seed"])):
    return {key(c): c for c in _gold(name)["cases"]}


def _box_key(c):
    return (c["m"], c["n"], c["seed"], c["flipc"], c["rule"])


def _mk_dual(spx, m, n, seed):
    A, b, c = t_dual._lp(m, n, seed)
    return spx.Context(A, b, c, window=-1, trace=200, algorithm=spx.ALGO_DUAL)


def _ck_dual(spx, shape, r, tp, tq, x, up, cnt):
    t_dual._check_against_golden(spx, _by_shape("dual_optima.json")[shape], r, tp, tq)


def _ck_se(spx, shape, r, tp, tq, x, up, cnt):
    t_se._check_against_golden(spx, _by_shape("dual_se_optima.json")[shape],
                               _by_shape("dual_optima.json")[shape]["highs_z"], r, tp, tq)


def _box_case(rule):
    def make(spx, m, n, seed):
        return t_box._ctx(spx, m, n, seed, 0, rule)

    def check(spx, shape, r, tp, tq, x, up, cnt):
        g = _by_shape("dual_box_optima.json", _box_key)[(*shape, 0, rule)]
        t_box._check_against_golden(spx, g, r, tp, tq, x, up, t_box._lp(*shape, 0))

    return Case(f"dual_box_{rule}", "dual", rule == dual_box_ref.STEEPEST, make, check,
                "dual" if rule == dual_box_ref.STEEPEST else None)


def _long_case(rule, flipc):
    def make(spx, m, n, seed):
        return t_long._ctx(spx, m, n, seed, flipc, rule)

    def check(spx, shape, r, tp, tq, x, up, cnt):
        g = _by_shape("dual_long_optima.json", _box_key)[(*shape, flipc, rule)]
        t_long._check_against_golden(spx, g, r, tp, tq, x, up, cnt[0], t_long._lp(*shape, flipc))

    return Case(f"dual_long_{rule}_flipc{flipc}", "dual", rule == dual_box_ref.STEEPEST, make, check,
                "dual" if rule == dual_box_ref.STEEPEST else None, ("dual_flips",))


def _ck_pbox(spx, shape, r, tp, tq, x, up, cnt):
    t_pbox._check_against_golden(spx, _by_shape("primal_box_optima.json")[shape], r, tp, tq, x, up, cnt[0],
                                 t_pbox._lp(*shape))


def _ck_pse(spx, shape, r, tp, tq, x, up, cnt):
    t_pse._check_against_golden(spx, _by_shape("primal_box_se_optima.json")[shape], r, tp, tq, x, up, cnt[0],
                                t_pse._lp(*shape))


def _ck_p1(spx, shape, r, tp, tq, x, up, cnt):
    """The golden file's pivot count, counters and optimum (the whole-solve
    checks of tests/test_gpu_primal_phase1.py), and its first 200 (p, q)."""
    g = _by_shape("primal_phase1_optima.json")[shape]
    _, b, c, u, A = t_p1._lp(*shape)
    assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
    assert tp[:200] == g["ref_trace_p"][:200] and tq[:200] == g["ref_trace_q"][:200]
    assert cnt[0] == (g["flips"], g["to_upper"]) and cnt[1] == t_p1._counters(g), cnt
    t_p1._check_optimum(spx, r, x, up, A, b, c, u, g["highs_z"])


def _ck_free(spx, shape, r, tp, tq, x, up, cnt):
    t_lu._check_against_golden(spx, _by_shape("primal_lu_optima.json")[shape], t_lu._lp(*shape), r, tp, tq, x, up, *cnt)


CASES = [
    Case("dual_dantzig", "dual", False, _mk_dual, _ck_dual, boxed=False),
    Case("dual_steepest", "dual", True, lambda spx, m, n, seed: t_se._ctx(spx, m, n, seed), _ck_se, "dual",
         boxed=False),
    _box_case(dual_box_ref.DANTZIG), _box_case(dual_box_ref.STEEPEST),
    _long_case(dual_box_ref.DANTZIG, 0), _long_case(dual_box_ref.DANTZIG, 1),
    _long_case(dual_box_ref.STEEPEST, 0), _long_case(dual_box_ref.STEEPEST, 1),
    Case("pbox_dantzig", "pbox", False, lambda spx, m, n, seed: t_pbox._ctx(spx, m, n, seed), _ck_pbox, None,
         ("primal_flips",)),
    Case("pbox_phase1", "pbox", False, lambda spx, m, n, seed: t_p1._ctx(spx, t_p1._lp(m, n, seed)), _ck_p1, None,
         ("primal_flips", "primal_phase1")),
    Case("pbox_free", "pbox", False, lambda spx, m, n, seed: t_lu._ctx(spx, t_lu._lp(m, n, seed)), _ck_free, None,
         ("primal_flips", "primal_phase1")),
    Case("pbox_steepest", "pbox", True, lambda spx, m, n, seed: t_pse._ctx(spx, m, n, seed), _ck_pse, "primal",
         ("primal_flips",)),
]
CASE_IDS = [c.name for c in CASES]


def _snap(ctx, case):
    """Everything the twins compare, read back now."""
    s = ctx.state(binv=True)
    tp, tq = ctx.trace()
    out = {"pivots": s["pivots"], "trace": (tp.tolist(), tq.tolist()), "b_ixs": s["b_ixs"].tolist(),
           "x_b": s["x_b"], "y": s["y"], "binv": s["binv"], "counters": tuple(getattr(ctx, k)() for k in case.counters)}
    if case.weights == "dual":
        out["w"] = ctx.dual_weights()  # basis order: every entry is live
    elif case.weights == "primal":
        nb = np.ones(ctx.n, dtype=bool)
        nb[s["b_ixs"]] = False
        out["w"] = ctx.primal_weights()[nb]  # the non-basic entries are live
    if case.boxed:
        out["x"], out["up"] = ctx.primal()
    return out


def _run(spx, case, shape):
    """(layout, snapshot after HEAD pivots, solve result, snapshot after it) under the environment as it is."""
    with case.make(spx, *shape) as ctx:
        st, piv = ctx.iterate(HEAD)
        assert piv == HEAD and st == spx.SolveStatus.MaxIter
        lay = ctx.loop_layout()  # (after a pass: the bounded steepest-edge setup runs with the first one)
        a = _snap(ctx, case)
        r = ctx.solve()
        return lay, a, r, _snap(ctx, case)


def _same(a, b, what):
    assert a["pivots"] == b["pivots"] and a["trace"] == b["trace"] and a["b_ixs"] == b["b_ixs"], what
    for k in ("x_b", "y", "binv", "w", "x", "up"):
        if k in a:
            assert np.array_equal(a[k], b[k]), (what, k)
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])


_DEFAULT = {}


def _default(spx, monkeypatch, case, shape):
    """The default layout's run of a case, made once and shared (read only)."""
    if (case.name, shape) not in _DEFAULT:
        for k in ENVS:
            monkeypatch.delenv(k, raising=False)
        _DEFAULT[(case.name, shape)] = _run(spx, case, shape)
    return _DEFAULT[(case.name, shape)]


ALL_LDS = {"dual_price_lds": 1, "dual_update_lds": 1, "dual_se_update_lds": 1, "dual_se_rho_lds": 1,
           "pbox_price_lds": 1, "pbox_update_lds": 1, "pbox_se_lds_vecs": 3}
# L = 256: 8 L = 2048, 16 L = 4096, 24 L = 6144 bytes
CAPPED = {
    5000: dict(ALL_LDS, dual_se_update_lds=0, dual_se_rho_lds=0, pbox_se_lds_vecs=1),
    3000: dict(ALL_LDS, dual_price_lds=0, dual_update_lds=0, dual_se_update_lds=0, dual_se_rho_lds=0,
               pbox_update_lds=0, pbox_se_lds_vecs=1),
    1000: dict(ALL_LDS, dual_price_lds=0, dual_update_lds=0, dual_se_update_lds=0, dual_se_rho_lds=0,
               pbox_price_lds=0, pbox_update_lds=0, pbox_se_lds_vecs=0),
}


def _expect(case, want, slack_unit):
    """The loop_layout() a case's context must report: its own loop's fields (the
    bounded loop sets the dual loop up too), -1 for what was never set up."""
    exp = {k: -1 for k in ALL_LDS}
    for k in ALL_LDS:
        if k.startswith("dual_") or (case.loop == "pbox" and k != "pbox_se_lds_vecs"):
            exp[k] = want[k]
    if case.loop == "pbox" and case.steep:
        exp["pbox_se_lds_vecs"] = want["pbox_se_lds_vecs"]
    exp["slack_unit"] = slack_unit
    return exp


# ---------------------------------------------------------------------------
# 1. small-shape twins
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cap", sorted(CAPPED, reverse=True))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_capped_layout_is_the_default_bit_for_bit(spx, monkeypatch, case, cap):
    shape = (256, 1024, 3)
    lay0, a0, r0, b0 = _default(spx, monkeypatch, case, shape)
    assert lay0 == _expect(case, ALL_LDS, 1), lay0  # unset: what the library chose before the hook existed
    monkeypatch.setenv("SPX_DUAL_LDS_CAP", str(cap))
    monkeypatch.setenv("SPX_PBOX_LDS_CAP", str(cap))
    lay, a, r, b = _run(spx, case, shape)
    print(f"{case.name} cap {cap}: layout {lay}, pivots {r.pivots}, z={r.z:.13g}")
    assert lay == _expect(case, CAPPED[cap], 1), lay
    _same(a, a0, f"after {HEAD} pivots")
    _same(b, b0, "after solve()")
    assert r.pivots == r0.pivots and r.z == r0.z and r.status == r0.status
    case.check(spx, shape, r, *b["trace"], b.get("x"), b.get("up"), b["counters"])


def test_cap_can_only_lower(spx, monkeypatch):
    """A cap above the built-in 150 KiB changes nothing: at 256 x 1024 everything
    stays in LDS, as with the variables unset."""
    monkeypatch.setenv("SPX_DUAL_LDS_CAP", str(1 << 30))
    monkeypatch.setenv("SPX_PBOX_LDS_CAP", str(1 << 30))
    case = CASES[CASE_IDS.index("pbox_steepest")]
    with case.make(spx, 256, 1024, 3) as ctx:
        ctx.iterate(1)
        assert ctx.loop_layout() == _expect(case, ALL_LDS, 1)


# ---------------------------------------------------------------------------
# 2. dense slacks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_dense_slacks_are_the_unit_slacks_bit_for_bit(spx, monkeypatch, case):
    shape = (130, 390, 2)
    lay0, a0, r0, b0 = _default(spx, monkeypatch, case, shape)
    assert lay0 == _expect(case, ALL_LDS, 1), lay0
    monkeypatch.setenv("SPX_DENSE_SLACKS", "1")
    lay, a, r, b = _run(spx, case, shape)
    print(f"{case.name} dense slacks: layout {lay}, pivots {r.pivots}, z={r.z:.13g}")
    assert lay == _expect(case, ALL_LDS, 0), lay
    _same(a, a0, f"after {HEAD} pivots")
    _same(b, b0, "after solve()")
    assert r.pivots == r0.pivots and r.z == r0.z and r.status == r0.status
    case.check(spx, shape, r, *b["trace"], b.get("x"), b.get("up"), b["counters"])


@pytest.mark.parametrize("m,n,seed", [(65, 200, 1), (130, 390, 2)])
def test_dense_slacks_exact_weights(spx, monkeypatch, m, n, seed):
    """refresh_primal_weights() with the slack columns streamed through the MFMA
    product: tests/test_gpu_primal_box_wexact.py::test_kernel_against_numpy's
    run and a-priori bound, with slack_unit off."""
    monkeypatch.setenv("SPX_DENSE_SLACKS", "1")
    A = t_wx._lp(m, n, seed)[4]
    with t_wx._ctx(spx, m, n, seed, primal_pricing=spx.PRIMAL_PRICING_DANTZIG) as ctx:
        st, piv = ctx.iterate(t_wx._head(m))
        assert piv == t_wx._head(m)
        ctx.set_primal_pricing(spx.PRIMAL_PRICING_STEEPEST)
        ctx.refresh_primal_weights()
        w = ctx.primal_weights()
        s = ctx.state(binv=True)
        lay = ctx.loop_layout()
    worst, cnt = t_wx._against_numpy(A, s, w)
    nslack = int(np.sum(~np.isin(np.arange(n - m, n), s["b_ixs"])))
    print(f"{m}x{n} dense slacks: layout {lay}, {cnt} non-basic columns ({nslack} slacks), worst error / bound = "
          f"{worst:.3g}")
    assert lay["slack_unit"] == 0
    assert cnt == n - m and nslack > 0
    assert worst <= 1.0, worst


# ---------------------------------------------------------------------------
# 3. the real thresholds, nothing forced
# ---------------------------------------------------------------------------
MARGIN = 100.0  # x the restatement's own residual (primal_box_wexact_optima.json's one_step margin)
TALL_HEAD = 24

# what the library must choose by itself: L = 6528 (24 L > 150 KiB >= 16 L), L = 9728 (16 L > 150 KiB >= 8 L)
AT_6401 = dict(ALL_LDS, dual_se_update_lds=0, dual_se_rho_lds=0, pbox_se_lds_vecs=1)
AT_9601 = dict(ALL_LDS, dual_price_lds=0, dual_update_lds=0, dual_se_update_lds=0, dual_se_rho_lds=0,
               pbox_update_lds=0, pbox_se_lds_vecs=1)


def _tall_lp(g):
    """(A_cols (n, m), N (m, 64), b, c, u or None) of a golden case, from the generator's own draws."""
    kind, m, n, seed = g["kind"], g["m"], g["n"], g["seed"]
    if kind == "dual":
        A, b, c = dual_ref.covering(m, n, seed)
        u = None
    elif kind == "long":
        A, b, c, u = dual_box_ref.boxed_tall(m, n, seed, bool(g["flipc"]))
    elif kind in ("pbox", "pbox_se"):
        A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    else:
        A, b, c, u = primal_phase1_ref.boxed_general_tall(m, n, seed)
    return np.ascontiguousarray(A.T), np.ascontiguousarray(A[:, :n - m]), b, c, u


def _tall_ctx(spx, g, At, b, c, u):
    kind = g["kind"]
    steep = g["rule"] == "steepest"
    kw = {"trace": TALL_HEAD}
    if kind in ("dual", "long"):
        kw.update(window=-1, algorithm=spx.ALGO_DUAL,
                  dual_pricing=spx.DUAL_PRICING_STEEPEST if steep else spx.DUAL_PRICING_DANTZIG)
        if kind == "long":
            kw.update(upper=u, dual_ratio=spx.DUAL_RATIO_LONG_STEP)
    else:
        kw.update(algorithm=spx.ALGO_PRIMAL_BOX, upper=u, primal_phase1=kind == "phase1",
                  primal_pricing=spx.PRIMAL_PRICING_STEEPEST if steep else spx.PRIMAL_PRICING_DANTZIG)
    return spx.Context(At, b, c, **kw)


def _tall_counters(ctx, kind):
    if kind == "long":
        f = ctx.dual_flips()
        return {"flips": f[0], "flip_passes": f[1], "max_flips": f[2]}
    if kind == "dual":
        return {}
    f = ctx.primal_flips()
    out = {"flips": f[0], "to_upper": f[1]}
    if kind == "phase1":
        p = ctx.primal_phase1()
        out.update({"p1_passes": p[0], "p1_pivots": p[1], "ninf0": p[2], "ninf": p[3]})
    return out


def _tall_state(ctx, g, N, b, c, u, want, where, ratios):
    """The state read back now against block_ref, within MARGIN x the residuals
    `want` the restatement left at the same point; measured / allowed into `ratios`."""
    kind = g["kind"]
    s = ctx.state(binv=True)
    up = ctx.primal()[1] if u is not None else None
    blk = block_ref.Block(N, s["b_ixs"])
    got = blk.residuals(s["binv"], s["x_b"], s["y"], blk.b_eff(b, u, up), c)
    if kind in ("dual", "long") and g["rule"] == "steepest":
        got["w"] = blk.dual_weight_residual(ctx.dual_weights())
    if kind == "pbox_se":
        got["w"] = blk.primal_weight_residual(ctx.primal_weights())
    assert blk.k == want["k"], (where, blk.k, want["k"])
    # a basic slack's column of B^-1 is an exact unit vector unless that slack has left the basis before
    assert got["nonunit"] == want["nonunit"], (where, got["nonunit"], want["nonunit"])
    for key in ("binv", "x_b", "y", "w"):
        if key in got:
            ratios[f"{where}:{key}"] = (got[key], MARGIN * want[key])
    return s, up, blk


def _run_tall(spx, name, layout, refresh=False):
    g = {c["name"]: c for c in _gold("lds_cap_optima.json")["cases"]}[name]
    kind = g["kind"]
    assert min(g["gaps"].values()) >= 1e-6
    t0 = time.perf_counter()
    At, N, b, c, u = _tall_lp(g)
    t1 = time.perf_counter()
    ratios = {}
    with _tall_ctx(spx, g, At, b, c, u) as ctx:
        st, piv = ctx.iterate(TALL_HEAD)
        lay = ctx.loop_layout()
        case = Case(name, "dual" if kind in ("dual", "long") else "pbox", g["rule"] == "steepest", None, None)
        assert lay == _expect(case, layout, 1), lay  # chosen by the library: nothing is forced here
        assert piv == TALL_HEAD
        tp, tq = ctx.trace()
        assert tp.tolist() == g["ref_trace_p"] and tq.tolist() == g["ref_trace_q"]
        cnt = _tall_counters(ctx, kind)
        cnt.pop("ninf", None)  # (rows out of their bounds mid-way: the golden file holds the count at the optimum)
        assert cnt == {k: g["counters_head"][k] for k in cnt}, (cnt, g["counters_head"])
        _tall_state(ctx, g, N, b, c, u, g["res_head"], "head", ratios)
        if refresh:  # the exact weights of this basis, from the MFMA product at this height
            ctx.refresh_primal_weights()
            nb, want = block_ref.Block(N, ctx.state()["b_ixs"]).primal_weights()
            w = ctx.primal_weights()[nb]
            err = float(np.max(np.abs(w.astype(block_ref.LD) - want) / want))
            ratios["head:w_exact"] = (err, MARGIN * g["res_head"]["w_exact"])
        r = ctx.solve()
        cnt = _tall_counters(ctx, kind)
        s, up, blk = _tall_state(ctx, g, N, b, c, u, g["res_opt"], "opt", ratios)
    t2 = time.perf_counter()
    viol, dviol, zc = blk.certificate(b, c, u, up)
    line = ", ".join(f"{k} {a:.2e}/{w:.2e}" for k, (a, w) in ratios.items())
    print(f"{name} {g['m']}x{g['n']}: layout {lay}")
    print(f"{name}: pivots {r.pivots} (golden {g['ref_pivots']}) counters {cnt} z={r.z:.13g} (HiGHS {g['highs_z']:.13g}) "
          f"bound violation {viol:.2e} reduced-cost violation {dviol:.2e}")
    print(f"{name}: measured / allowed: {line}")
    print(f"{name}: wall {t2 - t0:.1f} s (LP {t1 - t0:.1f} s, device and checks {t2 - t1:.1f} s)")
    assert r.status == spx.SolveStatus.OptimumFound
    assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
    assert cnt == {k: g["counters"][k] for k in cnt}, (cnt, g["counters"])
    for k, (a, w) in ratios.items():
        assert a <= w, (k, a, w)
    z = g["highs_z"]
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    assert abs(zc - z) <= REL * abs(z), (zc, z)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)


def test_6401_dual_steepest(spx):
    """k_dual_price<true> with k_dual_update<false, 2>: LDS pricing, global steepest-edge update."""
    _run_tall(spx, "dual_se_6401", AT_6401)


def test_6401_long_step_steepest(spx):
    """k_dual_price<true, true, true> with k_dual_update<false, 2, true>."""
    _run_tall(spx, "long_se_6401", AT_6401)


def test_6401_primal_box_steepest(spx):
    """k_pbox_price_se<1> with k_pbox_update<true>, and one refresh_primal_weights() at this height."""
    _run_tall(spx, "pbox_se_6401", AT_6401, refresh=True)


def test_9601_dual_dantzig(spx):
    """k_dual_price<false> with k_dual_update<false, 0>."""
    _run_tall(spx, "dual_9601", AT_9601)


def test_9601_long_step_dantzig(spx):
    """k_dual_price<false, true, true> with k_dual_update<false, 0, true>."""
    _run_tall(spx, "long_9601", AT_9601)


def test_9601_primal_box_dantzig(spx):
    """k_pbox_price<true> with k_pbox_update<false>."""
    _run_tall(spx, "pbox_9601", AT_9601)


def test_9601_primal_box_phase1(spx):
    """k_pbox_price1<true> with k_pbox_update1<false>."""
    _run_tall(spx, "pbox_p1_9601", AT_9601)
