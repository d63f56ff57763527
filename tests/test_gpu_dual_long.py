"""GPU: the bound-flipping (long-step) ratio test of the boxed dual simplex loop
(SPX_DUAL_RATIO_LONG_STEP, spx_set_dual_ratio, spx_get_dual_flips; DESIGN.md
§7d) on the boxed covering LPs of tests/dual_box_ref.py boxed(m, n, seed, flipc).

Golden values (tests/golden/dual_long_optima.json, written by
tests/golden/make_golden_dual_long.py): pivot count, the first 200 (p, q) pairs,
the final basis, the final at-upper set and the three flip counters of the numpy
restatement tests/dual_long_ref.py; HiGHS's optimum is the one
tests/golden/dual_box_optima.json holds for the same LP.  Over those runs the
smallest row-key gap is 1.1e-6 (1.2e-3 at the traced shapes), the smallest key
gap between consecutive candidates of a walk 3.7e-6 (1.25e-5 traced) and the
smallest |slope'| / slope of a walk decision 5.1e-4 (the generator refuses a
case below 1e-6), so neither the pivots nor the flip sets depend on the fp64
summation order.  Under the textbook ratio test the same contexts must walk
dual_box_optima.json's pivots with no flip counted.

Shapes: 7 x 20 (m below one wave), 65 x 200 (L = 128, heavy padding), 130 x 390
(m no multiple of 64), 256 x 1024 (multi-chunk columns, a multi-workgroup pricing
grid), passes with 0, 1 and up to 19 flips; 1024 x 4096 (optimum, pivots, flips
and certificate).
"""
import json
import os
import subprocess

import numpy as np
import pytest

import dual_long_ref as ref
import dual_ref
import dual_se_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9
RULES = [ref.DANTZIG, ref.STEEPEST]
RATIOS = [ref.TEXTBOOK, ref.LONG_STEP]


def _load(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden():
    """{ratio: {(m, n, seed, flipc, rule): case}} and the bound re-solve case."""
    box, lng = _load("dual_box_optima.json"), _load("dual_long_optima.json")
    key = lambda c: (c["m"], c["n"], c["seed"], c["flipc"], c["rule"])  # noqa: E731
    return {ref.TEXTBOOK: {key(c): c for c in box["cases"]}, ref.LONG_STEP: {key(c): c for c in lng["cases"]}}, \
        box["resolve"]


_LPS = {}


def _lp(m, n, seed, flipc):
    """(A_cols (n, m), b, c, u, A (m, n)) of the boxed covering LP, built once."""
    k = (m, n, seed, int(flipc))
    if k not in _LPS:
        A, b, c, u = ref.boxed(m, n, seed, bool(flipc))
        _LPS[k] = (np.ascontiguousarray(A.T), b, c, u, A)
    return _LPS[k]


def _rule(spx, rule):
    return spx.DUAL_PRICING_STEEPEST if rule == ref.STEEPEST else spx.DUAL_PRICING_DANTZIG


def _ratio(spx, ratio):
    return spx.DUAL_RATIO_LONG_STEP if ratio == ref.LONG_STEP else spx.DUAL_RATIO_TEXTBOOK


def _ctx(spx, m, n, seed, flipc, rule, ratio=ref.LONG_STEP, upper="lp", **kw):
    At, b, c, u, _ = _lp(m, n, seed, flipc)
    kw.setdefault("trace", 200)
    return spx.Context(At, b, c, window=-1, algorithm=spx.ALGO_DUAL, dual_pricing=_rule(spx, rule),
                       dual_ratio=_ratio(spx, ratio), upper=u if isinstance(upper, str) else upper, **kw)


def _check_primal(x, up, A, b, u):
    """tests/test_gpu_dual_box.py's primal checks."""
    res = float(np.max(np.abs(A @ x - b)))
    assert res <= 1e-9 * np.max(np.abs(b)), res
    assert np.min(x) >= -1e-9 and np.max(x - u) <= 1e-9, (np.min(x), np.max(x - u))
    assert np.array_equal(x[up], u[up])  # exactly the bound
    return res


def _counters(g):
    return (g.get("flips", 0), g.get("flip_passes", 0), g.get("max_flips", 0))  # (the textbook golden has none)


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
    assert flips == _counters(g), (flips, _counters(g))
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    _check_primal(x, up, A, b, u)
    assert abs(float(c @ x) - z) <= REL * abs(z)


def _solve(spx, m, n, seed, flipc, rule, ratio=ref.LONG_STEP, **kw):
    with _ctx(spx, m, n, seed, flipc, rule, ratio, **kw) as ctx:
        assert ctx.config()["dual_ratio"] == _ratio(spx, ratio)
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        flips = ctx.dual_flips()
    return r, tp.tolist(), tq.tolist(), x, up, flips


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("flipc", [0, 1])
@pytest.mark.parametrize("m,n,seed", dual_ref.TRACED)
def test_trace_parity(spx, golden, m, n, seed, flipc, rule, ratio):
    g = golden[0][ratio][(m, n, seed, flipc, rule)]
    r, tp, tq, x, up, flips = _solve(spx, m, n, seed, flipc, rule, ratio)
    print(f"{m}x{n} flipc={flipc} {rule} {ratio}: z={r.z:.13g} pivots={r.pivots} (golden {g['ref_pivots']}) "
          f"flips={flips} (golden {_counters(g)})")
    _check_against_golden(spx, g, r, tp, tq, x, up, flips, _lp(m, n, seed, flipc))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("flipc", [0, 1])
@pytest.mark.parametrize("kw", [{"global_y": True}, {"price_grid": 3}, {"refactor_every": 50}],
                         ids=["global_y", "price_grid3", "refactor50"])
def test_variants_256(spx, golden, kw, flipc, rule):
    """The global-memory ratio test and update, a three-workgroup pricing grid
    and a reinversion every 50 pivots (k_box_rhs recomputing the effective
    right-hand side the flips kept incrementally) walk the same pivots and flips."""
    m, n, seed = 256, 1024, 3
    r, tp, tq, x, up, flips = _solve(spx, m, n, seed, flipc, rule, **kw)
    print(f"{kw} flipc={flipc} {rule}: z={r.z:.13g} pivots={r.pivots} flips={flips}")
    _check_against_golden(spx, golden[0][ref.LONG_STEP][(m, n, seed, flipc, rule)], r, tp, tq, x, up, flips,
                          _lp(m, n, seed, flipc))


@pytest.mark.parametrize("rule", RULES)
def test_walk_from_global_memory(spx, golden, monkeypatch, rule):
    """k_dual_long keeps a thread's keys in registers up to 16,384 list slots;
    SPX_DUAL_LONG_GLOBAL=1 forces the path beyond that (every round reads the
    keys from global memory), which must walk the same pivots and flips."""
    m, n, seed, flipc = 256, 1024, 3, 1
    monkeypatch.setenv("SPX_DUAL_LONG_GLOBAL", "1")
    r, tp, tq, x, up, flips = _solve(spx, m, n, seed, flipc, rule)
    _check_against_golden(spx, golden[0][ref.LONG_STEP][(m, n, seed, flipc, rule)], r, tp, tq, x, up, flips,
                          _lp(m, n, seed, flipc))


@pytest.mark.parametrize("rule", RULES)
def test_stepping(spx, golden, rule):
    """The first 10 pivots one iterate(1) at a time, the rest by solve(): the
    same trace, flips and final state, and after every call A x = b holds for
    the primal vector read back (x_b, the effective right-hand side and the
    placements are consistent between calls)."""
    m, n, seed, flipc = 256, 1024, 3, 0
    _, b, c, u, A = _lp(m, n, seed, flipc)
    g = golden[0][ref.LONG_STEP][(m, n, seed, flipc, rule)]
    bmax = np.max(np.abs(b))
    seen = 0
    with _ctx(spx, m, n, seed, flipc, rule) as ctx:
        for k in range(10):
            ctx.iterate(1)
            x, up = ctx.primal()
            assert ctx.state()["pivots"] == k + 1
            assert np.max(np.abs(A @ x - b)) <= 1e-9 * bmax
            assert np.array_equal(x[up], u[up])
            f = ctx.dual_flips()
            assert f[0] >= seen
            seen = f[0]
        assert seen > 0  # some of the first 10 passes flipped
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        flips = ctx.dual_flips()
    _check_against_golden(spx, g, r, tp.tolist(), tq.tolist(), x, up, flips, _lp(m, n, seed, flipc))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("m,n,seed", [(130, 390, 2), (256, 1024, 3)])
def test_no_flip_identity(spx, m, n, seed, rule):
    """Bounds nothing can flip (every finite bound of boxed() replaced by 1e30):
    the long-step kernels give the textbook boxed pass bit for bit.  All bounds
    +inf: the unbounded context's, bit for bit (its kernels are launched)."""
    At, b, c, u, _ = _lp(m, n, seed, 0)
    big = np.where(np.isfinite(u), 1e30, u)

    def run(ratio, upper):
        with _ctx(spx, m, n, seed, 0, rule, ratio, upper=upper) as ctx:
            r = ctx.solve()
            t = [v.tolist() for v in ctx.trace()]
            x, up = ctx.primal()
            return r, t, x, up, ctx.dual_flips()

    r0, t0, x0, up0, f0 = run(ref.TEXTBOOK, big)
    r1, t1, x1, up1, f1 = run(ref.LONG_STEP, big)
    assert r0.status == spx.SolveStatus.OptimumFound and r0.pivots > 0
    assert t1 == t0 and r1.pivots == r0.pivots and r1.z == r0.z
    assert r1.b_ixs.tolist() == r0.b_ixs.tolist() and np.array_equal(r1.x_b, r0.x_b)
    assert np.array_equal(x1, x0) and np.array_equal(up1, up0)
    assert f0 == (0, 0, 0) and f1 == (0, 0, 0)
    r2, t2, x2, up2, f2 = run(ref.TEXTBOOK, None)
    r3, t3, x3, up3, f3 = run(ref.LONG_STEP, np.full(n, np.inf))
    assert t3 == t2 and r3.pivots == r2.pivots and r3.z == r2.z
    assert r3.b_ixs.tolist() == r2.b_ixs.tolist() and np.array_equal(r3.x_b, r2.x_b)
    assert np.array_equal(x3, x2) and not up3.any() and f3 == (0, 0, 0)


def test_infeasible_by_a_bound(spx):
    """x1 + x2 >= 2 with x1, x2 <= 0.5: both candidates are flipped and none
    enters; status 4 after 0 pivots, nothing flipped, no counter moved."""
    A, b, c, u = ref.tiny_box_infeasible()
    for rule in (spx.DUAL_PRICING_DANTZIG, spx.DUAL_PRICING_STEEPEST):
        with spx.Context(np.ascontiguousarray(A.T), b, c, window=-1, algorithm=spx.ALGO_DUAL, dual_pricing=rule,
                         dual_ratio=spx.DUAL_RATIO_LONG_STEP, upper=u) as ctx:
            r = ctx.solve()
            x, up = ctx.primal()
            assert r.status == spx.SolveStatus.Infeasible and r.status == 4 and r.pivots == 0, r
            assert not up.any() and ctx.dual_flips() == (0, 0, 0)
            assert r.b_ixs.tolist() == [2, 3] and np.array_equal(x, [0.0, 0.0, 4.0, -2.0])


@pytest.mark.parametrize("rule", RULES)
def test_optimum_1024(spx, golden, rule):
    """1024 x 4096: optimum, pivots and flips of the reference, and the
    certificate recomputed on the CPU from the returned basis and placements."""
    m, n, seed = dual_ref.SHAPES[4]
    At, b, c, u, A = _lp(m, n, seed, 0)
    g = golden[0][ref.LONG_STEP][(m, n, seed, 0, rule)]
    z = g["highs_z"]
    with _ctx(spx, m, n, seed, 0, rule, trace=0) as ctx:
        r = ctx.solve()
        x, up = ctx.primal()
        flips = ctx.dual_flips()
    print(f"{m}x{n} {rule}: z={r.z:.13g} (HiGHS {z:.13g}) pivots={r.pivots} (reference {g['ref_pivots']}, textbook "
          f"{g['textbook_pivots']}) flips={flips} (reference {_counters(g)})")
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    assert r.pivots == g["ref_pivots"] and flips == _counters(g)
    assert len(set(r.b_ixs.tolist())) == m
    res = _check_primal(x, up, A, b, u)
    viol, dviol, zc = ref.certificate(A, b, c, u, r.b_ixs, up)
    print(f"primal residual {res:.2e}, bound violation {viol:.2e}, reduced-cost sign violation {dviol:.2e}")
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= REL * abs(z)
    assert np.flatnonzero(up).tolist() == g["ref_at_upper"]


@pytest.mark.parametrize("rule", RULES)
def test_rule_switch(spx, golden, rule):
    """20 textbook pivots, then set_dual_ratio(LONG_STEP) and solve: the
    reference started from that basis and those placements.  And the reverse
    switch reaches HiGHS's optimum."""
    m, n, seed, flipc = 256, 1024, 3, 0
    _, b, c, u, A = _lp(m, n, seed, flipc)
    z = golden[0][ref.TEXTBOOK][(m, n, seed, flipc, rule)]["highs_z"]
    r20 = ref.dual_simplex_long(A, b, c, u, rule=rule, ratio=ref.TEXTBOOK, max_iter=20)
    want = ref.dual_simplex_long(A, b, c, u, rule=rule, basis=r20.b_ixs, at_upper=r20.at_upper)
    assert want.status == dual_ref.OPTIMUM and min(want.gap_row, want.gap_walk, want.gap_slope) >= 1e-6
    with _ctx(spx, m, n, seed, flipc, rule, ref.TEXTBOOK) as ctx:
        ctx.iterate(20)
        s = ctx.state()
        assert s["pivots"] == 20 and s["b_ixs"].tolist() == r20.b_ixs.tolist()
        assert np.array_equal(ctx.primal()[1], r20.at_upper) and ctx.dual_flips() == (0, 0, 0)
        ctx.set_dual_ratio(spx.DUAL_RATIO_LONG_STEP)
        assert ctx.config()["dual_ratio"] == spx.DUAL_RATIO_LONG_STEP
        r = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        flips = ctx.dual_flips()
    print(f"{rule}: 20 textbook pivots + {r.pivots - 20} long-step (reference {want.pivots}), flips={flips}")
    assert r.status == spx.SolveStatus.OptimumFound and r.pivots == 20 + want.pivots
    k = min(r.pivots, 200)
    assert list(zip(tp.tolist(), tq.tolist()))[20:k] == want.trace[:k - 20]
    assert r.b_ixs.tolist() == want.b_ixs.tolist() and np.array_equal(up, want.at_upper)
    assert flips == want.counters
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    _check_primal(x, up, A, b, u)
    with _ctx(spx, m, n, seed, flipc, rule, ref.LONG_STEP) as ctx:
        ctx.iterate(20)
        f20 = ctx.dual_flips()
        assert f20[0] > 0
        ctx.set_dual_ratio(spx.DUAL_RATIO_TEXTBOOK)
        r = ctx.solve()
        x, up = ctx.primal()
        assert ctx.dual_flips() == f20  # textbook passes flip nothing
    assert r.status == spx.SolveStatus.OptimumFound
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)
    _check_primal(x, up, A, b, u)


@pytest.mark.parametrize("rule", RULES)
def test_bound_resolve(spx, golden, rule):
    """The golden file's tightening re-solve (every 8th finite structural bound
    halved) under long-step: HiGHS's optimum of the tightened LP from the old basis."""
    m, n, seed = 256, 1024, 3
    res = golden[1]
    assert (res["m"], res["n"], res["seed"], res["flipc"]) == (m, n, seed, 0)
    _, b, c, u, A = _lp(m, n, seed, 0)
    u1 = u.copy()
    u1[np.where(np.isfinite(u[:n - m]))[0][::8]] *= 0.5
    with _ctx(spx, m, n, seed, 0, rule) as ctx:
        r0 = ctx.solve()
        assert r0.status == spx.SolveStatus.OptimumFound
        ctx.set_bounds(u1)
        s = ctx.state()
        assert s["status"] == spx.SolveStatus.MaxIter and s["b_ixs"].tolist() == r0.b_ixs.tolist()  # the old basis
        r1 = ctx.solve()
        x, up = ctx.primal()
    z1 = res["tight_highs_z"]
    print(f"{rule}: solve {r0.pivots} pivots; tightened: {r1.pivots - r0.pivots} more, z={r1.z:.13g} (HiGHS {z1:.13g})")
    assert r1.status == spx.SolveStatus.OptimumFound
    assert abs(r1.z - z1) <= REL * abs(z1), (r1.z, z1)
    assert r1.pivots > r0.pivots
    _check_primal(x, up, A, b, u1)


def test_weights_after_long_step_passes(spx):
    """Steepest-edge weights after 30 long-step passes: flips do not touch B^-1,
    so they are the squared row norms of numpy's inverse (1e-9 relative, the
    bound of tests/test_gpu_dual_se.py)."""
    m, n, seed = 256, 1024, 3
    At, b, c, u, _ = _lp(m, n, seed, 0)
    with _ctx(spx, m, n, seed, 0, ref.STEEPEST) as ctx:
        ctx.iterate(30)
        s = ctx.state()
        assert s["pivots"] == 30 and ctx.dual_flips()[0] > 0
        w = ctx.dual_weights()
    B = np.ascontiguousarray(At[np.asarray(s["b_ixs"], dtype=np.int64)].T)
    want = dual_se_ref.row_norms2(np.linalg.inv(B))
    err = float(np.max(np.abs(w - want) / want))
    print(f"largest relative weight error after 30 long-step passes: {err:.2e}")
    assert err <= REL, err


def test_reset_clears_counters_and_placements(spx, golden):
    m, n, seed, flipc = 130, 390, 2, 1
    g = golden[0][ref.LONG_STEP][(m, n, seed, flipc, ref.DANTZIG)]
    with _ctx(spx, m, n, seed, flipc, ref.DANTZIG) as ctx:
        r = ctx.solve()
        assert ctx.dual_flips() == _counters(g) and ctx.primal()[1].any()
        ctx.reset()
        assert ctx.dual_flips() == (0, 0, 0)
        assert not ctx.primal()[1].any()  # every column back at lower
        r2 = ctx.solve()
        tp, tq = ctx.trace()
        x, up = ctx.primal()
        _check_against_golden(spx, g, r2, tp.tolist(), tq.tolist(), x, up, ctx.dual_flips(), _lp(m, n, seed, flipc))
        assert r2.z == r.z


def test_errors(spx):
    m, n, seed = 7, 20, 0
    At, b, c, u, _ = _lp(m, n, seed, 0)
    with pytest.raises(ValueError):
        spx.Context(At, b, c, window=-1, algorithm=spx.ALGO_DUAL, dual_ratio=2)
    with _ctx(spx, m, n, seed, 0, ref.DANTZIG, ref.TEXTBOOK) as ctx:
        for bad in (2, -1):
            with pytest.raises(spx.SimplexError) as ei:
                ctx.set_dual_ratio(bad)
            assert ei.value.code == -1 and "ratio" in str(ei.value)
        assert ctx.config()["dual_ratio"] == spx.DUAL_RATIO_TEXTBOOK  # the refused calls changed nothing
        assert ctx.solve().status == spx.SolveStatus.OptimumFound and ctx.dual_flips() == (0, 0, 0)
    # valid on a context that runs the primal loop, like spx_set_dual_pricing
    A0, b0, c0 = dual_ref.covering(m, n, seed)
    with spx.Context(np.ascontiguousarray(A0.T), np.abs(b0), c0, window=-1) as ctx:
        ctx.set_dual_ratio(spx.DUAL_RATIO_LONG_STEP)
        assert ctx.dual_flips() == (0, 0, 0)


def test_cli_dual_ratio(golden, tmp_path):
    """./solver --dual --bounds FILE --dual-ratio long --json: the reference's pivots and flips."""
    m, n, seed, flipc = 65, 200, 1, 0
    _, b, c, u, A = _lp(m, n, seed, flipc)
    p = str(tmp_path / "cover.txt")
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
    for rule in RULES:
        r = subprocess.run([solver, "--dual", "--dual-pricing", rule, "--bounds", pb, "--dual-ratio", "long", "--json",
                            "--no-iter-lines", p], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        js = json.loads(r.stdout.splitlines()[-1])
        g = golden[0][ref.LONG_STEP][(m, n, seed, flipc, rule)]
        assert js["status"] == 1 and js["pivots"] == g["ref_pivots"] and js["dual_ratio"] == "long"
        assert (js["flips"], js["flip_passes"], js["max_flips"]) == _counters(g)
        assert abs(js["z"] - g["highs_z"]) <= REL * abs(g["highs_z"])
