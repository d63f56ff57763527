"""GPU: dw carried across the window fold (compact pricing; DESIGN.md §4
"Carrying dw").  A fold makes y_w += sum_t SY[t] r_t and Wt[j][t] = r_t . A_j is
stored for every column, so dw[j] += sum_t SY[t] Wt[j][t] is y_w . A_j - c_j
for the new y_w: the window opens with a compact pass instead of the dense
stream of A (an anchor), which comes back every P-th fold (SPX_DW_ANCHOR=P;
1 = every fold, 0 = never).  Only e_j depends on dw, so against anchoring at
every fold the path is the same and every state is the same bits; the anchor
count follows the rule (the first window, a stale dw, every P-th fold) however
the pivots are dispatched or chunked."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("b_ixs", "x_b", "y", "binv")


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _finish(ctx, out, weights=False):
    """the counters as the pivots left them (a state readback makes dw stale),
    then the state, the trace and the solve"""
    out["stats"] = ctx.dispatch_stats()
    out["compact"] = ctx.config()["compact_price"]
    out["state"] = ctx.state(binv=True)
    if weights:
        out["w"] = ctx.weights()
    out["trace"] = ctx.trace()
    out["solve"] = ctx.solve()
    out["stats_end"] = ctx.dispatch_stats()
    return out


def _run(spx, anchor, k, calls=None, weights=False, env=None, dense=False, **kw):
    """k pivots (in calls of `calls`) under SPX_DW_ANCHOR=anchor (None: the default period)"""
    e = dict(SPX_DENSE_PRICE="1" if dense else "0", **(env or {}))
    if anchor is not None:
        e["SPX_DW_ANCHOR"] = anchor
    with _env(**e):
        with spx.Context(trace=8192, **kw) as ctx:
            out = {"period": ctx.config()["dw_carry"], "compact0": ctx.config()["compact_price"]}
            left = k
            while left > 0:
                st, out["pivots"] = ctx.iterate(min(left, calls or left))
                left -= min(left, calls or left)
            return _finish(ctx, out, weights)


def _same_bits(a, b, what=""):
    assert a["pivots"] == b["pivots"], what
    assert np.array_equal(a["trace"], b["trace"]), what  # the same (p, q) per pivot
    for key in STATE:
        assert np.array_equal(a["state"][key], b["state"][key]), (what, key)
    assert a["solve"].status == b["solve"].status and a["solve"].pivots == b["solve"].pivots, what
    assert a["solve"].z == b["solve"].z, (what, a["solve"].z, b["solve"].z)


def _close(a, b, tol):
    return np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b)))


SHAPES = [(8, 256, 1024, 7, 250), (16, 300, 1200, 5, 200), (64, 512, 2048, 1, 400)]


@functools.lru_cache(maxsize=None)
def _shape_run(window, m, n, seed, k, anchor):
    import simplex_method_gpu_amd as spx

    return _run(spx, anchor, k, m=m, n=n, seed=seed, window=window, persist=False)


@pytest.mark.parametrize("window,m,n,seed,k", SHAPES)
def test_carry_is_anchoring_path_and_bits(spx, window, m, n, seed, k):
    ref = _shape_run(window, m, n, seed, k, 1)
    never = _shape_run(window, m, n, seed, k, 0)
    dflt = _shape_run(window, m, n, seed, k, None)
    folds = ref["stats"]["folds"]
    print(f"window {window}: folds {folds}, anchors {ref['stats']['dw_anchors']} / {never['stats']['dw_anchors']} / "
          f"{dflt['stats']['dw_anchors']}, periods {ref['period']} {never['period']} {dflt['period']}")
    assert ref["compact"] == never["compact"] == dflt["compact"] == 1
    assert (ref["period"], never["period"], dflt["period"]) == (0, -1, 32)
    assert folds >= 1 and never["stats"]["folds"] == folds and dflt["stats"]["folds"] == folds
    _same_bits(never, ref, "never")
    _same_bits(dflt, ref, "default")
    assert ref["solve"].status == spx.SolveStatus.OptimumFound
    assert never["stats"]["dw_anchors"] == 1
    assert ref["stats"]["dw_anchors"] == folds + 1
    assert dflt["stats"]["dw_anchors"] == 1 + folds // 32


def test_carry_oracle_trace(spx, oracle):
    window, m, n, seed, k = SHAPES[1]
    a = _shape_run(window, m, n, seed, k, 0)
    A, b, c = oracle.generate(m, n, seed)
    o = oracle.solve(A, b, c, eps=1e-7, trace_cap=4096)
    with _env(SPX_DENSE_PRICE="0", SPX_DW_ANCHOR="0"):
        with spx.Context(A, b, c, eps=1e-7, window=window, persist=False, trace=4096) as ctx:
            assert ctx.config()["compact_price"] == 1 and ctx.config()["dw_carry"] == -1
            r = ctx.solve()
            p, q = ctx.trace()
    assert r.status == spx.SolveStatus.OptimumFound and r.pivots == o.pivots
    assert np.array_equal(p, o.trace_p) and np.array_equal(q, o.trace_q)
    assert abs(r.z - o.z) <= 1e-9 * abs(o.z)
    assert r.pivots == a["solve"].pivots and abs(r.z - a["solve"].z) <= 1e-9 * abs(o.z)


def test_long_carry_to_the_optimum(spx):
    """every fold of a whole solve without an anchor (306 pivots at window 8:
    a fold every 7 pivots, 43 of them): the dense stream's pivots and z"""
    kw = dict(m=256, n=1024, seed=7, window=8, persist=False)
    out = {}
    for name, env in (("carry", dict(SPX_DENSE_PRICE="0", SPX_DW_ANCHOR="0")), ("dense", dict(SPX_DENSE_PRICE="1"))):
        with _env(**env):
            with spx.Context(trace=8192, **kw) as ctx:
                r = ctx.solve()
                out[name] = (r, ctx.trace(), ctx.dispatch_stats(), ctx.config()["compact_price"])
    (rc, tc, sc, cc), (rd, td, sd, cd) = out["carry"], out["dense"]
    print(f"long carry: pivots {rc.pivots} / {rd.pivots}, z {rc.z!r} / {rd.z!r}, folds {sc['folds']}, "
          f"anchors {sc['dw_anchors']}")
    assert cc == 1 and cd == 0
    assert sc["folds"] >= (rc.pivots - 9) // 7 + 1 >= 40 and sc["dw_anchors"] == 1
    assert rc.status == rd.status == spx.SolveStatus.OptimumFound
    assert rc.pivots == rd.pivots and np.array_equal(tc, td)
    assert rc.z == rd.z


BITS = dict(m=400, n=1600, seed=2, window=16, persist=False)


@functools.lru_cache(maxsize=None)
def _bits_ref():
    import simplex_method_gpu_amd as spx

    return _run(spx, 3, 300, **BITS)


@pytest.mark.parametrize("kw", [dict(graph_batch=-1), dict(calls=7), dict(price_block=256), dict(price_block=512)],
                         ids=["eager", "calls-of-7", "block256", "block512"])
def test_carry_same_bits_every_dispatch(spx, kw):
    ref = _bits_ref()
    got = _run(spx, 3, 300, **BITS, **kw)
    print(f"{kw}: anchors {got['stats']['dw_anchors']} / {ref['stats']['dw_anchors']}, folds {got['stats']['folds']}, "
          f"graph launches {got['stats']['graph_launches']} / {ref['stats']['graph_launches']}")
    assert got["compact"] == 1 and got["period"] == 3 and ref["period"] == 3
    assert ref["stats"]["graph_launches"] > 0
    _same_bits(got, ref, str(kw))
    assert got["stats"]["folds"] == ref["stats"]["folds"]
    assert got["stats"]["dw_anchors"] == ref["stats"]["dw_anchors"] == 1 + ref["stats"]["folds"] // 3
    assert got["stats_end"]["dw_anchors"] == ref["stats_end"]["dw_anchors"]


@pytest.mark.parametrize("kw", [dict(), dict(calls=7), dict(calls=5), dict(calls=1), dict(graph_batch=-1)],
                         ids=["one-call", "calls-of-7", "calls-of-5", "calls-of-1", "eager"])
def test_anchor_rule(spx, kw):
    """Period 3 at window 8: 100 pivots fold 14 times (before pass 9, then
    every 7 passes), the first window anchors and every third fold does:
    1 + 14 // 3 = 5, however the pivots are chunked."""
    got = _run(spx, 3, 100, m=256, n=1024, seed=7, window=8, persist=False, **kw)
    print(f"{kw}: folds {got['stats']['folds']}, anchors {got['stats']['dw_anchors']}")
    assert got["pivots"] == 100 and got["period"] == 3
    assert got["stats"]["folds"] == 1 + (100 - 9) // 7 == 14
    assert got["stats"]["dw_anchors"] == 5


def _twin(spx, fn):
    """fn(anchor) under the default period, never anchoring, and its SPX_DW_ANCHOR=1 twin"""
    return fn(None), fn(0), fn(1)


def _same_path_opt(spx, a, t, what, tol=None):
    assert a["pivots"] == t["pivots"], what
    assert np.array_equal(a["trace"], t["trace"]), what
    assert np.array_equal(a["state"]["b_ixs"], t["state"]["b_ixs"]), what
    for key in ("x_b", "y", "binv"):
        if tol is None:
            assert np.array_equal(a["state"][key], t["state"][key]), (what, key)
        else:
            assert _close(a["state"][key], t["state"][key], tol), (what, key)
    assert a["solve"].status == t["solve"].status == spx.SolveStatus.OptimumFound, what
    assert a["solve"].pivots == t["solve"].pivots, what
    if tol is None:
        assert a["solve"].z == t["solve"].z, what
    else:
        assert abs(a["solve"].z - t["solve"].z) <= tol * abs(t["solve"].z), what


def test_invalidation_reset(spx):
    """reset() after compact passes and carried folds: dw is stale, the first
    window anchors again, and the pivots are a fresh context's, bit for bit"""
    def fn(anchor, reset=True):
        e = dict(SPX_DENSE_PRICE="0")
        if anchor is not None:
            e["SPX_DW_ANCHOR"] = anchor
        with _env(**e):
            with spx.Context(trace=8192, **BITS) as ctx:
                out = {}
                if reset:
                    ctx.iterate(120)
                    assert ctx.config()["compact_price"] == 1 and ctx.ftran_cols() > 40
                    out["before"] = ctx.dispatch_stats()["dw_anchors"]
                    ctx.reset()
                    assert ctx.ftran_cols() == 0
                st, out["pivots"] = ctx.iterate(300)
                return _finish(ctx, out)

    d, never, twin = _twin(spx, fn)
    fresh = fn(0, reset=False)
    print(f"reset: anchors before {never['before']}, after {never['stats']['dw_anchors']}, fresh "
          f"{fresh['stats']['dw_anchors']}, twin {twin['stats']['dw_anchors']}")
    _same_bits(never, fresh, "reset vs fresh")
    _same_path_opt(spx, never, twin, "never vs twin")
    _same_path_opt(spx, d, twin, "default vs twin")
    assert never["before"] == 1 and fresh["stats"]["dw_anchors"] == 1
    assert never["stats"]["dw_anchors"] == 2  # the window after the reset, nothing else


def test_invalidation_reinversion(spx):
    """refactor_every=100: every reinversion leaves dw stale; the path of the
    run without reinversions, values within 1e-9 (a reinverted B_w has its
    own bits), and against the twin with the same reinversions the same bits"""
    def fn(anchor):
        return _run(spx, anchor, 300, refactor_every=100, **BITS)

    d, never, twin = _twin(spx, fn)
    plain = _run(spx, 0, 300, **BITS)
    print(f"reinversion: anchors {never['stats']['dw_anchors']} / {d['stats']['dw_anchors']} / "
          f"{twin['stats']['dw_anchors']}, folds {never['stats']['folds']}")
    _same_path_opt(spx, never, plain, "never vs no reinversion", 1e-9)
    _same_path_opt(spx, never, twin, "never vs twin")
    _same_path_opt(spx, d, twin, "default vs twin")
    # the first window and the one after the reinversions at 100 and 200 pivots
    # (the one at 300 ends the call)
    assert never["stats"]["dw_anchors"] == 3


def test_invalidation_set_basis(spx, oracle):
    m, n, seed = 300, 1200, 9
    A, b, c = oracle.generate(m, n, seed)
    o = oracle.solve(A, b, c, eps=1e-7)
    with spx.Context(A, b, c, window=16, persist=False) as ctx:
        ctx.iterate(150)
        basis = ctx.state()["b_ixs"].copy()

    def fn(anchor):
        e = dict(SPX_DENSE_PRICE="0")
        if anchor is not None:
            e["SPX_DW_ANCHOR"] = anchor
        with _env(**e):
            with spx.Context(A, b, c, window=16, persist=False, trace=8192) as ctx:
                out = {}
                ctx.iterate(40)  # carried folds, then the warm start
                out["before"] = ctx.dispatch_stats()["dw_anchors"]
                ctx.set_basis(basis)
                st, out["pivots"] = ctx.iterate(60)
                return _finish(ctx, out)

    d, never, twin = _twin(spx, fn)
    print(f"set_basis: anchors before {never['before']}, after {never['stats']['dw_anchors']}, twin "
          f"{twin['stats']['dw_anchors']}")
    _same_path_opt(spx, never, twin, "never vs twin")
    _same_path_opt(spx, d, twin, "default vs twin")
    assert abs(never["solve"].z - o.z) <= 1e-9 * abs(o.z)
    assert never["before"] == 1 and never["stats"]["dw_anchors"] == 2


def test_invalidation_cap_crossing(spx):
    """the list outgrows the stored rows in mid-solve (64 of them at window 8:
    several carried folds come first): dense pricing from there, on the
    twin's path"""
    window, m, n, seed, k = SHAPES[0]

    def fn(anchor):
        return _run(spx, anchor, k, calls=50, env=dict(SPX_CPRICE_CAP="64"), m=m, n=n, seed=seed, window=window,
                    persist=False)

    d, never, twin = _twin(spx, fn)
    print(f"cap: anchors {never['stats']['dw_anchors']} / {twin['stats']['dw_anchors']}, compact at the end "
          f"{never['compact']}")
    assert never["compact0"] == 1 and never["compact"] == 0 and twin["compact"] == 0
    _same_path_opt(spx, never, twin, "never vs twin")
    _same_path_opt(spx, d, twin, "default vs twin")
    # compact windows were folded before the crossing: the twin anchored at each, the carry at none
    assert never["stats"]["dw_anchors"] == 1 and twin["stats"]["dw_anchors"] >= 3


def test_invalidation_stepping(spx):
    """spx_price / spx_pivot inside a window and across a fold (which does not
    carry: dw is stale until the next fold's anchor), then iterate"""
    def fn(anchor):
        e = dict(SPX_DENSE_PRICE="0")
        if anchor is not None:
            e["SPX_DW_ANCHOR"] = anchor
        with _env(**e):
            with spx.Context(trace=8192, **BITS) as ctx:
                out = {}
                ctx.iterate(40)
                out["before"] = ctx.dispatch_stats()["dw_anchors"]
                for _ in range(3):  # inside the window
                    ctx.price()
                    ctx.pivot()
                ctx.iterate(10)
                out["mid"] = ctx.dispatch_stats()["dw_anchors"]
                for _ in range(18):  # across a fold
                    ctx.price()
                    ctx.pivot()
                st, out["pivots"] = ctx.iterate(80)
                return _finish(ctx, out)

    d, never, twin = _twin(spx, fn)
    print(f"stepping: anchors {never['before']} {never['mid']} {never['stats']['dw_anchors']}, twin "
          f"{twin['before']} {twin['mid']} {twin['stats']['dw_anchors']}")
    assert never["pivots"] == 40 + 3 + 10 + 18 + 80
    _same_path_opt(spx, never, twin, "never vs twin")
    _same_path_opt(spx, d, twin, "default vs twin")
    assert never["before"] == 1 and never["mid"] == 1  # steps inside a window leave dw valid
    assert never["stats"]["dw_anchors"] == 2  # the stepped fold left it stale: one anchor at the next fold


def test_carry_devex(spx):
    kw = dict(m=300, n=1200, seed=8, window=32, pricing=1, persist=False)
    twin = _run(spx, 1, 150, weights=True, **kw)
    for anchor in (0, None):
        a = _run(spx, anchor, 150, weights=True, **kw)
        assert a["compact"] == 1 and a["stats"]["folds"] >= 3
        assert a["stats"]["dw_anchors"] == 1 and twin["stats"]["dw_anchors"] == twin["stats"]["folds"] + 1
        assert np.array_equal(a["w"], twin["w"])
        assert np.array_equal(a["trace"], twin["trace"])
        for key in STATE:
            assert np.array_equal(a["state"][key], twin["state"][key]), key
        assert a["solve"].status == twin["solve"].status and a["solve"].pivots == twin["solve"].pivots
        assert a["solve"].z == twin["solve"].z
