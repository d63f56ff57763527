"""GPU: compact pricing (Params::AS: a window's passes after its first price
from the listed rows of A, dw and the Wt rows) against the dense A stream
(SPX_DENSE_PRICE=1).  The compact sum of B_w[q,:].A_j runs in the stream's
own order, so the states are the stream's; the reduced costs join
y_w.A_j - c_j at a different place and agree within rounding.  Checked here:
the same pivot path, states within 1e-10, the same optimum.  Within compact
pricing every dispatch and geometry gives the same bits, a list that outgrows
the stored rows (SPX_CPRICE_CAP) crosses into dense pricing on the same path,
and a reset context prices like a fresh one."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def _run(spx, dense, k, calls=None, weights=False, env=None, **kw):
    """k pivots (in calls of `calls`), the state, the trace, then the solve."""
    with _env(SPX_DENSE_PRICE="1" if dense else "0", **(env or {})):
        with spx.Context(trace=4096, **kw) as ctx:
            cfg0 = ctx.config()["compact_price"]
            piv, left = 0, k
            while left > 0:
                st, piv = ctx.iterate(min(left, calls or left))
                left -= min(left, calls or left)
            s = ctx.state(binv=True)
            if weights:
                s["w"] = ctx.weights()
            tr = ctx.trace()
            r = ctx.solve()
            return piv, s, tr, r, cfg0, ctx.config()["compact_price"], ctx.ftran_cols()


def _close(a, b, tol=1e-10):
    return np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b)))


def _same_path_close(a, d, k):
    assert a[0] == d[0] == k
    assert np.array_equal(a[1]["b_ixs"], d[1]["b_ixs"])
    assert np.array_equal(a[2], d[2])  # the same (p, q) per pivot
    for key in ("x_b", "y", "binv"):
        assert _close(a[1][key], d[1][key]), key
    assert a[3].status == d[3].status and a[3].pivots == d[3].pivots
    assert abs(a[3].z - d[3].z) <= 1e-9 * abs(d[3].z)


SHAPES = [(16, 300, 1200, 5, 200), (32, 256, 1024, 7, 250), (64, 512, 2048, 1, 400)]


@functools.lru_cache(maxsize=None)
def _shape_runs(window, m, n, seed, k):
    import simplex_method_gpu_amd as spx

    kw = dict(m=m, n=n, seed=seed, window=window, persist=False)
    return _run(spx, False, k, **kw), _run(spx, True, k, **kw)


@pytest.mark.parametrize("window,m,n,seed,k", SHAPES)
def test_cprice_matches_dense_price(spx, window, m, n, seed, k):
    a, d = _shape_runs(window, m, n, seed, k)
    assert a[4] == 1 and a[5] == 1 and d[4] == 0 and d[5] == 0  # which path ran, start to optimum
    assert a[6] >= 40  # the list the compact passes read grew through several extensions
    _same_path_close(a, d, k)


def test_cprice_oracle_trace(spx, oracle):
    window, m, n, seed, k = SHAPES[0]
    a, _ = _shape_runs(window, m, n, seed, k)
    A, b, c = oracle.generate(m, n, seed)
    o = oracle.solve(A, b, c, eps=1e-7, trace_cap=4096)
    with _env(SPX_DENSE_PRICE="0"):
        with spx.Context(A, b, c, eps=1e-7, window=window, persist=False, trace=4096) as ctx:
            assert ctx.config()["compact_price"] == 1
            r = ctx.solve()
            p, q = ctx.trace()
    assert r.status == spx.SolveStatus.OptimumFound and r.pivots == o.pivots
    assert np.array_equal(p, o.trace_p) and np.array_equal(q, o.trace_q)
    assert abs(r.z - o.z) <= 1e-9 * abs(o.z)
    assert r.pivots == a[3].pivots and abs(r.z - a[3].z) <= 1e-9 * abs(o.z)  # (generated on the device: the same LP)


BITS = dict(m=400, n=1600, seed=2, window=16, persist=False)


@functools.lru_cache(maxsize=None)
def _bits_ref():
    import simplex_method_gpu_amd as spx

    return _run(spx, False, 300, **BITS)


@pytest.mark.parametrize("kw", [dict(graph_batch=-1), dict(calls=7), dict(price_block=256), dict(price_block=512),
                                dict(refactor_every=100)],
                         ids=["eager", "calls-of-7", "block256", "block512", "reinvert"])
def test_cprice_same_bits_every_dispatch(spx, kw):
    ref = _bits_ref()
    got = _run(spx, False, 300, **BITS, **kw)
    assert got[4] == 1 and got[5] == 1
    if "refactor_every" in kw:  # a reinverted B_w has its own bits: same path, close values
        assert np.array_equal(got[1]["b_ixs"], ref[1]["b_ixs"])
        assert np.array_equal(got[2], ref[2])
        for key in ("x_b", "y", "binv"):
            assert _close(got[1][key], ref[1][key], 1e-9), key
        assert got[3].pivots == ref[3].pivots and abs(got[3].z - ref[3].z) <= 1e-9 * abs(ref[3].z)
        return
    assert np.array_equal(got[2], ref[2])
    for key in ("b_ixs", "x_b", "y", "binv"):
        assert np.array_equal(got[1][key], ref[1][key]), key
    assert got[3].pivots == ref[3].pivots and got[3].z == ref[3].z


def test_cprice_reset_after_compact_passes(spx):
    """spx_reset after the list has grown: the list is empty again, and the
    compact passes of the first window (which read the lanes' runs that only a
    fold or a rebuild writes) must see no run -- the trace, the states and the
    optimum of a fresh context, bit for bit; in graph and eager dispatch."""
    ref = _bits_ref()
    for kw in (dict(), dict(graph_batch=-1)):
        with _env(SPX_DENSE_PRICE="0"):
            with spx.Context(trace=4096, **BITS, **kw) as ctx:
                ctx.iterate(120)
                assert ctx.config()["compact_price"] == 1 and ctx.ftran_cols() > 40
                ctx.reset()
                assert ctx.ftran_cols() == 0
                st, piv = ctx.iterate(300)
                s = ctx.state(binv=True)
                tr = ctx.trace()
                r = ctx.solve()
        assert piv == 300
        assert np.array_equal(tr, ref[2])
        for key in ("b_ixs", "x_b", "y", "binv"):
            assert np.array_equal(s[key], ref[1][key]), key
        assert r.status == ref[3].status and r.pivots == ref[3].pivots and r.z == ref[3].z


def test_cprice_fallback_mid_solve(spx):
    """The list outgrows the stored rows (32 of them at 512 x 2048): the solve
    crosses into dense pricing, on the uncapped run's path."""
    window, m, n, seed, k = SHAPES[2]
    a, _ = _shape_runs(window, m, n, seed, k)
    kw = dict(m=m, n=n, seed=seed, window=window, persist=False)
    c = _run(spx, False, k, calls=50, env=dict(SPX_CPRICE_CAP="32"), **kw)
    assert c[4] == 1 and c[5] == 0  # compact at the start, dense by the optimum
    assert c[6] > 32
    _same_path_close(c, a, k)
    # room for 16 pivots is needed: a cap below that prices densely from the start
    w = _run(spx, False, k, env=dict(SPX_CPRICE_CAP="8"), **kw)
    assert w[5] == 0
    _same_path_close(w, a, k)


def test_cprice_set_basis_past_cap_and_oracle(spx, oracle):
    """Warm start onto a basis whose list is past the cap (dense pricing from
    there) and onto one inside it (the rows rebuilt whole): the oracle's optimum."""
    m, n, seed = 300, 1200, 9
    A, b, c = oracle.generate(m, n, seed)
    o = oracle.solve(A, b, c, eps=1e-7)
    with spx.Context(A, b, c, window=16, persist=False) as ctx:
        ctx.iterate(150)
        basis = ctx.state()["b_ixs"].copy()
    S = int(np.sum(basis != (n - m) + np.arange(m)))  # rows whose slack is not basic in them: the rebuilt list
    assert S > 40
    for env, compact in ((dict(SPX_CPRICE_CAP=str(S - 5)), 0), ({}, 1)):
        with _env(SPX_DENSE_PRICE="0", **env):
            with spx.Context(A, b, c, window=16, persist=False) as ctx:
                assert ctx.config()["compact_price"] == 1
                ctx.set_basis(basis)
                assert ctx.ftran_cols() == S
                ctx.iterate(20)
                assert ctx.config()["compact_price"] == compact
                r = ctx.solve()
        assert r.status == spx.SolveStatus.OptimumFound
        assert abs(r.z - o.z) <= 1e-9 * abs(o.z)


def test_cprice_devex(spx):
    kw = dict(m=300, n=1200, seed=8, window=32, pricing=1, persist=False)
    a = _run(spx, False, 150, weights=True, **kw)
    d = _run(spx, True, 150, weights=True, **kw)
    assert a[4] == 1 and d[4] == 0
    assert np.array_equal(a[1]["b_ixs"], d[1]["b_ixs"])
    assert np.array_equal(a[2], d[2])
    assert _close(a[1]["w"], d[1]["w"], 1e-9)
    assert _close(a[1]["x_b"], d[1]["x_b"], 1e-9)
    assert a[3].status == d[3].status and a[3].pivots == d[3].pivots
    assert abs(a[3].z - d[3].z) <= 1e-9 * max(1.0, abs(d[3].z))


def test_cprice_steepest_edge_keeps_the_stream(spx):
    kw = dict(m=300, n=1200, seed=3, window=64, pricing=2, persist=False)
    a = _run(spx, False, 150, weights=True, **kw)
    d = _run(spx, True, 150, weights=True, **kw)
    assert a[4] == 0 and a[5] == 0
    assert np.array_equal(a[2], d[2])
    for key in ("b_ixs", "x_b", "y", "binv", "w"):
        assert np.array_equal(a[1][key], d[1][key]), key
    assert a[3].pivots == d[3].pivots and a[3].z == d[3].z
