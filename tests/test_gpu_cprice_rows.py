"""GPU: the row form of compact pricing's operand fetch (spx_cprows.h: a
column's listed entries of AS read as coalesced chunks and handed to the lanes
through the wave's LDS slot) against the gather form (SPX_CPRICE_ROWS=0: every
lane fetches its own terms).  Both put the same operands into the same fma
chain, so every state is compared bit for bit: the trace, b_ixs, x_b, y,
B^-1, and the solve's pivots and z.  Covered: every dispatch, the tier edges
(the limit below, at and above a chunk boundary, and a list that outgrows the
limit mid-solve), a pitch of AS that is odd or no multiple of 64, lists of
hundreds of rows whose lanes' runs pass the 8 terms held in registers, the
empty list after a reset, and Devex."""
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


def _run(spx, rows, k, calls=None, weights=False, env=None, args=(), basis=None, reset_after=0, solve_max=None, **kw):
    """k pivots (in calls of `calls`), the state, the trace, then the solve (to
    the optimum, or solve_max pivots in all); rows: SPX_CPRICE_ROWS (None: the
    default)."""
    e = dict(SPX_DENSE_PRICE="0", **(env or {}))
    if rows is not None:
        e["SPX_CPRICE_ROWS"] = rows
    with _env(**e):
        with spx.Context(*args, trace=4096, persist=False, **kw) as ctx:
            info = dict(cfg0=ctx.config()["compact_price"], rows=ctx.cprice_rows())
            if basis is not None:
                ctx.set_basis(basis)
                info["cols0"] = ctx.ftran_cols()
            if reset_after:
                ctx.iterate(reset_after)
                info["cols_before_reset"] = ctx.ftran_cols()
                ctx.reset()
                info["cols0"] = ctx.ftran_cols()
            piv, left = 0, k
            while left > 0:
                st, piv = ctx.iterate(min(left, calls or left))
                left -= min(left, calls or left)
            s = ctx.state(binv=True)
            if weights:
                s["w"] = ctx.weights()
            info["cols_k"] = ctx.ftran_cols()
            info["cfg_k"] = ctx.config()["compact_price"]
            tr = ctx.trace()
            r = ctx.solve() if solve_max is None else ctx.solve(solve_max)
            info["cols"] = ctx.ftran_cols()
            return piv, s, tr, r, info


def _same_bits(got, ref, weights=False):
    assert got[0] == ref[0]
    assert np.array_equal(got[2], ref[2])  # the same (p, q) per pivot
    for key in ("b_ixs", "x_b", "y", "binv") + (("w",) if weights else ()):
        assert np.array_equal(got[1][key], ref[1][key]), key
    assert got[3].status == ref[3].status and got[3].pivots == ref[3].pivots and got[3].z == ref[3].z
    assert got[4]["cols_k"] == ref[4]["cols_k"] and got[4]["cols"] == ref[4]["cols"]


BITS = dict(m=400, n=1600, seed=2, window=16)


@functools.lru_cache(maxsize=None)
def _bits_gather():
    import simplex_method_gpu_amd as spx

    return _run(spx, 0, 300, **BITS)


@pytest.mark.parametrize("kw", [dict(), dict(graph_batch=-1), dict(calls=7)], ids=["graph", "eager", "calls-of-7"])
def test_rows_same_bits_every_dispatch(spx, kw):
    ref = _bits_gather()
    got = _run(spx, None, 300, **BITS, **kw)
    assert ref[4]["cfg0"] == 1 and ref[4]["cfg_k"] == 1 and got[4]["cfg0"] == 1 and got[4]["cfg_k"] == 1
    assert ref[0] == 300
    # m = 400: 512 rows of AS, the default limit; a slot of 8 chunks of 64
    # doubles and the unit entry's pair
    assert got[4]["rows"] == {"rows": 512, "slot_bytes": 8 * (512 + 2)}
    assert ref[4]["rows"] == {"rows": 0, "slot_bytes": 0}
    assert 0 < ref[4]["cols_k"] <= 512  # the row form priced every compact pass
    _same_bits(got, ref)


EDGE = dict(m=512, n=2048, seed=1, window=64)


@functools.lru_cache(maxsize=None)
def _edge_gather():
    import simplex_method_gpu_amd as spx

    return _run(spx, 0, 400, **EDGE)


@pytest.mark.parametrize("limit", [1, 63, 64, 65, 128, 129])
def test_rows_tier_edges(spx, limit):
    """The limit on either side of a multiple of 64.  The list of this solve
    grows window by window to 95 rows after 400 pivots (105 at the optimum;
    asserted past 65 on the gather run, which this change does not touch), so
    the limits up to 65 see the solve cross from the row form to the gather
    form.  Every list of up to 128 rows is read as 2 chunks, so 64 / 65 cross
    no chunk step, and with 128 / 129 only the slot's size differs here: the
    list never passes 128.  The 4- and 8-chunk loops are run by
    test_rows_forced_list and test_rows_devex_forced_list."""
    ref = _edge_gather()
    got = _run(spx, limit, 400, **EDGE)
    slot = 8 * (64 * (2 if limit <= 128 else 4) + 2)
    assert got[4]["rows"] == {"rows": limit, "slot_bytes": slot}
    print("list after 400 pivots / at the optimum:", ref[4]["cols_k"], ref[4]["cols"])
    assert ref[4]["cfg_k"] == 1 and got[4]["cfg_k"] == 1
    if limit <= 65:
        assert got[4]["cols_k"] > limit  # crossed into the gather form
    _same_bits(got, ref)


@pytest.mark.parametrize("cap", [33, 40])
def test_rows_odd_and_tiny_pitch(spx, cap):
    """SPX_CPRICE_CAP = 33 / 40: the pitch of AS is odd / no multiple of 64, the
    limit is clamped to it, and the last column's row ends the allocation."""
    env = dict(SPX_CPRICE_CAP=cap)
    ref = _run(spx, 0, 300, calls=50, env=env, **BITS)
    got = _run(spx, None, 300, calls=50, env=env, **BITS)
    assert got[4]["rows"] == {"rows": cap, "slot_bytes": 8 * (128 + 2)}
    assert got[4]["cfg0"] == 1 and ref[4]["cfg0"] == 1
    _same_bits(got, ref)


def test_rows_warm_start_long_list(spx, oracle):
    """The warm start of test_cprice_set_basis_past_cap_and_oracle: the rows of
    AS rebuilt whole for a list of more than 40 rows."""
    m, n, seed = 300, 1200, 9
    A, b, c = oracle.generate(m, n, seed)
    with spx.Context(A, b, c, window=16, persist=False) as ctx:
        ctx.iterate(150)
        basis = ctx.state()["b_ixs"].copy()
    S = int(np.sum(basis != (n - m) + np.arange(m)))
    assert S > 40
    ref = _run(spx, 0, 60, args=(A, b, c), basis=basis, window=16)
    got = _run(spx, None, 60, args=(A, b, c), basis=basis, window=16)
    assert ref[4]["cols0"] == S and got[4]["cols0"] == S
    assert got[4]["cfg_k"] == 1
    _same_bits(got, ref)


def _struct_basis(m, n, S):
    """Structural column i basic in row i for i < S, the slack elsewhere: the
    list is the rows 0 .. S-1, and lane l of the stream holds the rows 2 l,
    2 l + 1 (mod 128): S / 64 of them."""
    b = (n - m) + np.arange(m, dtype=np.int64)
    b[:S] = np.arange(S)
    return b


@pytest.mark.parametrize("m,S,nc", [(1024, 150, 4), (2048, 300, 8), (2048, 490, 8), (2560, 600, 0)])
def test_rows_forced_list(spx, m, S, nc):
    """A list forced long by a warm start (the construction of
    profiles/cprice_cap_probe.txt): 150 rows read as 4 chunks, 300 and 490 as
    8 chunks, two columns in flight.  At 490 the lanes 0 .. 52 hold 8 listed
    rows each, so their unit entry, and every row a fold appends to them, is a
    ninth term and later: the rest of the run, read from the slot.  600 rows
    (of 640 stored at m = 2560) are past the limit of 512: the gather form,
    runs of 9 and 10 terms.  Such a basis is far from primal feasible (x_b down
    to -4e6), so the primal loop has no optimum to reach from it and the solve
    is held to 120 pivots: the bits of every pass are what is compared."""
    n = 2 * m
    basis = _struct_basis(m, n, S)
    kw = dict(m=m, n=n, seed=0, window=16, basis=basis, solve_max=120)
    ref = _run(spx, 0, 40, **kw)
    got = _run(spx, None, 40, **kw)
    assert got[4]["rows"]["rows"] == 512
    assert ref[4]["cols0"] == S and got[4]["cols0"] == S
    print("pivots", ref[0], "list after them", ref[4]["cols_k"], "solve", ref[3].status, ref[3].pivots, ref[4]["cols"])
    assert ref[0] == 40 and ref[4]["cols_k"] > S  # the passes ran and the list grew
    assert got[4]["cfg0"] == 1
    if nc == 4:
        assert 128 < S and got[4]["cols_k"] <= 256
    elif nc == 8:
        assert 256 < S and got[4]["cols_k"] <= 512 + 15
    else:
        assert S > 512
    _same_bits(got, ref)


def test_rows_empty_list_after_reset(spx):
    """reset() after 120 pivots: the first window's compact passes price with
    an empty list (S = 0: the gather form, which reads no run)."""
    ref = _bits_gather()
    for kw in (dict(), dict(graph_batch=-1)):
        got = _run(spx, None, 300, reset_after=120, **BITS, **kw)
        assert got[4]["cols_before_reset"] > 40 and got[4]["cols0"] == 0
        _same_bits(got, ref)


def test_rows_devex(spx):
    kw = dict(m=300, n=1200, seed=8, window=32, pricing=1)
    ref = _run(spx, 0, 150, weights=True, **kw)
    got = _run(spx, None, 150, weights=True, **kw)
    assert got[4]["cfg0"] == 1 and ref[4]["cfg0"] == 1
    _same_bits(got, ref, weights=True)


@pytest.mark.parametrize("m,S", [(1024, 150), (2048, 300)])
def test_rows_devex_forced_list(spx, m, S):
    """Devex on the forced lists of 150 and 300 rows: the Devex loops of 4 and
    of 8 chunks (test_rows_devex reaches 2 chunks only)."""
    n = 2 * m
    kw = dict(m=m, n=n, seed=0, window=16, pricing=1, basis=_struct_basis(m, n, S), solve_max=120, weights=True)
    ref = _run(spx, 0, 40, **kw)
    got = _run(spx, None, 40, **kw)
    assert ref[4]["cols0"] == S and got[4]["cfg0"] == 1
    assert ref[0] == 40 and S < ref[4]["cols_k"] <= (256 if S == 150 else 512)
    _same_bits(got, ref, weights=True)
