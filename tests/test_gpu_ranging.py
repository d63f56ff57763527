"""GPU: sensitivity ranging at the optimum (spx_ranging_cost, spx_ranging_rhs,
spx_ranging_times; k_rng_gather, k_rng_cost, k_rng_cost_min, k_rng_rhs,
k_rng_rhs_min).

The kernels against the numpy restatement (tests/ranging_ref.py), computed in
longdouble from the device's own optimum: the basis and the placements, and B^-1,
y and x_b as spx_get_state returns them.  Values are compared within an a-priori
bound, not a chosen tolerance.  With eps = 2^-53, for the entry (i, k) that wins
a row's minimum,

    e_T = 8 m eps sum_t |rho_it| |A_tk|        (the dot T_ik in any summation order, fused or not)
    e_d = 8 m eps sum_t |y_t| |A_tk|           (the dot d_k, likewise)
    |ratio_device - ratio| <= 4 (e_d + ratio e_T) / |g|

(a quotient s / g with errors e_d in s and e_T in g moves by (e_d + ratio e_T) /
|g| to first order; the division and the reference's own rounding are inside
the factor 4).  A non-basic column's own range is s_j: 4 e_d.  Right-hand side:
beta is an entry of the same B^-1 and x_b the same vector, bit for bit, so the
ratio is one subtraction and one division away: 8 eps ratio; a lower-shifted
context adds 4 e_x / |beta| with e_x = 4 eps (|x_b| + |l|), for the lower bound
spx_get_state added and this test subtracted again.  Where the device's winner
is another entry than the restatement's (allowed only under the runner-up
exemption below) that entry's bound is added.  The largest measured share of the
bound is printed per case.

Indices are compared only where the restatement's runner-up is at least (1 + 1e-6)
x the minimum; the case builder (ranging_ref.refuse_case) refuses an LP with an
entry of T or B^-1 within [tol / 2, 2 tol], or with more than 5 % of its rows or
columns under that exemption, and runs here on the device's optimum again.

The semantics through the library's own re-solve: c_j (SPX_ALGO_PRIMAL_BOX) or b_r
(SPX_ALGO_DUAL) moved to 0.999 of a reported limit makes no pivot and no flip; to
1.001, the first pass enters the reported column / the first pivot's row is the
reported one.  Probes have 0.001 Lambda |g*| > 10 eps (the pricing tolerance) or
0.001 Lambda |beta*| > 10 feas_tol, so the loop's own tolerances cannot hide or
fake the change.
"""
import os
import subprocess

import numpy as np
import pytest

import primal_box_ref
import ranging_ref as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS53 = 2.0 ** -53
TOL = 1e-9      # the contexts' piv_tol (the default)
EPS = 1e-7      # their pricing tolerance
FEAS = 1e-9     # and feasibility tolerance

_LPS = {}


def _lp(kind, m, n, seed):
    k = (kind, m, n, seed)
    if k not in _LPS:
        _LPS[k] = rr.build_lp(kind, m, n, seed)
    return _LPS[k]


def _ctx(spx, kind, lp, c=None, b=None, **kw):
    A, b0, c0, l, u = lp
    At = np.ascontiguousarray(A.T)
    kw.setdefault("trace", 4096)
    kw.setdefault("window", -1)
    b = b0 if b is None else b
    c = c0 if c is None else c
    if kind == "dual":
        return spx.Context(At, b, c, algorithm=spx.ALGO_DUAL, upper=u, **kw)
    if kind == "primal":
        return spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, **kw)
    return spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, lower=l, upper=u, primal_phase1=True, **kw)


def _device_ref(ctx, lp):
    """The restatement in longdouble from the device's optimum, and what the bounds need."""
    A, b, c, l, u = lp
    n = A.shape[1]
    s = ctx.state(binv=True)
    _, up = ctx.primal()
    fr = np.zeros(n, dtype=bool) if l is None else np.isneginf(l)
    lsh = np.zeros(n) if l is None else np.where(fr, 0.0, l)
    rng = np.where(np.isfinite(u), u - lsh, np.inf)
    bix = s["b_ixs"]
    xs = s["x_b"] - lsh[bix]
    cost, rhs = rr.both(A, c, bix, up, s["binv"], s["y"], xs, rng, fr, tol=TOL, dtype=np.longdouble)
    e_x = 4.0 * EPS53 * (np.abs(s["x_b"]) + np.abs(lsh[bix])) * (lsh[bix] != 0.0)
    return s, up, fr, cost, rhs, e_x


def _compare_cost(A, s, cost, got):
    """(worst |device - restatement| / bound, indices compared, indices exempt); asserts the infinities and indices."""
    m, n = A.shape
    S, y = np.abs(s["binv"]), np.abs(s["y"])
    Aa = np.abs(A)
    e_T = 8.0 * m * EPS53 * (S @ Aa[:, cost.nb])
    e_d = 8.0 * m * EPS53 * (y @ Aa)
    pos_of = np.full(n, -1)
    pos_of[cost.nb] = np.arange(len(cost.nb))
    worst, compared, skipped = 0.0, 0, 0

    def entry_bound(i, k, ratio):
        p = pos_of[k]
        t = float(cost.T[i, p])
        g = t if cost.sigma[k] == 0.0 else float(cost.sigma[k]) * t
        return 4.0 * (e_d[k] + ratio * e_T[i, p]) / abs(g)

    for j in range(n):
        i = cost.row_of[j]
        for ref, sec, kref, dev, kdev in ((cost.down[j], cost.second_down[j], cost.block_down[j], got.down[j],
                                           got.block_down[j]),
                                          (cost.up[j], cost.second_up[j], cost.block_up[j], got.up[j], got.block_up[j])):
            if not np.isfinite(ref):
                assert np.isinf(dev) and dev > 0 and kdev == -1 and kref == -1, (j, dev, kdev)
                continue
            ref = float(ref)
            assert np.isfinite(dev) and dev >= 0.0 and kdev >= 0, (j, ref, dev, kdev)
            if i < 0:  # non-basic: its own reduced cost
                assert kdev == j == kref
                bound = 4.0 * e_d[j]
                if ref == 0.0 and dev == 0.0:
                    continue
            else:
                bound = entry_bound(i, kref, ref)
                if rr.exempt(ref, sec):
                    skipped += 1
                    if kdev != kref:
                        assert pos_of[kdev] >= 0
                        bound += entry_bound(i, kdev, ref)
                else:
                    compared += 1
                    assert kdev == kref, (j, i, ref, float(sec), kref, kdev)
            share = abs(dev - ref) / bound if bound > 0.0 else (0.0 if dev == ref else np.inf)
            worst = max(worst, share)
    return worst, compared, skipped


def _compare_rhs(s, rhs, got, e_x):
    m = len(rhs.down)
    S = s["binv"]
    worst, compared, skipped = 0.0, 0, 0
    for r in range(m):
        for ref, sec, kref, dev, kdev in ((rhs.down[r], rhs.second_down[r], rhs.leave_down[r], got.down[r],
                                           got.leave_down[r]),
                                          (rhs.up[r], rhs.second_up[r], rhs.leave_up[r], got.up[r], got.leave_up[r])):
            if not np.isfinite(ref):
                assert np.isinf(dev) and dev > 0 and kdev == -1 and kref == -1, (r, dev, kdev)
                continue
            ref = float(ref)
            assert np.isfinite(dev) and dev >= 0.0 and 0 <= kdev < 2 * m, (r, ref, dev, kdev)
            bound = 8.0 * EPS53 * ref + 4.0 * e_x[kref // 2] / abs(S[kref // 2, r])
            if rr.exempt(ref, sec):
                skipped += 1
                if kdev != kref:
                    bound += 4.0 * e_x[kdev // 2] / abs(S[kdev // 2, r])
            else:
                compared += 1
                assert kdev == kref, (r, ref, float(sec), kref, kdev)
            share = abs(dev - ref) / bound if bound > 0.0 else (0.0 if dev == ref else np.inf)
            worst = max(worst, share)
    return worst, compared, skipped


@pytest.mark.parametrize("kind,m,n,seed", rr.CASES)
def test_kernels_against_restatement(spx, kind, m, n, seed):
    """7 x 20 (m < 16), 65 x 200 (one row past 64), 130 x 390 (two row blocks,
    three column tiles, a ragged last tile both ways), 256 x 1024 (tile-exact);
    after a bounded primal solve, a boxed dual solve, and general_lu with free
    and lower-shifted columns through phase 1."""
    lp = _lp(kind, m, n, seed)
    A = lp[0]
    with _ctx(spx, kind, lp) as ctx:
        r = ctx.solve()
        assert r.status == spx.SolveStatus.OptimumFound
        gc = ctx.cost_ranging()
        gr = ctx.rhs_ranging()
        s, up, fr, cost, rhs, e_x = _device_ref(ctx, lp)
        assert s["pivots"] == r.pivots and s["status"] == spx.SolveStatus.OptimumFound
    assert rr.refuse_case(cost, rhs, s["binv"], TOL) == []
    wc, cc, sc = _compare_cost(A, s, cost, gc)
    wr, cr, sr = _compare_rhs(s, rhs, gr, e_x)
    nslack = int(np.sum(cost.nb >= n - m))
    print(f"{kind} {m}x{n}: {r.pivots} pivots, {int(up.sum())} columns at upper, {nslack} non-basic slacks, "
          f"{int(fr.sum())} free columns; cost: worst error / bound = {wc:.3g}, {cc} indices compared, {sc} exempt; "
          f"rhs: worst error / bound = {wr:.3g}, {cr} compared, {sr} exempt")
    assert nslack > 0 and cc > 0 and cr > 0
    assert sc <= rr.SHARE * 2 * m and sr <= rr.SHARE * 2 * m
    assert wc <= 1.0, wc
    assert wr <= 1.0, wr


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_tiny_exact_tie(spx):
    """Columns 1 and 2 are identical: their ratios tie exactly in both rows and
    the smaller column is reported, wherever the two sit on the non-basic list."""
    A, b, c, u, basis = rr.tiny_tie()
    with spx.Context(np.ascontiguousarray(A.T), b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, window=-1) as ctx:
        r = ctx.solve()
        assert r.status == spx.SolveStatus.OptimumFound and sorted(r.b_ixs.tolist()) == sorted(basis)
        g = ctx.cost_ranging()
        h = ctx.rhs_ranging()
    assert g.down[0] == 2.0 and g.down[4] == 2.0 and g.block_down[0] == 1 and g.block_down[4] == 1
    assert np.isinf(g.up[0]) and g.block_up[0] == -1 and np.isinf(g.up[4]) and g.block_up[4] == -1
    assert g.up[1:4].tolist() == [2.0, 2.0, 3.0] and g.block_up[1:4].tolist() == [1, 2, 3]
    assert np.all(np.isinf(g.down[1:4])) and g.block_down[1:4].tolist() == [-1, -1, -1]
    row = {int(j): i for i, j in enumerate(r.b_ixs)}
    assert h.down[0] == 4.0 and h.leave_down[0] == 2 * row[0] and h.down[1] == 5.0 and h.leave_down[1] == 2 * row[4]
    assert np.all(np.isinf(h.up)) and h.leave_up.tolist() == [-1, -1]


def test_tiny_free_column_blocks_both_ways(spx):
    """A free column left non-basic at the optimum (reduced cost exactly 0) with
    T = (1, 1): both basic columns' costs are blocked at 0 in both directions."""
    A, b, c, l, u, basis = rr.tiny_free()
    with spx.Context(np.ascontiguousarray(A.T), b, c, algorithm=spx.ALGO_PRIMAL_BOX, lower=l, upper=u, window=-1) as ctx:
        r = ctx.solve()
        assert r.status == spx.SolveStatus.OptimumFound and sorted(r.b_ixs.tolist()) == sorted(basis)
        g = ctx.cost_ranging()
        h = ctx.rhs_ranging()
    for j in basis + [3]:
        assert g.down[j] == 0.0 and g.up[j] == 0.0 and g.block_down[j] == 3 and g.block_up[j] == 3, j
    assert g.up[1] == 2.0 and g.block_up[1] == 1
    assert h.down.tolist() == [4.0, 5.0]


def test_bit_for_bit_across_calls_and_options(spx, monkeypatch):
    """Two calls in a row, a three-workgroup pricing grid, y in global memory and
    a 1000-byte LDS cap: the same bits (the geometry is a function of m and n)."""
    kind, m, n, seed = "primal", 130, 390, 2
    lp = _lp(kind, m, n, seed)
    got = []
    for kw, env in (({}, None), ({"price_grid": 3}, None), ({"global_y": True}, None), ({}, "1000")):
        if env:
            monkeypatch.setenv("SPX_PBOX_LDS_CAP", env)
        with _ctx(spx, kind, lp, **kw) as ctx:
            assert ctx.solve().status == spx.SolveStatus.OptimumFound
            c1, r1 = ctx.cost_ranging(), ctx.rhs_ranging()
            c2, r2 = ctx.cost_ranging(), ctx.rhs_ranging()
            assert _same(c1, c2) and _same(r1, r2), kw
            got.append((c1, r1, ctx.state()["b_ixs"]))
        if env:
            monkeypatch.delenv("SPX_PBOX_LDS_CAP")
    for c1, r1, bix in got[1:]:
        assert np.array_equal(bix, got[0][2])
        assert _same(c1, got[0][0]) and _same(r1, got[0][1])


def test_bit_for_bit_across_histories(spx):
    """The answer is a function of the basis and the placements: after
    refactor_every=7 (another pivot history to the same basis) and after
    spx_set_basis (the non-basic list rebuilt in ascending order) the results
    are the bits of the plain solve's, once each context's B^-1 is the
    reinversion of that basis (a B^-1 kept by rank-1 updates has other bits)."""
    kind, m, n, seed = "primal", 130, 390, 2
    lp = _lp(kind, m, n, seed)
    with _ctx(spx, kind, lp) as a, _ctx(spx, kind, lp, refactor_every=7) as b:
        ra, rb = a.solve(), b.solve()
        assert ra.status == rb.status == spx.SolveStatus.OptimumFound
        if not (np.array_equal(ra.b_ixs, rb.b_ixs) and np.array_equal(a.primal()[1], b.primal()[1])):
            pytest.skip("refactor_every=7 took another path to the optimum: another basis order")
        a.reinvert()
        b.reinvert()
        ca, ha = a.cost_ranging(), a.rhs_ranging()
        cb, hb = b.cost_ranging(), b.rhs_ranging()
        assert _same(ca, cb) and _same(ha, hb)
        # the same basis through spx_set_basis: placements kept, list ascending, no pivot to the optimum
        a.set_basis(ra.b_ixs)
        with pytest.raises(spx.SimplexError) as ei:
            a.cost_ranging()  # (set since the optimum: refused until solved again)
        assert ei.value.code == -5
        r2 = a.solve()
        assert r2.status == spx.SolveStatus.OptimumFound and r2.pivots == ra.pivots
        assert np.array_equal(r2.b_ixs, ra.b_ixs)
        a.reinvert()  # (x_b as the reinversion forms it, as above; the list stays ascending)
        c2, h2 = a.cost_ranging(), a.rhs_ranging()
        assert _same(ca, c2) and _same(ha, h2)


def test_ranging_leaves_the_loop_state_alone(spx):
    """Steepest edge, 130 x 390.  A context that ranges (refused with a pivot and
    a recurrence pending after iterate(40); answered at the optimum, where the
    last pivot is still pending in B^-1) and one that never asks: the same
    trace, and after set_cost and 40 more pivots the same B^-1, x_b, y and
    weights, bit for bit."""
    kind, m, n, seed = "primal", 130, 390, 2
    lp = _lp(kind, m, n, seed)
    c2 = primal_box_ref.cost_variant(lp[2], n - m, seed)
    out = []
    for ask in (False, True):
        with _ctx(spx, kind, lp, primal_pricing=spx.PRIMAL_PRICING_STEEPEST, timing=True) as ctx:
            st, piv = ctx.iterate(40)
            assert piv == 40 and st == spx.SolveStatus.MaxIter
            if ask:
                for call in (ctx.cost_ranging, ctx.rhs_ranging):
                    with pytest.raises(spx.SimplexError) as ei:
                        call()
                    assert ei.value.code == -5 and "optimum" in str(ei.value)
                assert ctx.ranging_times() == ((0.0, 0.0), (0, 0))
            r = ctx.solve()
            assert r.status == spx.SolveStatus.OptimumFound
            if ask:
                ctx.cost_ranging()
                ctx.rhs_ranging()
                (tc, tr), launches = ctx.ranging_times()
                assert launches == (1, 1) and tc > 0.0 and tr > 0.0
                assert ctx.ranging_times() == ((0.0, 0.0), (0, 0))
            else:
                assert ctx.ranging_times() == ((0.0, 0.0), (0, 0))
            ctx.set_cost(c2)
            st, piv = ctx.iterate(40)
            assert piv == r.pivots + 40
            tp, tq = ctx.trace()
            out.append((tp.tolist(), tq.tolist(), ctx.state(binv=True), ctx.primal_weights(), ctx.primal()[1],
                        ctx.primal_flips()))
    a, b = out
    assert a[0] == b[0] and a[1] == b[1] and a[5] == b[5]
    assert np.array_equal(a[2]["b_ixs"], b[2]["b_ixs"]) and np.array_equal(a[4], b[4])
    for key in ("x_b", "y", "binv"):
        assert np.array_equal(a[2][key], b[2][key]), key
    nb = np.ones(n, dtype=bool)
    nb[a[2]["b_ixs"]] = False
    assert np.array_equal(a[3][nb], b[3][nb])


# ---------------------------------------------------------------------------------------------------------------------
# the semantics through the library's own re-solve

def _pick(cands, count):
    """`count` of the candidates, spread over the list."""
    cands = list(cands)
    if len(cands) <= count:
        return cands
    return [cands[int(round(k * (len(cands) - 1) / (count - 1)))] for k in range(count)]


def test_cost_limits_through_the_primal_resolve(spx):
    kind, m, n, seed = "primal", 65, 200, 1
    lp = _lp(kind, m, n, seed)
    A, b, c, l, u = lp
    with _ctx(spx, kind, lp) as ctx:
        r0 = ctx.solve()
        assert r0.status == spx.SolveStatus.OptimumFound
        g = ctx.cost_ranging()
        s, up, fr, cost, rhs, _ = _device_ref(ctx, lp)
    pos_of = np.full(n, -1)
    pos_of[cost.nb] = np.arange(len(cost.nb))
    basic, nonbasic = [], []
    for j in range(n):
        i = cost.row_of[j]
        for sign, lim, blk, ref, sec in ((-1.0, g.down[j], g.block_down[j], cost.down[j], cost.second_down[j]),
                                         (1.0, g.up[j], g.block_up[j], cost.up[j], cost.second_up[j])):
            if not np.isfinite(lim):
                continue
            gstar = 1.0 if i < 0 else abs(float(cost.T[i, pos_of[blk]]))
            # the margin rule, and a runner-up beyond 1.001 Lambda: past the limit only the blocker prices out
            if 0.001 * lim * gstar > 10.0 * EPS and (i < 0 or float(sec) > 1.01 * float(ref)):
                (nonbasic if i < 0 else basic).append((j, sign, float(lim), int(blk)))
    probes = _pick(basic, 5) + _pick(nonbasic, 4)
    assert len(probes) >= 8 and {p[1] for p in probes} == {-1.0, 1.0}
    for j, sign, lim, blk in probes:
        with _ctx(spx, kind, lp) as ctx:
            r = ctx.solve()
            assert r.pivots == r0.pivots and np.array_equal(r.b_ixs, r0.b_ixs)
            flips = ctx.primal_flips()
            c1 = c.copy()
            c1[j] += sign * 0.999 * lim
            ctx.set_cost(c1)
            r1 = ctx.solve()
            assert r1.status == spx.SolveStatus.OptimumFound
            assert r1.pivots == r0.pivots and ctx.primal_flips() == flips, (j, sign, lim)
            up0 = ctx.primal()[1]
            c2 = c.copy()
            c2[j] += sign * 1.001 * lim
            ctx.set_cost(c2)
            st, piv = ctx.iterate(1)
            f2 = ctx.primal_flips()
            assert piv > r0.pivots or f2[0] > flips[0], (j, sign, lim)  # at least one pass did something
            if f2[0] == flips[0]:
                assert ctx.trace()[0][r0.pivots] == blk, (j, sign, blk, ctx.trace()[0][r0.pivots])
            else:  # the first pass was a flip of the entering column: the blocker changed sides
                up1 = ctx.primal()[1]
                assert up1[blk] != up0[blk] or (piv > r0.pivots and ctx.trace()[0][r0.pivots] == blk), (j, sign, blk)
    print(f"cost limits: {len(probes)} probes, {sum(1 for p in probes if cost.row_of[p[0]] >= 0)} on basic columns")


def test_rhs_limits_through_the_dual_resolve(spx):
    kind, m, n, seed = "dual", 65, 200, 1
    lp = _lp(kind, m, n, seed)
    A, b, c, l, u = lp
    with _ctx(spx, kind, lp) as ctx:
        r0 = ctx.solve()
        assert r0.status == spx.SolveStatus.OptimumFound
        g = ctx.rhs_ranging()
        s, up, fr, cost, rhs, _ = _device_ref(ctx, lp)
    cands = []
    for r in range(m):
        for sign, lim, key, ref, sec in ((-1.0, g.down[r], g.leave_down[r], rhs.down[r], rhs.second_down[r]),
                                         (1.0, g.up[r], g.leave_up[r], rhs.up[r], rhs.second_up[r])):
            if not np.isfinite(lim):
                continue
            beta = abs(s["binv"][int(key) // 2, r])
            if 0.001 * lim * beta > 10.0 * FEAS and float(sec) > 1.01 * float(ref):
                cands.append((r, sign, float(lim), int(key)))
    probes = _pick([p for p in cands if p[3] % 2 == 0], 5) + _pick([p for p in cands if p[3] % 2 == 1], 3)
    assert len(probes) >= 8 and {p[1] for p in probes} == {-1.0, 1.0}
    verified = 0
    for r, sign, lim, key in probes:
        with _ctx(spx, kind, lp) as ctx:
            q = ctx.solve()
            assert q.pivots == r0.pivots and np.array_equal(q.b_ixs, r0.b_ixs)
            flips = ctx.dual_flips()
            b1 = b.copy()
            b1[r] += sign * 0.999 * lim
            ctx.set_rhs(b1)
            q1 = ctx.solve()
            assert q1.status == spx.SolveStatus.OptimumFound
            assert q1.pivots == r0.pivots and ctx.dual_flips() == flips, (r, sign, lim)
            b2 = b.copy()
            b2[r] += sign * 1.001 * lim
            ctx.set_rhs(b2)
            st, piv = ctx.iterate(1)
            if st == spx.SolveStatus.Infeasible:  # past the limit the LP has no solution: a row was chosen, none entered
                assert piv == r0.pivots
                continue
            assert piv == r0.pivots + 1, (r, sign, lim, st)
            assert ctx.trace()[1][r0.pivots] == key // 2, (r, sign, key, ctx.trace()[1][r0.pivots])
            verified += 1
    print(f"rhs limits: {len(probes)} probes, {sum(1 for p in probes if p[3] % 2)} leaving to an upper bound, "
          f"{verified} with a first pivot to compare")
    assert verified >= 6


def test_refusals_leave_the_state_untouched(spx):
    kind, m, n, seed = "primal", 65, 200, 1
    lp = _lp(kind, m, n, seed)
    A, b, c, l, u = lp
    with _ctx(spx, kind, lp) as ref:
        want = ref.solve()
        sw = ref.state(binv=True)
    with _ctx(spx, kind, lp, timing=True) as ctx:
        def refused(word):
            for call in (ctx.cost_ranging, ctx.rhs_ranging):
                with pytest.raises(spx.SimplexError) as ei:
                    call()
                assert ei.value.code == -5 and word in str(ei.value), str(ei.value)
        refused("optimum")  # nothing solved yet
        ctx.iterate(5)
        refused("optimum")  # MAX_ITER
        r = ctx.solve()
        assert r.status == spx.SolveStatus.OptimumFound and r.pivots == want.pivots and r.z == want.z
        sg = ctx.state(binv=True)
        for key in ("x_b", "y", "binv", "b_ixs"):
            assert np.array_equal(sg[key], sw[key]), key
        g0 = ctx.cost_ranging()
        ctx.set_cost(c)  # the same cost: still changed since the optimum
        refused("optimum")
        assert ctx.solve().status == spx.SolveStatus.OptimumFound
        g1 = ctx.cost_ranging()  # (spx_set_cost reinverted B^-1: other bits, the same answer)
        assert np.array_equal(np.isinf(g0.down), np.isinf(g1.down)) and np.array_equal(np.isinf(g0.up), np.isinf(g1.up))
        ctx.set_rhs(b)
        refused("optimum")
        assert ctx.solve().status == spx.SolveStatus.OptimumFound
        ctx.set_bounds(u)
        refused("optimum")
        assert ctx.solve().status == spx.SolveStatus.OptimumFound
        ctx.cost_ranging()
        ctx.reset()
        refused("optimum")
        assert ctx.ranging_times()[1] == (3, 0)
        # NULL result arrays
        assert ctx._L.spx_ranging_cost(ctx._h, None, None, None, None) == -1
    # the windowed primal loop: refused by name, pointing at spx_set_algorithm, at its optimum too
    A0, b0, c0, _ = primal_box_ref.boxed_primal(m, n, seed)
    with spx.Context(np.ascontiguousarray(A0.T), b0, c0) as ctx:
        r = ctx.solve()
        assert r.status == spx.SolveStatus.OptimumFound
        for call in (ctx.cost_ranging, ctx.rhs_ranging):
            with pytest.raises(spx.SimplexError) as ei:
                call()
            assert ei.value.code == -5 and "SPX_ALGO_PRIMAL" in str(ei.value) and "spx_set_algorithm" in str(ei.value)
        r2 = ctx.solve()
        assert r2.pivots == r.pivots and r2.z == r.z
    # without timing the timing hook is refused
    with _ctx(spx, kind, lp) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.ranging_times()
        assert ei.value.code == -5


def test_index_pointers_may_be_null(spx):
    kind, m, n, seed = "dual", 7, 20, 0
    lp = _lp(kind, m, n, seed)
    with _ctx(spx, kind, lp) as ctx:
        assert ctx.solve().status == spx.SolveStatus.OptimumFound
        g, h = ctx.cost_ranging(), ctx.rhs_ranging()
        dn, up = np.zeros(n), np.zeros(n)
        assert ctx._L.spx_ranging_cost(ctx._h, dn.ctypes.data, up.ctypes.data, None, None) == 0
        assert np.array_equal(dn, g.down) and np.array_equal(up, g.up)
        dn, up = np.zeros(m), np.zeros(m)
        assert ctx._L.spx_ranging_rhs(ctx._h, dn.ctypes.data, up.ctypes.data, None, None) == 0
        assert np.array_equal(dn, h.down) and np.array_equal(up, h.up)


@pytest.mark.parametrize("kind", ["primal", "dual"])
def test_cli_ranging_files(spx, tmp_path, kind):
    """./solver --primal-box | --dual --bounds F --ranging PREFIX: the two files
    hold the Python arrays to %.17g."""
    m, n, seed = 65, 200, 1
    lp = _lp(kind, m, n, seed)
    A, b, c, l, u = lp
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
    prefix = str(tmp_path / "rng")
    solver = os.path.join(ROOT, "solver")
    flag = "--primal-box" if kind == "primal" else "--dual"
    r = subprocess.run([solver, flag, "--bounds", pb, "--ranging", prefix, "--no-iter-lines", p], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    with _ctx(spx, kind, lp, window=0) as ctx:
        assert ctx.solve().status == spx.SolveStatus.OptimumFound
        g, h = ctx.cost_ranging(), ctx.rhs_ranging()

    def lines(res):
        return ["%.17g %.17g %d %d" % (a, b_, k, q) for a, b_, k, q in zip(*res)]

    assert open(prefix + ".cost.txt").read().splitlines() == lines(g)
    assert open(prefix + ".rhs.txt").read().splitlines() == lines(h)
    # a solve that stops short of the optimum: the library's refusal, no files
    prefix2 = str(tmp_path / "short")
    r = subprocess.run([solver, flag, "--bounds", pb, "--ranging", prefix2, "--max-iter", "3", "--no-iter-lines", p],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--ranging failed" in r.stderr and "optimum" in r.stderr
    assert not os.path.exists(prefix2 + ".cost.txt")
