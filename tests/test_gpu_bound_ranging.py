"""GPU: bound ranging and the objective at the range ends (spx_ranging_bound,
spx_ranging_objective, spx_ranging_bound_times; k_rng_bound_gather, k_rng_bound,
k_rng_bound_min, k_rng_bound_basic).

The kernels against the numpy restatement (tests/bound_ranging_ref.py), computed
in longdouble from the device's own optimum: the basis and the placements, and
B^-1 and x_b as spx_get_state returns them.  Values are compared within an
a-priori bound of tests/test_gpu_ranging.py's form, not a chosen tolerance.  With
eps = 2^-53, for the entry (i, k) that wins a column's minimum,

    e_T = 8 m eps sum_t |rho_it| |A_tk|        (the dot alpha_i in any summation order, fused or not)
    |ratio_device - ratio| <= 4 ratio e_T / |alpha_i|  +  4 e_x / |alpha_i|

(a quotient x / alpha or (u - x) / alpha with an error e_T in alpha moves by ratio
e_T / |alpha| to first order; x_b is the same vector bit for bit, the division,
the subtraction and the reference's own rounding are inside the factor 4; e_x =
4 eps (|x_b| + |l|) in a lower-shifted context, for the lower bound spx_get_state
added and this test subtracted again, 0 otherwise).  An own-bound winner is the
range u - l itself: exact.  A basic column's slacks are x_i and ub_B[i] - x_i:
e_x + 4 eps |value|.  Where the device's winner is another entry than the
restatement's (allowed only under the runner-up exemption) that entry's bound
is added.  The largest measured share of the bound is printed per case.

Indices are compared only where the restatement's runner-up (the own bound
counted among the candidates) is at least (1 + 1e-6) x the minimum; the case
builder (bound_ranging_ref.refuse_case) refuses an LP with an entry of T within
[tol / 2, 2 tol] or with more than 5 % of its non-basic columns under that
exemption, and runs here on the device's optimum again.

The objective at the range ends against a longdouble recomputation from the
device's vectors (x, y, d as read back; z recomputed as c.x): |end_device - end|
<= e_z + 4 eps (|z| + |delta mult|) with e_z = 8 n eps sum_j |c_j| (|x_j| + 2 |l_j|)
(the device sums c_B.x'_B of the shifted values and adds c.l again).

The semantics through the library's own re-solve (SPX_ALGO_DUAL takes a changed
bound from the old basis): a bound moved by 0.999 of a reported limit re-solves
with no pivot and no flip, and to the objective the range end predicts; by
1.001, the first pivot's row is the reported one, or, for the own bound,
spx_set_bounds_lu refuses l > u.  Probes have 0.001 Lambda |alpha*| > 10 feas_tol
and a runner-up beyond 1.01 Lambda, so the loop's tolerances cannot hide or fake
the change.
"""
import os
import subprocess

import numpy as np
import pytest

import bound_ranging_ref as br
import primal_box_ref
import ranging_ref as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS53 = 2.0 ** -53
TOL = 1e-9      # the contexts' piv_tol (the default)
FEAS = 1e-9     # and feasibility tolerance

_LPS = {}
_SOLVED = {}


def _lp(kind, m, n, seed):
    k = (kind, m, n, seed)
    if k not in _LPS:
        _LPS[k] = rr.build_lp(kind, m, n, seed)
    return _LPS[k]


def _ctx(spx, kind, lp, **kw):
    A, b, c, l, u = lp
    At = np.ascontiguousarray(A.T)
    kw.setdefault("trace", 4096)
    kw.setdefault("window", -1)
    if kind == "dual":
        return spx.Context(At, b, c, algorithm=spx.ALGO_DUAL, upper=u, **kw)
    if kind == "primal":
        return spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, **kw)
    return spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, lower=l, upper=u, primal_phase1=True, **kw)


def _bounds(lp):
    """(free, the lower bounds with 0 for a free column, the ranges)."""
    A, b, c, l, u = lp
    n = A.shape[1]
    fr = np.zeros(n, dtype=bool) if l is None else np.isneginf(l)
    lsh = np.zeros(n) if l is None else np.where(fr, 0.0, l)
    return fr, lsh, np.where(np.isfinite(u), u - lsh, np.inf)


def _device_ref(ctx, lp):
    """The restatement in longdouble from the device's optimum, and what the bounds need."""
    A = lp[0]
    s = ctx.state(binv=True)
    x, up = ctx.primal()
    fr, lsh, rng = _bounds(lp)
    bix = s["b_ixs"]
    xs = s["x_b"] - lsh[bix]
    ref = br.bound_ranging(A, bix, up, s["binv"], xs, rng, free=fr, tol=TOL, dtype=np.longdouble)
    e_x = 4.0 * EPS53 * (np.abs(s["x_b"]) + np.abs(lsh[bix])) * (lsh[bix] != 0.0)
    return s, x, up, fr, rng, ref, e_x


def _solved(spx, case):
    """One solve per case, shared by the tests that only read: the three rangings, their objective ends, the
    device's vectors and the restatement."""
    if case not in _SOLVED:
        kind = case[0]
        lp = _lp(*case)
        with _ctx(spx, kind, lp) as ctx:
            r = ctx.solve()
            assert r.status == spx.SolveStatus.OptimumFound
            gb, gr, gc = ctx.bound_ranging(), ctx.rhs_ranging(), ctx.cost_ranging()
            ends = {"bound": ctx.ranging_objective(gb), "rhs": ctx.ranging_objective(gr),
                    "cost": ctx.ranging_objective(gc)}
            s, x, up, fr, rng, ref, e_x = _device_ref(ctx, lp)
            assert s["pivots"] == r.pivots and s["status"] == spx.SolveStatus.OptimumFound
            d = ctx.reduced_costs()
            z = ctx.objective()
        _SOLVED[case] = dict(r=r, gb=gb, gr=gr, gc=gc, ends=ends, s=s, x=x, up=up, fr=fr, rng=rng, ref=ref, e_x=e_x,
                             d=d, z=z)
    return _SOLVED[case]


def _share(dev, ref, bound):
    return abs(dev - ref) / bound if bound > 0.0 else (0.0 if dev == ref else np.inf)


def _compare(A, s, ref, got, e_x):
    """(worst |device - restatement| / bound, indices compared, indices exempt, side-1 blockers, own-bound winners);
    asserts the infinities and the indices."""
    m, n = A.shape
    e_T = 8.0 * m * EPS53 * (np.abs(s["binv"]) @ np.abs(A)[:, ref.nb])
    pos_of = np.full(n, -1)
    pos_of[ref.nb] = np.arange(len(ref.nb))
    worst, compared, skipped, side1, own = 0.0, 0, 0, 0, 0

    def entry_bound(key, p, ratio):
        if key == br.OWN:
            return 0.0
        i = int(key) // 2
        return 4.0 * (ratio * e_T[i, p] + e_x[i]) / abs(float(ref.T[i, p]))

    for j in range(n):
        i, p = ref.row_of[j], pos_of[j]
        for rv, sec, kref, dev, kdev in ((ref.down[j], ref.second_down[j], ref.leave_down[j], got.down[j],
                                          got.leave_down[j]),
                                         (ref.up[j], ref.second_up[j], ref.leave_up[j], got.up[j], got.leave_up[j])):
            if not np.isfinite(rv):
                assert np.isinf(dev) and dev > 0 and kdev == -1 and kref == -1, (j, dev, kdev)
                continue
            rv = float(rv)
            assert np.isfinite(dev) and dev >= 0.0 and (kdev == br.OWN or 0 <= kdev < 2 * m), (j, rv, dev, kdev)
            if i >= 0:  # basic: its own slack
                assert kdev == kref, (j, i, kref, kdev)
                bound = e_x[i] + 4.0 * EPS53 * abs(rv)
            else:
                bound = entry_bound(kref, p, rv)
                if rr.exempt(rv, sec):
                    skipped += 1
                    if kdev != kref:
                        bound += entry_bound(kdev, p, rv)
                else:
                    compared += 1
                    assert kdev == kref, (j, rv, float(sec), kref, kdev)
                    side1 += int(kref >= 0 and kref % 2 == 1)
                    own += int(kref == br.OWN)
            worst = max(worst, _share(dev, rv, bound))
    return worst, compared, skipped, side1, own


@pytest.mark.parametrize("kind,m,n,seed", rr.CASES)
def test_kernels_against_restatement(spx, kind, m, n, seed):
    """7 x 20 (one tile), 65 x 200 (two row halves merged through LDS, two column
    tiles), 130 x 390 (two row blocks merged by k_rng_bound_min, m no multiple of
    16), 256 x 1024 (full 128-row blocks); after a bounded primal solve, a boxed
    dual solve, and general_lu with free and lower-shifted columns through phase 1."""
    lp = _lp(kind, m, n, seed)
    A = lp[0]
    q = _solved(spx, (kind, m, n, seed))
    ref, gb = q["ref"], q["gb"]
    assert br.refuse_case(ref, TOL) == []
    worst, compared, skipped, side1, own = _compare(A, q["s"], ref, gb, q["e_x"])
    nb = ref.nb
    print(f"{kind} {m}x{n}: {q['r'].pivots} pivots, {int(np.sum(ref.kind == 1))} non-basic columns at upper, "
          f"{int(np.sum(ref.kind == 2))} free; worst error / bound = {worst:.3g}, {compared} indices compared "
          f"({side1} side 1, {own} own bound), {skipped} exempt")
    assert compared > 0 and np.sum(ref.kind == 1) > 0 and side1 + own > 0
    assert skipped <= rr.SHARE * 2 * len(nb)  # the cap on the exemption: it cannot hide a failure
    assert worst <= 1.0, worst


@pytest.mark.parametrize("kind,m,n,seed", rr.CASES)
def test_nonbasic_slack_is_rhs_ranging_bit_for_bit(spx, kind, m, n, seed):
    """A non-basic slack of row r at lower: up == rhs.down[r] and down == rhs.up[r],
    values and indices, bit for bit (the unit column passes through the MFMA
    tiles exactly).  Where the slack's own upper bound caps "up" it is the
    range, strictly below the row's ratio."""
    q = _solved(spx, (kind, m, n, seed))
    gb, gr, ref, rng = q["gb"], q["gr"], q["ref"], q["rng"]
    seen = capped = 0
    for r in range(m):
        j = n - m + r
        if ref.kind[j] != 0:
            continue
        seen += 1
        assert gb.down[j] == gr.up[r] and gb.leave_down[j] == gr.leave_up[r], (r, gb.down[j], gr.up[r])
        if gb.leave_up[j] == br.OWN:
            capped += 1
            assert gb.up[j] == rng[j] and rng[j] < gr.down[r]
        else:
            assert gb.up[j] == gr.down[r] and gb.leave_up[j] == gr.leave_down[r], (r, gb.up[j], gr.down[r])
    print(f"{kind} {m}x{n}: {seen} non-basic slacks at lower, {capped} capped by their own bound")
    assert seen > capped


@pytest.mark.parametrize("kind,m,n,seed", rr.CASES)
def test_objective_ends_against_recomputation(spx, kind, m, n, seed):
    """All three kinds against longdouble arithmetic from the device's vectors."""
    A, b, c, l, u = _lp(kind, m, n, seed)
    q = _solved(spx, (kind, m, n, seed))
    ref, x, d, y = q["ref"], q["x"], q["d"], q["s"]["y"]
    ld = np.longdouble
    z = float(np.sum(c.astype(ld) * x.astype(ld)))
    lsh = _bounds((A, b, c, l, u))[1]
    e_z = 8.0 * n * EPS53 * float(np.sum(np.abs(c) * (np.abs(x) + 2.0 * np.abs(lsh))))
    assert abs(q["z"] - z) <= e_z
    moves = (ref.row_of < 0) & (ref.kind != 2)
    worst = 0.0
    for what, g, mult, mv in (("cost", q["gc"], x, None), ("rhs", q["gr"], y, None), ("bound", q["gb"], d, moves)):
        od, ou = br.objective_ends(what, z, g.down, g.up, mult, moves=mv, dtype=ld)
        got = q["ends"][what]
        zero = (mult == 0.0) if mv is None else ((mult == 0.0) | ~mv)
        for dev, rv, delta in ((got.down, od, g.down), (got.up, ou, g.up)):
            fin = np.isfinite(rv.astype(np.float64))
            assert np.array_equal(dev[~fin], rv[~fin].astype(np.float64)), what  # +-inf with its sign
            assert np.all(dev[zero] == q["z"]), what  # an exactly-zero multiplier: z, even where the delta is +inf
            term = np.abs(np.where(zero | ~fin, 0.0, delta) * mult)
            bound = e_z + 4.0 * EPS53 * (abs(z) + term)
            err = np.abs(dev[fin] - rv[fin].astype(np.float64))
            worst = max(worst, float(np.max(err / bound[fin])) if fin.any() else 0.0)
        if what != "rhs":
            assert np.any(zero & (np.isinf(g.down) | np.isinf(g.up))), what  # the exact-zero rule was exercised
    print(f"{kind} {m}x{n}: objective ends, worst error / bound = {worst:.3g}")
    assert worst <= 1.0, worst


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


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
            g1 = ctx.bound_ranging()
            g2 = ctx.bound_ranging()
            assert _same(g1, g2), kw
            got.append((g1, ctx.state()["b_ixs"]))
        if env:
            monkeypatch.delenv("SPX_PBOX_LDS_CAP")
    for g1, bix in got[1:]:
        assert np.array_equal(bix, got[0][1])
        assert _same(g1, got[0][0])
    assert _same(got[0][0], _solved(spx, (kind, m, n, seed))["gb"])  # and after cost / rhs ranging in the same context


def test_bit_for_bit_across_histories(spx):
    """After refactor_every=7 (another pivot history to the same basis), once
    each context's B^-1 is the reinversion of that basis: the same bits."""
    kind, m, n, seed = "primal", 130, 390, 2
    lp = _lp(kind, m, n, seed)
    with _ctx(spx, kind, lp) as a, _ctx(spx, kind, lp, refactor_every=7) as b:
        ra, rb = a.solve(), b.solve()
        assert ra.status == rb.status == spx.SolveStatus.OptimumFound
        assert np.array_equal(ra.b_ixs, rb.b_ixs) and np.array_equal(a.primal()[1], b.primal()[1])
        a.reinvert()
        b.reinvert()
        assert _same(a.bound_ranging(), b.bound_ranging())


def test_bound_ranging_leaves_the_loop_state_alone(spx):
    """Steepest edge, 130 x 390.  A context that asks (refused with a pivot and a
    recurrence pending after iterate(40); answered at the optimum, where the last
    pivot is still pending in B^-1) and one that never asks: the same trace, and
    after set_cost and 40 more pivots the same B^-1, x_b, y and weights, bit for
    bit."""
    kind, m, n, seed = "primal", 130, 390, 2
    lp = _lp(kind, m, n, seed)
    c2 = primal_box_ref.cost_variant(lp[2], n - m, seed)
    out = []
    for ask in (False, True):
        with _ctx(spx, kind, lp, primal_pricing=spx.PRIMAL_PRICING_STEEPEST, timing=True) as ctx:
            st, piv = ctx.iterate(40)
            assert piv == 40 and st == spx.SolveStatus.MaxIter
            if ask:
                with pytest.raises(spx.SimplexError) as ei:
                    ctx.bound_ranging()
                assert ei.value.code == -5 and "optimum" in str(ei.value)
            assert ctx.bound_ranging_times() == (0.0, 0)
            r = ctx.solve()
            assert r.status == spx.SolveStatus.OptimumFound
            if ask:
                g = ctx.bound_ranging()
                ctx.ranging_objective(g)
                t, k = ctx.bound_ranging_times()
                assert k == 1 and t > 0.0
                assert ctx.ranging_times() == ((0.0, 0.0), (0, 0))  # spx_ranging_times keeps its two slots
            assert ctx.bound_ranging_times() == (0.0, 0)
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
    cands = list(cands)
    if len(cands) <= count:
        return cands
    if count == 1:
        return [cands[len(cands) // 2]]
    return [cands[int(round(k * (len(cands) - 1) / (count - 1)))] for k in range(count)]


def test_bound_limits_through_the_dual_resolve(spx):
    kind, m, n, seed = "dual", 65, 200, 1
    lp = _lp(kind, m, n, seed)
    A, b, c, l, u = lp
    q = _solved(spx, (kind, m, n, seed))
    r0, g, ref, d, ends, rng = q["r"], q["gb"], q["ref"], q["d"], q["ends"]["bound"], q["rng"]
    pos_of = np.full(n, -1)
    pos_of[ref.nb] = np.arange(len(ref.nb))
    rows, owns = [], []
    for j in ref.nb:
        if ref.kind[j] == 2:
            continue
        for sign, lim, key, rv, sec, end in ((-1.0, g.down[j], g.leave_down[j], ref.down[j], ref.second_down[j],
                                              ends.down[j]),
                                             (1.0, g.up[j], g.leave_up[j], ref.up[j], ref.second_up[j], ends.up[j])):
            if not np.isfinite(lim) or not float(sec) > 1.01 * float(rv):
                continue
            if key == br.OWN:
                if lim > 1e-3:
                    owns.append((int(j), sign, float(lim), int(key), float(end)))
                continue
            alpha = abs(float(ref.T[int(key) // 2, pos_of[j]]))
            if 0.001 * lim * alpha > 10.0 * FEAS:
                rows.append((int(j), sign, float(lim), int(key), float(end)))
    lower = [p for p in rows if ref.kind[p[0]] == 0 and p[3] % 2 == 0]
    upper = [p for p in rows if ref.kind[p[0]] == 1 and p[3] % 2 == 0]
    side1 = [p for p in rows if p[3] % 2 == 1]
    probes = (_pick([p for p in lower if p[1] > 0], 2) + _pick([p for p in lower if p[1] < 0], 2) +
              _pick([p for p in upper if p[1] > 0], 1) + _pick([p for p in upper if p[1] < 0], 1) +
              _pick(side1, 2) + _pick(owns, 2))
    assert len(probes) >= 8 and {p[1] for p in probes} == {-1.0, 1.0}
    assert {int(ref.kind[p[0]]) for p in probes} == {0, 1}
    assert any(p[3] >= 0 and p[3] % 2 == 1 for p in probes) and any(p[3] == br.OWN for p in probes)
    # The bound on a re-solved objective against the predicted end.  Rounding: both objectives' own sums (e_z) and
    # the reduced cost's (e_d).  And the device's B^-1 = M is that of B only up to R = |M B - I|, measured here in
    # longdouble (a property of the loop's B^-1, not of ranging): x_b = M b is off by R |x_B|, so z by |c_B| R |x_B|
    # (e_B); y by |y - c_B M| + |c_B| R |M|, so d_j by that times |A_j| (e_y).
    x, y = q["x"], q["s"]["y"]
    e_z = 8.0 * n * EPS53 * (float(np.sum(np.abs(c) * np.abs(x))) + float(np.sum(np.abs(y) * np.abs(b))))
    ld = np.longdouble
    bix, M = q["s"]["b_ixs"], q["s"]["binv"].astype(ld)
    R = np.abs(M @ A[:, bix].astype(ld) - np.eye(m, dtype=ld))
    cB = np.abs(c[bix]).astype(ld)
    e_B = float(cB @ R @ np.abs(q["s"]["x_b"]).astype(ld))
    y_off = np.abs(y.astype(ld) - c[bix].astype(ld) @ M) + cB @ R @ np.abs(M)
    verified, worst = 0, 0.0
    for j, sign, lim, key, end in probes:
        def moved(f):
            l2, u2 = np.zeros(n), u.copy()
            if ref.kind[j] == 0:
                l2[j] = sign * f * lim
            else:
                u2[j] = u[j] + sign * f * lim
            return l2, u2
        with _ctx(spx, kind, lp) as ctx:
            r = ctx.solve()
            assert r.pivots == r0.pivots and np.array_equal(r.b_ixs, r0.b_ixs)
            flips = ctx.dual_flips()
            ctx.set_bounds_lu(*moved(0.999))
            r1 = ctx.solve()
            assert r1.status == spx.SolveStatus.OptimumFound
            assert r1.pivots == r0.pivots and ctx.dual_flips() == flips, (j, sign, lim, key)
            # the objective on the way to the range end: z + 0.999 (end - z)
            want = q["z"] + 0.999 * (end - q["z"])
            e_d = 8.0 * m * EPS53 * (float(np.abs(y) @ np.abs(A[:, j])) + abs(c[j]))
            e_y = float(y_off @ np.abs(A[:, j]).astype(ld))
            bound = 4.0 * (2.0 * e_z + 2.0 * e_B + lim * (e_d + e_y))
            worst = max(worst, _share(r1.z, want, bound))
            if key == br.OWN:  # past the limit the bounds cross: refused, nothing changed
                with pytest.raises(spx.SimplexError) as ei:
                    ctx.set_bounds_lu(*moved(1.001))
                assert ei.value.code == -1 and "above its upper bound" in str(ei.value)
                continue
            ctx.set_bounds_lu(*moved(1.001))
            st, piv = ctx.iterate(1)
            if st == spx.SolveStatus.Infeasible:  # past the limit the LP has no solution: a row was chosen, none entered
                assert piv == r0.pivots
                continue
            assert piv == r0.pivots + 1, (j, sign, lim, st)
            assert ctx.trace()[1][r0.pivots] == key // 2, (j, sign, key, ctx.trace()[1][r0.pivots])
            verified += 1
    print(f"bound limits: {len(probes)} probes ({len(side1)} side-1 and {len(owns)} own-bound candidates), "
          f"{verified} with a first pivot to compare; re-solved objective at 0.999: worst error / bound = {worst:.3g}")
    assert verified >= 4
    assert worst <= 1.0, worst


def test_refusals_and_null_pointers(spx):
    kind, m, n, seed = "primal", 65, 200, 1
    lp = _lp(kind, m, n, seed)
    A, b, c, l, u = lp
    with _ctx(spx, kind, lp, timing=True) as ctx:
        def refused(word):
            with pytest.raises(spx.SimplexError) as ei:
                ctx.bound_ranging()
            assert ei.value.code == -5 and word in str(ei.value), str(ei.value)
            dn, up = np.zeros(n), np.zeros(n)
            for what in (0, 1, 2):
                assert ctx._L.spx_ranging_objective(ctx._h, what, dn.ctypes.data, up.ctypes.data, dn.ctypes.data,
                                                    up.ctypes.data) == -5
        refused("optimum")  # nothing solved yet
        ctx.iterate(5)
        refused("optimum")  # MAX_ITER
        assert ctx.solve().status == spx.SolveStatus.OptimumFound
        g = ctx.bound_ranging()
        for setter, arg in ((ctx.set_cost, c), (ctx.set_rhs, b), (ctx.set_bounds, u)):
            setter(arg)
            refused("optimum")
            assert ctx.solve().status == spx.SolveStatus.OptimumFound
        g1 = ctx.bound_ranging()
        assert np.array_equal(g.leave_down, g1.leave_down) and np.array_equal(g.leave_up, g1.leave_up)
        ctx.reset()
        refused("optimum")
        assert ctx.bound_ranging_times()[1] == 2
        assert ctx.solve().status == spx.SolveStatus.OptimumFound
        # NULL result arrays are refused, NULL index arrays are not; an unknown kind of ranging is an argument error
        assert ctx._L.spx_ranging_bound(ctx._h, None, None, None, None) == -1
        dn, up = np.zeros(n), np.zeros(n)
        assert ctx._L.spx_ranging_bound(ctx._h, dn.ctypes.data, up.ctypes.data, None, None) == 0
        g2 = ctx.bound_ranging()
        assert np.array_equal(dn, g2.down) and np.array_equal(up, g2.up)
        assert ctx._L.spx_ranging_objective(ctx._h, 3, dn.ctypes.data, up.ctypes.data, dn.ctypes.data,
                                            up.ctypes.data) == -1
        with pytest.raises(TypeError):
            ctx.ranging_objective((dn, up))
    # the windowed primal loop: refused by name, pointing at spx_set_algorithm, at its optimum too
    A0, b0, c0, _ = primal_box_ref.boxed_primal(m, n, seed)
    with spx.Context(np.ascontiguousarray(A0.T), b0, c0) as ctx:
        r = ctx.solve()
        assert r.status == spx.SolveStatus.OptimumFound
        with pytest.raises(spx.SimplexError) as ei:
            ctx.bound_ranging()
        assert ei.value.code == -5 and "SPX_ALGO_PRIMAL" in str(ei.value) and "spx_set_algorithm" in str(ei.value)
        r2 = ctx.solve()
        assert r2.pivots == r.pivots and r2.z == r.z
    # without timing the timing hook is refused
    with _ctx(spx, kind, lp) as ctx:
        with pytest.raises(spx.SimplexError) as ei:
            ctx.bound_ranging_times()
        assert ei.value.code == -5


def test_tiny_hand_made(spx):
    """The exact tie of two rows (the smaller 2 row + side), the own bound tying a
    row (the row), the own bound winning, a fixed column, and tiny_free's free
    non-basic column."""
    A, b, c, u, basis = br.tie_rows()
    At = np.ascontiguousarray(A.T)
    for u2, want_up, want_key in ((np.inf, 4.0, "row"), (4.0, 4.0, "row"), (3.0, 3.0, br.OWN), (0.0, 0.0, br.OWN)):
        uu = u.copy()
        uu[2] = u2
        with spx.Context(At, b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=uu, window=-1) as ctx:
            r = ctx.solve()
            assert r.status == spx.SolveStatus.OptimumFound and sorted(r.b_ixs.tolist()) == basis
            g = ctx.bound_ranging()
            rows = {int(j): i for i, j in enumerate(r.b_ixs)}
            key = 2 * min(rows.values()) if want_key == "row" else want_key  # both rows tie: the smaller row
            assert g.up[2] == want_up and g.leave_up[2] == key, (u2, g.up[2], g.leave_up[2])
            assert np.isinf(g.down[2]) and g.leave_down[2] == -1
            assert g.up[0] == 4.0 and g.leave_up[0] == 2 * rows[0] and np.isinf(g.down[0]) and g.leave_down[0] == -1
    # rows 1 and 4 tie: other lanes of the accumulator layout than rows 0 and 1
    A, b, c, u, basis = br.tie_rows_far()
    with spx.Context(np.ascontiguousarray(A.T), b, c, algorithm=spx.ALGO_PRIMAL_BOX, upper=u, window=-1) as ctx:
        r = ctx.solve()
        assert r.status == spx.SolveStatus.OptimumFound and r.b_ixs.tolist() == basis
        g = ctx.bound_ranging()
        assert g.up[6] == 4.0 and g.leave_up[6] == 2, (g.up[6], g.leave_up[6])
    A, b, c, l, u, basis = rr.tiny_free()
    with spx.Context(np.ascontiguousarray(A.T), b, c, algorithm=spx.ALGO_PRIMAL_BOX, lower=l, upper=u, window=-1) as ctx:
        r = ctx.solve()
        assert r.status == spx.SolveStatus.OptimumFound and sorted(r.b_ixs.tolist()) == sorted(basis)
        g = ctx.bound_ranging()
        e = ctx.ranging_objective(g)
        z = ctx.objective()
    assert np.isinf(g.down[3]) and np.isinf(g.up[3]) and g.leave_down[3] == -1 and g.leave_up[3] == -1
    rows = {int(j): i for i, j in enumerate(r.b_ixs)}
    assert g.up[1] == 4.0 and g.leave_up[1] == 2 * rows[0]
    assert e.down[3] == z and e.up[3] == z and e.up[1] == z - 4.0 * 2.0  # d_1 = 2


@pytest.mark.parametrize("kind", ["primal", "dual"])
def test_cli_bound_ranging_file(spx, tmp_path, kind):
    """./solver --primal-box | --dual --bounds F --bound-ranging PREFIX: the file
    holds the Python arrays to %.17g; --ranging beside it writes what it writes alone."""
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
    r = subprocess.run([solver, flag, "--bounds", pb, "--bound-ranging", prefix, "--ranging", prefix, "--no-iter-lines", p],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    with _ctx(spx, kind, lp, window=0) as ctx:
        assert ctx.solve().status == spx.SolveStatus.OptimumFound
        gc, gr = ctx.cost_ranging(), ctx.rhs_ranging()
        g = ctx.bound_ranging()
        e = ctx.ranging_objective(g)
    want = ["%.17g %.17g %d %d %.17g %.17g" % t for t in zip(g.down, g.up, g.leave_down, g.leave_up, e.down, e.up)]
    assert open(prefix + ".bound.txt").read().splitlines() == want
    for res, name in ((gc, ".cost.txt"), (gr, ".rhs.txt")):
        assert open(prefix + name).read().splitlines() == ["%.17g %.17g %d %d" % t for t in zip(*res)]
    # a solve that stops short of the optimum: the library's refusal, no file
    prefix2 = str(tmp_path / "short")
    r = subprocess.run([solver, flag, "--bounds", pb, "--bound-ranging", prefix2, "--max-iter", "3", "--no-iter-lines", p],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--bound-ranging failed" in r.stderr and "optimum" in r.stderr
    assert not os.path.exists(prefix2 + ".bound.txt")
