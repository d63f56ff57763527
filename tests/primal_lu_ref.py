"""Dense numpy restatement of the bounded primal simplex loop with general bounds
l <= x <= u (include/simplex.h, spx_set_bounds_lu under SPX_ALGO_PRIMAL_BOX with
SPX_FLAG_PRIMAL_PHASE1).  It extends
tests/primal_phase1_ref.py primal_simplex_phase1 (same conventions: maximise
c.x, A x = b with the slack identity in A's last m columns, explicit B^-1, first
index on every tie, no reinversion) with two things.

The shift.  lsh_j = l_j where finite, 0 for a free column; the loop runs on x' =
x - lsh with ranges r_j = u_j - lsh_j (+inf stays) and right-hand side b - A.lsh
(the columns with lsh_j != 0 in ascending j), and knows nothing else of l.  The
results come back in the caller's variables: x_b plus the basic column's lsh, a
non-basic column exactly l_j or u_j, z plus sum_j c_j lsh_j (ascending j).

The free rule (l_j = -inf and u_j = +inf).
  - A non-basic free column sits at 0 and is never at upper.  It is a candidate
    when |d_j| > eps, with sigma_j = +1 if d_j < 0, else -1; its key is -|d_j|
    under the same argmin (first column on ties) as every other candidate.
  - An entering free column never flips (its range is infinite); with no
    blocking row it is UNBOUNDED in phase 2, BREAKDOWN in phase 1; a pivot puts
    x_b[q] = sigma_p theta.
  - A row whose basic column is free never blocks, is never below or above
    (w_i = 0, not counted in ninf) and so never leaves: a leaving column is
    never free, and the placements after a pivot are primal_simplex_phase1's.
  - Optimum: the bounded non-basic columns satisfy primal_simplex_phase1's sign
    conditions and every free non-basic column has |d_j| <= eps.

With l = 0 and no free column every line below computes what
primal_simplex_phase1 computes, in the same order.  `general_lu` is the
generator the tests share: its draws fix tests/golden/primal_lu_optima.json.
"""
from dataclasses import dataclass

import numpy as np

from dual_ref import MAX_ITER, OPTIMUM, tied, whole
from dual_se_ref import _rel_gap
from primal_box_ref import UNBOUNDED, all_bounded
from primal_phase1_ref import BREAKDOWN, INFEASIBLE, Phase1Result, boxed_general, contradict  # noqa: F401


def general_lu(m, n, seed, free=True):
    """boxed_general(m, n, seed) with general bounds, returned as (A, b, c, l, u).
    Structural column j: j % 5 == 2 is free with a cost of either sign (only
    with `free`); else j % 11 == 7 is fixed at a value of either sign; else j % 3
    == 0 gets a finite lower bound of either sign and keeps its range.  Slack i
    with i % 7 == 3 gets the lower bound -0.05 (its row's right-hand side is
    relaxed by that much).  b moves by A.l, so the shifted LP has
    boxed_general's right-hand side: the >= rows and the ranged rows whose slack
    starts out of its bounds stay.  With `free` every slack without a bound gets
    a wide one (|b_i| + (n - m) / 4): all rows are then ranged, which keeps the
    LP bounded with a fifth of its columns free."""
    A, b, c, u = boxed_general(m, n, seed)
    r = np.random.default_rng(seed + 9000)
    ns = n - m
    j = np.arange(ns)
    lo = r.uniform(-0.5, 0.5, ns)
    fx = r.uniform(-0.2, 0.3, ns)
    cf = r.uniform(-1.0, 1.0, ns)
    is_free = (j % 5 == 2) & free
    is_fixed = ~is_free & (j % 11 == 7)
    is_low = ~is_free & ~is_fixed & (j % 3 == 0)
    l = np.zeros(n)
    u = u.copy()
    c = c.copy()
    l[:ns][is_low] = lo[is_low]
    u[:ns][is_low] = u[:ns][is_low] + lo[is_low]  # (+inf stays)
    l[:ns][is_fixed] = fx[is_fixed]
    u[:ns][is_fixed] = fx[is_fixed]
    l[:ns][is_free] = -np.inf
    u[:ns][is_free] = np.inf
    c[:ns][is_free] = cf[is_free]
    i = np.arange(m)
    l[ns:][i % 7 == 3] = -0.05
    if free:  # every row two-sided, far enough out to cut nothing else off
        wide = ~np.isfinite(u[ns:])
        u[ns:][wide] = np.abs(b[wide]) + 0.25 * ns
    lsh = np.where(np.isfinite(l), l, 0.0)
    b = b + A @ lsh
    return A, b, c, l, u


def shift_lp(m, n, seed):
    """general_lu without free columns and with every range finite
    (primal_box_ref.all_bounded on u - l): every non-basic column has a dual
    feasible side, so the dual loop takes the slack basis too."""
    A, b, c, l, u = general_lu(m, n, seed, free=False)
    return A, b, c, l, l + all_bounded(u - l, n - m)


def moved_lower(l, u, seed):
    """The re-solve's second lower bounds: every finite non-zero l_j that is not
    a fixed column's moves by up to 0.1 either way, never above u_j."""
    r = np.random.default_rng(seed + 9500)
    d = r.uniform(-0.1, 0.1, len(l))
    mv = np.isfinite(l) & (l != 0.0) & (l != u)
    l2 = l.copy()
    l2[mv] = np.minimum(l[mv] + d[mv], u[mv])
    return l2


def lower_twin(A, b, u, seed):
    """(l, b2, u2): the LP (A, b, c, 0 <= x <= u) of a neighbouring golden file
    moved to lower bounds l: l_j ~ U[-0.5, 0.5] on about 40 % of all n columns,
    slacks included, 0 elsewhere; b2 = b + A.l; u2 = u + l (+inf stays).  No
    column becomes fixed or free.  The shifted problem of (A, b2, c, l, u2) is
    the neighbour's own LP up to rounding of order 1e-14, so, its golden argmins
    being separated by 1e-6, the twin walks the neighbour's golden passes."""
    n = A.shape[1]
    r = np.random.default_rng(seed + 9700)
    pick = r.uniform(0, 1, n) < 0.4
    l = np.where(pick, r.uniform(-0.5, 0.5, n), 0.0)
    return l, b + A @ l, np.where(np.isfinite(u), u + l, np.inf)


def shifted(A, b, l, u):
    """(b_eff, range) as the device forms them from finite lower bounds: b_eff =
    b - sum_j l_j A_j over l_j != 0 in ascending j, one product and one
    subtraction per entry (no fma); range_j = fl(u_j - l_j), +inf stays."""
    beff = np.array(b, dtype=np.float64)
    for j in np.flatnonzero(l != 0.0):
        beff = beff - l[j] * A[:, j]
    return beff, np.where(np.isfinite(u), u - l, np.inf)


def tiny_unbounded_free():
    """max -x0, x0 free, one row x0 + s = 1: x0 falls without a bound (the slack
    rises, nothing blocks)."""
    A = np.array([[1.0, 1.0]])
    return A, np.array([1.0]), np.array([-1.0, 0.0]), np.array([-np.inf, 0.0]), np.array([np.inf, np.inf])


@dataclass
class LuResult(Phase1Result):
    """Phase1Result in the caller's variables: x_b includes the basic columns'
    lower bounds and z the sum c.l; `x_shifted` is the loop's own x_b."""
    x_shifted: np.ndarray = None
    free_entered: int = 0   # pivots whose entering column is free
    free_basic: int = 0     # free columns in the final basis
    fixed_flips: int = 0    # passes in which a fixed column (u_j = l_j) enters and flips at once
    ray_col: int = -1       # UNBOUNDED: the entering column that no row blocks
    # `ties` has one key more than Phase1Result's: "free_price", the passes whose pricing tie has a free column among
    # the tied minima

    def primal_lu(self, l, u):
        x = np.where(self.at_upper, u, np.where(np.isfinite(l), l, 0.0))
        x[self.b_ixs] = self.x_b
        return x


def _classify(x_b, lo, ub, feas_tol):
    return np.where(x_b < lo - feas_tol, 1.0, np.where(x_b > ub + feas_tol, -1.0, 0.0))


def primal_simplex_lu(A, b, c, l, u, basis=None, at_upper=None, eps=1e-7, feas_tol=1e-9, piv_tol=1e-9,
                      max_iter=1 << 62, trace_cap=200):
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    l = np.asarray(l, dtype=np.float64)
    uu = np.asarray(u, dtype=np.float64)
    m, n = A.shape
    ns = n - m
    free = np.isneginf(l)
    assert not np.any(free & np.isfinite(uu)) and not np.any(l > uu) and not np.any(np.isposinf(l))
    # the shift: the loop below sees 0 <= x' <= u (free columns: -inf < x' < +inf)
    lsh = np.where(free, 0.0, l)
    u = np.where(np.isfinite(uu), uu - lsh, np.inf)
    lo0 = np.where(free, -np.inf, 0.0)  # the shifted lower bounds
    if basis is None:
        b_ixs = np.arange(ns, n)
        Binv = np.eye(m)
    else:
        b_ixs = np.array(basis, dtype=np.int64)
        Binv = np.linalg.inv(A[:, b_ixs])
    up = np.zeros(n, dtype=bool) if at_upper is None else np.array(at_upper, dtype=bool)
    basic = np.zeros(n, dtype=bool)
    basic[b_ixs] = True
    up &= ~basic
    up &= np.isfinite(u)
    c_B = c[b_ixs].copy()
    y = c_B @ Binv
    y_stale = False
    beff = b.copy()
    for j in range(n):  # ascending j: the lower term, then the at-upper term
        if lsh[j] != 0.0:
            beff = beff - lsh[j] * A[:, j]
        if up[j]:
            beff = beff - u[j] * A[:, j]
    x_b = Binv @ beff

    trace = []
    gap_price = gap_ratio = gap_flip = np.inf
    flips = to_upper = p1_passes = p1_pivots = 0
    ties = {"price": 0, "ratio": 0, "flip": 0, "p1_price": 0, "p1_ratio": 0, "p1_flip": 0, "free_price": 0}
    free_entered = fixed_flips = 0
    ray_col = -1
    integral = True
    hist = []
    it = 0
    w = _classify(x_b, lo0[b_ixs], u[b_ixs], feas_tol)
    ninf = ninf0 = int(np.count_nonzero(w))

    def result(status):
        z = float(c_B @ x_b)
        zu = 0.0
        for j in np.flatnonzero(up):  # ascending j
            zu += c[j] * u[j]
        zl = 0.0
        for j in range(n):  # ascending j
            zl += c[j] * lsh[j]
        return LuResult(status, z + (zu + zl), it, b_ixs.copy(), x_b + lsh[b_ixs], up.copy(),
                        trace, float(gap_price), float(gap_ratio), float(gap_flip), flips, to_upper, p1_passes,
                        p1_pivots, ninf0, ninf, hist, c_B @ Binv if y_stale else y.copy(), Binv.copy(), ties, integral,
                        x_b.copy(), free_entered, int(np.count_nonzero(free[b_ixs])), fixed_flips, ray_col)

    def tie(name, hit, ph1):
        ties[name] += int(hit)
        if ph1:
            ties["p1_" + name] += int(hit)

    status = MAX_ITER
    while it < max_iter:
        ph1 = ninf > 0
        hist.append(ninf)
        # 1. pricing
        if ph1:
            d = (w @ Binv) @ A
        else:
            if y_stale:
                y = c_B @ Binv
                y_stale = False
            d = y @ A - c
        sigma = np.where(free, np.where(d < 0.0, 1.0, -1.0), np.where(up, -1.0, 1.0))
        key = np.where(~basic, np.where(free, -np.abs(d), sigma * d), np.inf)
        cand = key < -eps
        if not cand.any():
            status = INFEASIBLE if ph1 else OPTIMUM
            break
        key = np.where(cand, key, np.inf)
        p = int(np.argmin(key))
        tie("price", tied(key), ph1)
        ties["free_price"] += int(tied(key) and bool(np.any(free & (key == key[p]))))
        if cand.sum() > 1:
            two = np.partition(key, 1)[:2]
            gap_price = min(gap_price, _rel_gap(two[0], two[1]))
        sp = sigma[p]
        # 2. FTRAN
        alpha = Binv @ A[:, p]
        ahat = sp * alpha
        # 3. ratio test
        ub = u[b_ixs]
        lob = lo0[b_ixs]
        feas = w == 0.0 if ph1 else np.ones(m, dtype=bool)
        lo = feas & (ahat > piv_tol) & np.isfinite(lob)  # a free basic column has no lower bound to leave to
        hi = feas & (ahat < -piv_tol) & np.isfinite(ub)
        t = np.full(m, np.inf)
        t[lo] = np.maximum(x_b[lo], 0.0) / ahat[lo]
        t[hi] = np.maximum(ub[hi] - x_b[hi], 0.0) / (-ahat[hi])
        if ph1:
            bl = (w > 0.0) & (ahat < -piv_tol)  # rises to 0: leaves to its lower bound
            ab = (w < 0.0) & (ahat > piv_tol)   # falls to u_k: leaves to its upper bound
            t[bl] = x_b[bl] / ahat[bl]
            t[ab] = (x_b[ab] - ub[ab]) / ahat[ab]
            lo = lo | bl
            hi = hi | ab
        rows = lo | hi
        q = int(np.argmin(t)) if rows.any() else -1
        if rows.sum() > 1:
            two = np.partition(t, 1)[:2]
            gap_ratio = min(gap_ratio, _rel_gap(two[0], two[1]))
        u_p = u[p]
        if np.isfinite(u_p) and q >= 0:
            if u_p > 0.0:  # (a fixed column, u_p = 0 <= t_q whatever t_q is: the flip does not hang on rounding)
                gap_flip = min(gap_flip, _rel_gap(u_p, t[q]))
            tie("flip", u_p == t[q], ph1)
        if q >= 0:
            tie("ratio", tied(t), ph1)
        p1_passes += int(ph1)
        # 4. flip
        if np.isfinite(u_p) and (q < 0 or u_p <= t[q]):
            x_b = x_b - u_p * ahat
            up[p] = not up[p]
            flips += 1
            fixed_flips += int(u_p == 0.0)
            integral = integral and whole(x_b)
            if ph1:
                w = _classify(x_b, lo0[b_ixs], u[b_ixs], feas_tol)
                ninf = int(np.count_nonzero(w))
            continue
        # 5. no row
        if q < 0:
            p1_passes -= int(ph1)  # (the pass committed nothing)
            status = BREAKDOWN if ph1 else UNBOUNDED
            ray_col = p
            break
        # 6. pivot
        theta = t[q]
        rho = Binv[q].copy()
        aq = alpha[q]
        x_b = x_b - theta * ahat
        x_b[q] = (u_p if up[p] else 0.0) + sp * theta
        if ph1:
            y_stale = True
            p1_pivots += 1
        else:
            y = y - (d[p] / aq) * rho
        c_B[q] = c[p]
        leave = b_ixs[q]
        assert not free[leave]
        basic[leave] = False
        up[leave] = bool(hi[q])
        to_upper += int(hi[q])
        basic[p] = True
        up[p] = False
        free_entered += int(free[p])
        b_ixs[q] = p
        Binv = Binv - np.outer(alpha / aq, rho)
        Binv[q] = rho / aq
        integral = integral and whole(x_b, y, Binv)
        if it < trace_cap:
            trace.append((p, q))
        it += 1
        if ph1:
            w = _classify(x_b, lo0[b_ixs], u[b_ixs], feas_tol)
            ninf = int(np.count_nonzero(w))
    return result(status)


def certificate_lu(A, b, c, l, u, b_ixs, at_upper):
    """(bound violation, reduced-cost sign violation, z) of a basis with
    placements on the unshifted problem, from scratch with a dense solve: x_N at
    l_j or u_j (a free column at 0), x_B = B^-1 (b - N x_N); the largest amount
    by which some x_j leaves [l_j, u_j]; d = c_B B^-1 A - c over the non-basic
    columns must be >= 0 at lower, <= 0 at upper and 0 for a free column (a
    fixed column's sign is free); z = c.x."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    b_ixs = np.asarray(b_ixs, dtype=np.int64)
    up = np.asarray(at_upper, dtype=bool)
    basic = np.zeros(n, dtype=bool)
    basic[b_ixs] = True
    free = np.isneginf(l)
    x = np.where(up, u, np.where(free, 0.0, l))
    x[basic] = 0.0
    B = A[:, b_ixs]
    x[b_ixs] = np.linalg.solve(B, b - A @ x)
    viol = float(max(np.max(l - x), np.max(x - u), 0.0))
    y = np.linalg.solve(B.T, c[b_ixs])
    d = y @ A - c
    nb = ~basic
    fixed = l == u
    bad = np.where(free, np.abs(d), np.where(up, d, -d))
    bad = np.where(nb & ~fixed, bad, 0.0)
    return viol, float(max(np.max(bad), 0.0)), float(c @ x)
