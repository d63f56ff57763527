"""Dense numpy restatement of the dual simplex loop with boxed variables
0 <= x_j <= u_j (include/simplex.h, SPX_ALGO_DUAL + spx_set_bounds): explicit
B^-1, Dantzig or exact-row-norm steepest-edge leaving rows, the textbook
bounded dual ratio test with a pivot tolerance (no bound flipping), first index
on every tie, no reinversion.  Conventions are the library's: maximise c.x,
A x = b with the slack identity in A's last m columns, e_j = y.A_j - c_j; u has
n entries (slacks included, +inf = none).

A non-basic column sits at 0 (sigma_j = +1) or at u_j (sigma_j = -1) and is
dual feasible with e_j >= -eps at lower, e_j <= +eps at upper;
x_b = B^-1 (b - sum_{j at upper} u_j A_j), z = c_B.x_b + sum_{j at upper} c_j u_j.

One pass:
  1. delta_i = x_b[i] if x_b[i] < -feas_tol, x_b[i] - u_k if x_b[i] > u_k +
     feas_tol (k the row's basic column), else 0.  Dantzig: q = argmin -|delta_i|,
     steepest edge: q = argmin -delta_i^2 / w_i, over delta_i != 0 (none:
     optimum).  s = +1 if delta_q < 0 (the row leaves to its lower bound), else -1.
  2. a_j = rho.A_j, d_j = y.A_j - c_j, ahat_j = s sigma_j a_j; candidates are the
     non-basic ahat_j < -piv_tol, key max(sigma_j d_j, 0) / -ahat_j (none:
     infeasible).
  3. alpha = B^-1 A_p, theta = delta_q / alpha_q, x_b -= theta alpha, x_b[q] =
     (u_p if p was at upper else 0) + theta, y -= (d_p / alpha_q) rho; the
     leaving column becomes non-basic at lower (s = +1) or at upper (s = -1).

`gap_row` / `gap_ratio` are the smallest relative gaps between the best and the
second-best key of the two argmins, as in tests/dual_se_ref.py.  `boxed` is the
generator the boxed tests share: its draws fix tests/golden/dual_box_optima.json.
"""
from dataclasses import dataclass, field

import numpy as np

import dual_ref
from dual_ref import INFEASIBLE, MAX_ITER, OPTIMUM, tied, whole
from dual_se_ref import _rel_gap, row_norms2

NOT_DUAL_FEASIBLE = "not_dual_feasible"
DANTZIG, STEEPEST = "dantzig", "steepest"


def boxed(m, n, seed, flipc=False):
    A, b, c = dual_ref.covering(m, n, seed)
    ns = n - m
    r = np.random.default_rng(seed + 1000)
    u = np.full(n, np.inf)
    us = r.uniform(0.25, 0.75, ns)
    us[::4] = np.inf
    u[:ns] = us
    sl = r.uniform(0.5, 1.5, m) * ns / 8
    sl[np.arange(m) % 3 != 0] = np.inf
    u[ns:] = sl
    if flipc:   # bounded structurals with c_j > 0: dual feasible only at their upper bound
        k = np.where(np.isfinite(u[:ns]))[0][::5]
        c = c.copy()
        c[k] = -0.5 * c[k]
    return A, b, c, u


def boxed_tall(m, n, seed, flipc=False):
    """boxed() for m far above n - m (tests/test_gpu_lds_cap.py: n = m + 64).
    There boxed()'s ranged rows contradict each other: 64 columns cannot keep
    every third row's G x within [h, h + u_slack] for thousands of independent
    h.  The structural draws are boxed()'s; the bounded slacks get 16 x its
    bounds, which leaves the LP feasible and the slacks flippable."""
    A, b, c, u = boxed(m, n, seed, flipc)
    u[n - m:] = u[n - m:] * 16.0
    return A, b, c, u


def tiny_box_infeasible():
    """x1 + x2 >= 2 with x1, x2 <= 0.5: the bounds make the covering row infeasible."""
    A = np.array([[1.0, 1.0, 1.0, 0.0], [-1.0, -1.0, 0.0, 1.0]])
    return A, np.array([4.0, -2.0]), np.array([-1.0, -1.0, 0.0, 0.0]), np.array([0.5, 0.5, np.inf, np.inf])


@dataclass
class DualBoxResult:
    status: str
    z: float
    pivots: int
    b_ixs: np.ndarray
    x_b: np.ndarray
    at_upper: np.ndarray            # n bools: non-basic at its upper bound
    trace: list = field(default_factory=list)
    gap_row: float = np.inf
    gap_ratio: float = np.inf
    to_upper: int = 0               # pivots whose row left to its upper bound
    placed: int = 0                 # columns the entry normalisation put at upper
    bad_column: int = -1            # NOT_DUAL_FEASIBLE: the column without an upper bound
    y: np.ndarray = None            # final duals and inverse
    Binv: np.ndarray = None
    ties: dict = field(default_factory=dict)  # passes whose argmin met an exact tie: "row", "ratio"
    integral: bool = True           # x_b, y and B^-1 held integers only after every pass

    def primal(self, u):
        x = np.where(self.at_upper, np.where(np.isfinite(u), u, 0.0), 0.0)
        x[self.b_ixs] = self.x_b
        return x


def dual_simplex_box(A, b, c, u, rule=DANTZIG, basis=None, at_upper=None, eps=1e-7, feas_tol=1e-9, piv_tol=1e-9,
                     max_iter=1 << 62, trace_cap=200):
    """From the slack basis with every column at lower, or from `basis` (m
    distinct columns, basis order) and the placements `at_upper`."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    m, n = A.shape
    ns = n - m
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
    c_B = c[b_ixs].copy()
    y = c_B @ Binv

    def x_basic():
        beff = b.copy()
        for j in np.flatnonzero(up):  # ascending j
            beff = beff - u[j] * A[:, j]
        return Binv @ beff

    # entry normalisation
    e = y @ A - c
    placed = 0
    for j in np.flatnonzero(~basic):
        if e[j] < -eps:
            if not np.isfinite(u[j]):
                return DualBoxResult(NOT_DUAL_FEASIBLE, np.nan, 0, b_ixs.copy(), x_basic(), up.copy(), bad_column=int(j))
            if not up[j]:
                up[j] = True
                placed += 1
        elif e[j] > eps and up[j]:
            up[j] = False
    x_b = x_basic()

    trace = []
    gap_row = gap_ratio = np.inf
    to_upper = 0
    ties = {"row": 0, "ratio": 0}
    integral = True
    it = 0
    status = MAX_ITER
    while it < max_iter:
        # 1. leaving row
        ub = u[b_ixs]
        delta = np.where(x_b < -feas_tol, x_b, np.where(x_b > ub + feas_tol, x_b - ub, 0.0))
        rows = delta != 0.0
        if not rows.any():
            status = OPTIMUM
            break
        if rule == STEEPEST:
            rkey = np.where(rows, -(delta * delta) / row_norms2(Binv), np.inf)
        else:
            rkey = np.where(rows, -np.abs(delta), np.inf)
        q = int(np.argmin(rkey))
        ties["row"] += int(tied(rkey))
        if rows.sum() > 1:
            two = np.partition(rkey, 1)[:2]
            gap_row = min(gap_row, _rel_gap(two[0], two[1]))
        s = 1.0 if delta[q] < 0.0 else -1.0
        # 2. pivot row and ratio test
        rho = Binv[q].copy()
        a = rho @ A
        d = y @ A - c
        sigma = np.where(up, -1.0, 1.0)
        ahat = s * sigma * a
        cand = (~basic) & (ahat < -piv_tol)
        if not cand.any():
            status = INFEASIBLE
            break
        key = np.where(cand, np.maximum(sigma * d, 0.0) / np.where(cand, -ahat, 1.0), np.inf)
        p = int(np.argmin(key))  # smallest column index on ties
        ties["ratio"] += int(tied(key))
        if cand.sum() > 1:
            two = np.partition(key, 1)[:2]
            gap_ratio = min(gap_ratio, _rel_gap(two[0], two[1]))
        # 3. FTRAN and update
        alpha = Binv @ A[:, p]
        aq = alpha[q]
        theta = delta[q] / aq
        x_b = x_b - theta * alpha
        x_b[q] = (u[p] if up[p] else 0.0) + theta
        y = y - (d[p] / aq) * rho
        c_B[q] = c[p]
        leave = b_ixs[q]
        basic[leave] = False
        up[leave] = s < 0.0
        to_upper += int(s < 0.0)
        basic[p] = True
        up[p] = False
        b_ixs[q] = p
        Binv = Binv - np.outer(alpha / aq, rho)
        Binv[q] = rho / aq
        integral = integral and whole(x_b, y, Binv)
        if it < trace_cap:
            trace.append((p, q))
        it += 1
    z = float(c_B @ x_b)
    zu = 0.0
    for j in np.flatnonzero(up):  # ascending j
        zu += c[j] * u[j]
    return DualBoxResult(status, z + zu, it, b_ixs.copy(), x_b.copy(), up.copy(), trace, float(gap_row),
                         float(gap_ratio), to_upper, placed, y=y.copy(), Binv=Binv.copy(), ties=ties,
                         integral=integral)


def farkas(A, b, u, b_ixs, at_upper, tol=1e-9):
    """Infeasibility from a basis alone.  For a basic row i with rho = row i of
    B^-1 every x with A x = b has x_k = rho.b - sum_{j non-basic} a_j x_j (a =
    rho.A), so over the box 0 <= x <= u it lies in [rho.b - sum_{a_j > 0} a_j u_j,
    rho.b - sum_{a_j < 0} a_j u_j] (an infinite u_j with a_j beyond `tol` opens
    that end; |a_j| <= tol counts as 0 with a finite u_j).  Returns (row,
    margin) of the row whose interval misses [0, u_k] by the most (the placements
    only pick the rows to try: those out of bounds now), or (-1, 0.0)."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[1]
    b_ixs = np.asarray(b_ixs, dtype=np.int64)
    up = np.array(at_upper, dtype=bool)
    basic = np.zeros(n, dtype=bool)
    basic[b_ixs] = True
    up &= ~basic
    B = A[:, b_ixs]
    x_b = np.linalg.solve(B, b - A[:, up] @ u[up])
    ub = u[b_ixs]
    best = (-1, 0.0)
    nb = ~basic
    fin = np.isfinite(u)
    uf = np.where(fin, u, 0.0)
    rows = np.flatnonzero((x_b < -tol) | (x_b > ub + tol))
    Binv = np.linalg.inv(B) if len(rows) else None
    for i in rows:
        rho = Binv[i]
        a = np.where(nb, rho @ A, 0.0)
        rb = float(rho @ b)
        hi = np.inf if (nb & ~fin & (a < -tol)).any() else rb - float(np.sum(np.where(fin & (a < 0.0), a * uf, 0.0)))
        lo = -np.inf if (nb & ~fin & (a > tol)).any() else rb - float(np.sum(np.where(fin & (a > 0.0), a * uf, 0.0)))
        margin = max(-hi, lo - ub[i])  # > 0: the interval lies below 0 or above u_k
        if margin > best[1]:
            best = (int(i), float(margin))
    return best


def certificate(A, b, c, u, b_ixs, at_upper):
    """From a basis and placements alone: (worst bound violation of x, worst
    sign violation of the reduced costs, z)."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[1]
    up = np.array(at_upper, dtype=bool)
    b_ixs = np.asarray(b_ixs, dtype=np.int64)
    basic = np.zeros(n, dtype=bool)
    basic[b_ixs] = True
    up &= ~basic
    B = A[:, b_ixs]
    beff = b - A[:, up] @ u[up]
    x_b = np.linalg.solve(B, beff)
    x = np.where(up, np.where(np.isfinite(u), u, 0.0), 0.0)
    x[b_ixs] = x_b
    viol = max(float(np.max(-x)), float(np.max(x - u)), 0.0)
    y = np.linalg.solve(B.T, c[b_ixs])
    e = y @ A - c
    nb = ~basic
    dviol = max(float(np.max(np.where(nb & ~up, -e, 0.0))), float(np.max(np.where(nb & up, e, 0.0))), 0.0)
    return viol, dviol, float(c @ x)
