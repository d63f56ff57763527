"""Dense numpy restatement of the bounded primal simplex loop, 0 <= x_j <= u_j
(include/simplex.h, SPX_ALGO_PRIMAL_BOX): explicit B^-1, Dantzig entering
column, the two-sided ratio test with a pivot tolerance, bound flips, first
index on every tie, no reinversion.  Conventions are the library's: maximise
c.x, A x = b with the slack identity in A's last m columns, e_j = y.A_j - c_j;
u has n entries (slacks included, +inf = none).

A non-basic column sits at 0 (sigma_j = +1) or at u_j (sigma_j = -1);
x_b = B^-1 (b - sum_{j at upper} u_j A_j), z = c_B.x_b + sum_{j at upper} c_j u_j.
The basis must be primal feasible on entry (-feas_tol <= x_b[i] <= u_k +
feas_tol, k the row's basic column): there is no phase 1 and no normalisation.

One pass:
  1. d_j = y.A_j - c_j, candidates are the non-basic sigma_j d_j < -eps,
     p = argmin sigma_j d_j (none: optimum).
  2. alpha = B^-1 A_p, ahat = sigma_p alpha.
  3. Row i with ahat_i > piv_tol leaves to its lower bound, t_i = max(x_b[i], 0)
     / ahat_i; row i with ahat_i < -piv_tol and a finite bound u_k leaves to its
     upper bound, t_i = max(u_k - x_b[i], 0) / -ahat_i; q = argmin t_i.
  4. u_p finite and (no row, or u_p <= t_q): a flip.  x_b -= u_p ahat, p changes
     sides, no pivot.
  5. No row and u_p = +inf: unbounded.
  6. Else theta = t_q: x_b -= theta ahat, x_b[q] = (u_p if p was at upper else
     0) + sigma_p theta, y -= (d_p / alpha_q) rho with rho row q of B^-1 before
     the pivot; the leaving column becomes non-basic at the bound it left to.

`pivots` counts pivots only (a flip pass is not one); `trace` holds the pivots'
(p, q).  `gap_price` / `gap_ratio` are the smallest relative gaps between the
best and the second-best key of the two argmins, `gap_flip` the smallest
relative distance between u_p and t_q where both are finite: above the golden
generator's threshold the pass sequence does not depend on the fp64 summation
order.  `boxed_primal` is the generator the tests share: its draws fix
tests/golden/primal_box_optima.json.
"""
from dataclasses import dataclass, field

import numpy as np

from dual_box_ref import certificate  # noqa: F401  (the tests take it from here)
from dual_ref import MAX_ITER, OPTIMUM, tied, whole
from dual_se_ref import _rel_gap

UNBOUNDED = "unbounded"
NOT_PRIMAL_FEASIBLE = "not_primal_feasible"


def boxed_primal(m, n, seed):
    """max c.x, A x <= b (b > 0), 0 <= x <= u: A has negative entries, so ranged
    rows (bounded slacks) and rows leaving to their upper bound bind."""
    r = np.random.default_rng(seed + 2000)
    ns = n - m
    A = np.zeros((m, n))
    A[:, :ns] = r.uniform(-0.5, 1.0, (m, ns))
    A[:, ns:] = np.eye(m)
    b = r.uniform(0.5, 1.5, m) * ns / 8
    c = np.zeros(n)
    c[:ns] = r.uniform(0.5, 1.5, ns)
    us = r.uniform(0.25, 0.75, ns)
    us[::4] = np.inf
    sl = b * r.uniform(1.02, 1.3, m)
    sl[np.arange(m) % 3 != 0] = np.inf
    u = np.concatenate([us, sl])
    return A, b, c, u


def cost_variant(c, ns, seed):
    """The cost re-solve case's second objective."""
    c2 = np.array(c, dtype=np.float64)
    c2[:ns] = c2[:ns] * np.random.default_rng(seed + 3000).uniform(0.5, 1.5, ns)
    return c2


def all_bounded(u, ns, cap=1.0, slack_cap=None):
    """u with every bound finite: `cap` for a structural column that had none,
    `slack_cap` (default ns) for a slack.  Every non-basic column then has a
    dual feasible side whatever the sign of its reduced cost."""
    u2 = np.array(u, dtype=np.float64)
    u2[:ns] = np.where(np.isfinite(u2[:ns]), u2[:ns], cap)
    u2[ns:] = np.where(np.isfinite(u2[ns:]), u2[ns:], float(ns) if slack_cap is None else slack_cap)
    return u2


def tiny_flip():
    """max 2 x0 + x1, x0 + x1 + s = 4, x0 <= 1, x1 <= 5.  Pass 1: x0 enters, the
    slack's ratio is 4 but u_0 = 1 comes first: a flip (x_b = 3).  Pass 2: x1
    enters, the slack leaves at t = 3 < u_1: a pivot.  x = (1, 3), z = 5."""
    A = np.array([[1.0, 1.0, 1.0]])
    return A, np.array([4.0]), np.array([2.0, 1.0, 0.0]), np.array([1.0, 5.0, np.inf])


def tiny_unbounded():
    """max x0, x0 - x1 + s = 1: x0 enters for the slack, then x1 enters with
    alpha = -1 against a basic column without an upper bound."""
    A = np.array([[1.0, -1.0, 1.0]])
    return A, np.array([1.0]), np.array([1.0, 1.0, 0.0]), np.array([np.inf, np.inf, np.inf])


def tiny_not_feasible():
    """The slack basis gives x_b = (2, -1): row 1 (its slack, column 3) is below 0."""
    A = np.array([[1.0, 1.0, 1.0, 0.0], [-1.0, -1.0, 0.0, 1.0]])
    return A, np.array([2.0, -1.0]), np.array([1.0, 1.0, 0.0, 0.0]), np.array([1.5, 1.5, np.inf, np.inf])


@dataclass
class PrimalBoxResult:
    status: str
    z: float
    pivots: int
    b_ixs: np.ndarray
    x_b: np.ndarray
    at_upper: np.ndarray            # n bools: non-basic at its upper bound
    trace: list = field(default_factory=list)
    gap_price: float = np.inf
    gap_ratio: float = np.inf
    gap_flip: float = np.inf
    flips: int = 0                  # flip passes
    to_upper: int = 0               # pivots whose row left to its upper bound
    bad_row: int = -1               # NOT_PRIMAL_FEASIBLE: the first row out of its bounds
    bad_column: int = -1            # ... and its basic column
    y: np.ndarray = None            # final duals and inverse
    Binv: np.ndarray = None
    # passes in which a decision met an exact tie: "price" (entering argmin), "ratio" (leaving-row argmin),
    # "flip" (u_p == t_q: the rule flips)
    ties: dict = field(default_factory=dict)
    integral: bool = True           # x_b, y and B^-1 held integers only after every pass

    def primal(self, u):
        x = np.where(self.at_upper, np.where(np.isfinite(u), u, 0.0), 0.0)
        x[self.b_ixs] = self.x_b
        return x


def primal_simplex_box(A, b, c, u, basis=None, at_upper=None, eps=1e-7, feas_tol=1e-9, piv_tol=1e-9,
                       max_iter=1 << 62, trace_cap=200):
    """From the slack basis with every column at lower, or from `basis` (m
    distinct columns, basis order) and the placements `at_upper`.  max_iter
    bounds the pivots."""
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
    up &= np.isfinite(u)  # a column at an upper bound that does not exist sits at lower
    c_B = c[b_ixs].copy()
    y = c_B @ Binv
    beff = b.copy()
    for j in np.flatnonzero(up):  # ascending j
        beff = beff - u[j] * A[:, j]
    x_b = Binv @ beff

    def result(status, it, **kw):
        z = float(c_B @ x_b)
        zu = 0.0
        for j in np.flatnonzero(up):  # ascending j
            zu += c[j] * u[j]
        return PrimalBoxResult(status, z + zu, it, b_ixs.copy(), x_b.copy(), up.copy(), trace, float(gap_price),
                               float(gap_ratio), float(gap_flip), flips, to_upper, y=y.copy(), Binv=Binv.copy(),
                               ties=ties, integral=integral, **kw)

    trace = []
    gap_price = gap_ratio = gap_flip = np.inf
    flips = to_upper = 0
    ties = {"price": 0, "ratio": 0, "flip": 0}
    integral = True
    it = 0
    # entry check
    bad = np.flatnonzero((x_b < -feas_tol) | (x_b > u[b_ixs] + feas_tol))
    if len(bad):
        return result(NOT_PRIMAL_FEASIBLE, 0, bad_row=int(bad[0]), bad_column=int(b_ixs[bad[0]]))

    status = MAX_ITER
    while it < max_iter:
        # 1. pricing
        d = y @ A - c
        sigma = np.where(up, -1.0, 1.0)
        key = np.where(~basic, sigma * d, np.inf)
        cand = key < -eps
        if not cand.any():
            status = OPTIMUM
            break
        key = np.where(cand, key, np.inf)
        p = int(np.argmin(key))  # smallest column on ties
        ties["price"] += int(tied(key))
        if cand.sum() > 1:
            two = np.partition(key, 1)[:2]
            gap_price = min(gap_price, _rel_gap(two[0], two[1]))
        sp = sigma[p]
        # 2. FTRAN
        alpha = Binv @ A[:, p]
        ahat = sp * alpha
        # 3. ratio test
        ub = u[b_ixs]
        lo = ahat > piv_tol
        hi = (ahat < -piv_tol) & np.isfinite(ub)
        t = np.full(m, np.inf)
        t[lo] = np.maximum(x_b[lo], 0.0) / ahat[lo]
        t[hi] = np.maximum(ub[hi] - x_b[hi], 0.0) / (-ahat[hi])
        rows = lo | hi
        q = int(np.argmin(t)) if rows.any() else -1  # first row on ties
        if rows.sum() > 1:
            two = np.partition(t, 1)[:2]
            gap_ratio = min(gap_ratio, _rel_gap(two[0], two[1]))
        u_p = u[p]
        if np.isfinite(u_p) and q >= 0:
            gap_flip = min(gap_flip, _rel_gap(u_p, t[q]))
            ties["flip"] += int(u_p == t[q])
        if q >= 0:
            ties["ratio"] += int(tied(t))
        # 4. flip
        if np.isfinite(u_p) and (q < 0 or u_p <= t[q]):
            x_b = x_b - u_p * ahat
            up[p] = not up[p]
            flips += 1
            integral = integral and whole(x_b)
            continue
        # 5. unbounded
        if q < 0:
            status = UNBOUNDED
            break
        # 6. pivot
        theta = t[q]
        rho = Binv[q].copy()
        aq = alpha[q]
        x_b = x_b - theta * ahat
        x_b[q] = (u_p if up[p] else 0.0) + sp * theta
        y = y - (d[p] / aq) * rho
        c_B[q] = c[p]
        leave = b_ixs[q]
        basic[leave] = False
        up[leave] = bool(hi[q])
        to_upper += int(hi[q])
        basic[p] = True
        up[p] = False
        b_ixs[q] = p
        Binv = Binv - np.outer(alpha / aq, rho)
        Binv[q] = rho / aq
        integral = integral and whole(x_b, y, Binv)
        if it < trace_cap:
            trace.append((p, q))
        it += 1
    return result(status, it)
