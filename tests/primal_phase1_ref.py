"""Dense numpy restatement of the bounded primal simplex loop with its composite
phase 1 (include/simplex.h, SPX_ALGO_PRIMAL_BOX with SPX_FLAG_PRIMAL_PHASE1;
DESIGN.md §7f), on the conventions of tests/primal_box_ref.py: maximise c.x,
A x = b with the slack identity in A's last m columns, 0 <= x <= u, explicit
B^-1, first index on every tie, no reinversion.

Row i with basic column k is *below* when x_b[i] < -feas_tol, *above* when
x_b[i] > u_k + feas_tol and feasible otherwise; ninf counts the below and above
rows.  A pass that starts with ninf > 0 is a phase-1 pass:

  1. w_i = +1 (below), -1 (above), 0 (feasible); y1 = w.B^-1; d_j = y1.A_j (no
     cost term); candidates are the non-basic sigma_j d_j < -eps, p = argmin
     sigma_j d_j.  None: INFEASIBLE.
  2. alpha = B^-1 A_p, ahat = sigma_p alpha; x_b moves by -t ahat.
  3. A feasible row blocks as in phase 2.  A below row blocks only when ahat_i <
     -piv_tol, at t_i = x_b[i] / ahat_i (it rises to 0 and leaves to its lower
     bound); an above row only when ahat_i > piv_tol, at t_i = (x_b[i] - u_k) /
     ahat_i (it falls to u_k and leaves to its upper bound).  q = argmin t_i.
  4. Flip, pivot: phase 2's.  No row and u_p = +inf: BREAKDOWN (cannot happen in
     exact arithmetic: the library's SPX_STATUS_THETA_OVERFLOW).
  5. y is not maintained.  The rows are classified again from the new x_b.

The first pass that starts with ninf == 0 recomputes y = c_B.B^-1 (if a phase-1
pivot happened since y was last current) and is an ordinary pass of
primal_box_ref.primal_simplex_box; from then on y is maintained and the rows are
not classified again.  `pivots`, the trace, `flips` and `to_upper` count both
phases.  `boxed_general` is the generator the tests share: its draws fix
tests/golden/primal_phase1_optima.json.
"""
from dataclasses import dataclass, field

import numpy as np

from dual_ref import MAX_ITER, OPTIMUM, tied, whole
from dual_se_ref import _rel_gap
from primal_box_ref import UNBOUNDED, certificate  # noqa: F401  (the tests take it from here)

INFEASIBLE = "infeasible"
BREAKDOWN = "breakdown"


def boxed_general(m, n, seed):
    """>= rows below 0 at the slack basis, ranged rows whose slack starts above
    its bound, profitable columns without an upper bound: the slack basis is
    neither primal nor dual feasible; x0 keeps the LP feasible."""
    r = np.random.default_rng(seed + 4000)
    ns = n - m
    A = np.zeros((m, n))
    A[:, :ns] = r.uniform(-0.5, 1.0, (m, ns))
    A[:, ns:] = np.eye(m)
    us = r.uniform(0.25, 0.75, ns)
    us[::4] = np.inf
    x0 = r.uniform(0, 0.25, ns)
    ax = A[:, :ns] @ x0
    f = r.uniform(1.1, 1.5, m)
    b = np.abs(ax) * f + 0.05 * ns / 8
    ge = (np.arange(m) % 3 == 1) & (ax > 0)
    A[ge, :ns] *= -1
    b[ge] = -(ax[ge] * r.uniform(0.5, 0.9, int(ge.sum())))
    c = np.zeros(n)
    c[:ns] = r.uniform(-0.5, 1.5, ns)
    sl = np.full(m, np.inf)
    rg = np.arange(m) % 3 == 0
    sl[rg] = np.abs(b[rg]) * r.uniform(0.3, 0.8, int(rg.sum()))
    u = np.concatenate([us, sl])
    return A, b, c, u


def boxed_general_tall(m, n, seed, every=300):
    """boxed_general() for m far above n - m (tests/test_gpu_lds_cap.py: n = m +
    64), where a third of thousands of rows out of their bounds would take
    phase 1 thousands of pivots: the same kinds of row in the same order of
    draws, but only every `every`-th row is a >= row below 0 or a ranged row
    whose slack starts above its bound; the other ranged rows get bounds their
    slack starts inside (primal_box_ref.boxed_primal's 1.02 .. 1.3 b)."""
    r = np.random.default_rng(seed + 4000)
    ns = n - m
    A = np.zeros((m, n))
    A[:, :ns] = r.uniform(-0.5, 1.0, (m, ns))
    A[:, ns:] = np.eye(m)
    us = r.uniform(0.25, 0.75, ns)
    us[::4] = np.inf
    x0 = r.uniform(0, 0.25, ns)
    ax = A[:, :ns] @ x0
    f = r.uniform(1.1, 1.5, m)
    b = np.abs(ax) * f + 0.05 * ns / 8
    i = np.arange(m)
    ge = (i % every == 1) & (ax > 0)
    A[ge, :ns] *= -1
    b[ge] = -(ax[ge] * r.uniform(0.5, 0.9, int(ge.sum())))
    c = np.zeros(n)
    c[:ns] = r.uniform(-0.5, 1.5, ns)
    sl = np.full(m, np.inf)
    rg = (i % 3 == 0) & ~ge
    tight = r.uniform(0.3, 0.8, m)
    wide = r.uniform(1.02, 1.3, m)
    sl[rg] = np.abs(b[rg]) * np.where(i[rg] % every == 0, tight[rg], wide[rg])
    u = np.concatenate([us, sl])
    return A, b, c, u


def contradict(A, b, u):
    """boxed_general's LP made infeasible: row 1 = -row 0 on the structural
    columns, b0 = 1, b1 = -2, both slacks without a bound (r0.x <= 1 and
    r0.x >= 2)."""
    A = A.copy()
    b = b.copy()
    u = u.copy()
    m, n = A.shape
    ns = n - m
    A[1, :ns] = -A[0, :ns]
    b[0], b[1] = 1.0, -2.0
    u[ns], u[ns + 1] = np.inf, np.inf
    return A, b, u


def tiny_infeasible():
    """x0 + s = -1, x0 <= 2: the slack is below 0 and x0 can only lower it."""
    A = np.array([[1.0, 1.0]])
    return A, np.array([-1.0]), np.array([1.0, 0.0]), np.array([2.0, np.inf])


def rhs_variant(b, seed):
    """The stuck warm start's second right-hand side."""
    return b * np.random.default_rng(seed + 5000).uniform(0.6, 1.4, len(b))


@dataclass
class Phase1Result:
    status: str
    z: float
    pivots: int
    b_ixs: np.ndarray
    x_b: np.ndarray
    at_upper: np.ndarray
    trace: list = field(default_factory=list)
    gap_price: float = np.inf
    gap_ratio: float = np.inf
    gap_flip: float = np.inf
    flips: int = 0
    to_upper: int = 0
    p1_passes: int = 0   # phase-1 passes, flip passes included
    p1_pivots: int = 0
    ninf0: int = 0       # infeasible rows at entry
    ninf: int = 0        # ... at the end
    ninf_hist: list = field(default_factory=list)  # ninf at the start of every pass
    y: np.ndarray = None   # final duals (c_B.B^-1 where phase 1 left y stale, as the library reads it back) and inverse
    Binv: np.ndarray = None
    # passes in which a decision met an exact tie: "price", "ratio", "flip" (u_p == t_q) as in
    # tests/primal_box_ref.py over both phases, "p1_price", "p1_ratio", "p1_flip" over the phase-1 passes alone
    ties: dict = field(default_factory=dict)
    integral: bool = True  # x_b, y and B^-1 held integers only after every pass

    def primal(self, u):
        x = np.where(self.at_upper, np.where(np.isfinite(u), u, 0.0), 0.0)
        x[self.b_ixs] = self.x_b
        return x


def _classify(x_b, ub, feas_tol):
    return np.where(x_b < -feas_tol, 1.0, np.where(x_b > ub + feas_tol, -1.0, 0.0))


def primal_simplex_phase1(A, b, c, u, basis=None, at_upper=None, eps=1e-7, feas_tol=1e-9, piv_tol=1e-9,
                          max_iter=1 << 62, trace_cap=200):
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
    up &= np.isfinite(u)
    c_B = c[b_ixs].copy()
    y = c_B @ Binv
    y_stale = False
    beff = b.copy()
    for j in np.flatnonzero(up):  # ascending j
        beff = beff - u[j] * A[:, j]
    x_b = Binv @ beff

    trace = []
    gap_price = gap_ratio = gap_flip = np.inf
    flips = to_upper = p1_passes = p1_pivots = 0
    ties = {"price": 0, "ratio": 0, "flip": 0, "p1_price": 0, "p1_ratio": 0, "p1_flip": 0}
    integral = True
    hist = []
    it = 0
    w = _classify(x_b, u[b_ixs], feas_tol)
    ninf = ninf0 = int(np.count_nonzero(w))

    def result(status):
        z = float(c_B @ x_b)
        zu = 0.0
        for j in np.flatnonzero(up):  # ascending j
            zu += c[j] * u[j]
        return Phase1Result(status, z + zu, it, b_ixs.copy(), x_b.copy(), up.copy(), trace, float(gap_price),
                            float(gap_ratio), float(gap_flip), flips, to_upper, p1_passes, p1_pivots, ninf0, ninf, hist,
                            c_B @ Binv if y_stale else y.copy(), Binv.copy(), ties, integral)

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
        sigma = np.where(up, -1.0, 1.0)
        key = np.where(~basic, sigma * d, np.inf)
        cand = key < -eps
        if not cand.any():
            status = INFEASIBLE if ph1 else OPTIMUM
            break
        key = np.where(cand, key, np.inf)
        p = int(np.argmin(key))
        tie("price", tied(key), ph1)
        if cand.sum() > 1:
            two = np.partition(key, 1)[:2]
            gap_price = min(gap_price, _rel_gap(two[0], two[1]))
        sp = sigma[p]
        # 2. FTRAN
        alpha = Binv @ A[:, p]
        ahat = sp * alpha
        # 3. ratio test
        ub = u[b_ixs]
        feas = w == 0.0 if ph1 else np.ones(m, dtype=bool)
        lo = feas & (ahat > piv_tol)
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
            integral = integral and whole(x_b)
            if ph1:
                w = _classify(x_b, u[b_ixs], feas_tol)
                ninf = int(np.count_nonzero(w))
            continue
        # 5. no row
        if q < 0:
            p1_passes -= int(ph1)  # (the pass committed nothing)
            status = BREAKDOWN if ph1 else UNBOUNDED
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
        if ph1:
            w = _classify(x_b, u[b_ixs], feas_tol)
            ninf = int(np.count_nonzero(w))
    return result(status)
