"""Dense numpy restatement of the dual simplex loop with dual steepest-edge
pricing (include/simplex.h, SPX_DUAL_PRICING_STEEPEST): tests/dual_ref.py's
loop with the leaving row

    q = argmax x_b[i]^2 / w_i  over x_b[i] < -feas_tol,   w_i = ||row_i(B^-1)||^2

(first index on ties), the same ratio test, explicit B^-1, no reinversion.  The
weights used for the choice are the exact squared row norms of the current
inverse; the library's update formula

    w'_i = max(w_i - 2 r_i tau_i + r_i^2 w_q, floor)  (i != q),  w'_q = w_q / alpha_q^2
    r_i = alpha_i / alpha_q,  tau = B^-1 rho,  w_q = rho.rho

is evaluated beside them (`update_err`: its largest relative distance from the
next inverse's row norms over the solve).  `gap_row` / `gap_ratio` are the
smallest relative gaps between the best and the second-best key of the two
argmins: pivot-for-pivot comparison with another implementation is legitimate
only while they stay far above fp64 summation-order noise.
"""
from dataclasses import dataclass, field

import numpy as np

from dual_ref import INFEASIBLE, MAX_ITER, OPTIMUM, tied, whole

W_FLOOR = 1e-300


@dataclass
class DualSEResult:
    status: str
    z: float
    pivots: int
    b_ixs: np.ndarray
    x_b: np.ndarray
    trace: list = field(default_factory=list)
    gap_row: float = np.inf
    gap_ratio: float = np.inf
    update_err: float = 0.0
    weights: np.ndarray = None  # exact weights of the final basis
    y: np.ndarray = None        # final duals and inverse
    Binv: np.ndarray = None
    ties: dict = field(default_factory=dict)  # passes whose argmin met an exact tie: "row", "ratio"
    integral: bool = True       # x_b, y and B^-1 held integers only after every pass


def row_norms2(Binv):
    return np.einsum("ij,ij->i", Binv, Binv)


def update_weights(w, alpha, q, rho, tau):
    """The library's weight update for a pivot on row q (see the module text)."""
    aq = alpha[q]
    wq = float(rho @ rho)
    r = alpha / aq
    out = np.maximum(w - 2.0 * r * tau + r * r * wq, W_FLOOR)
    out[q] = wq / (aq * aq)
    return out


def _rel_gap(k1, k2):
    """|k1 - k2| relative to the larger magnitude (0 when both keys are 0)."""
    big = max(abs(k1), abs(k2))
    return 0.0 if big == 0.0 else abs(k1 - k2) / big


def dual_simplex_se(A, b, c, basis=None, feas_tol=1e-9, piv_tol=1e-9, max_iter=1 << 62, trace_cap=200,
                    check_update=False):
    """From the slack basis, or from `basis` (m distinct columns, basis order;
    it must be dual feasible)."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    m, n = A.shape
    ns = n - m
    if basis is None:
        b_ixs = np.arange(ns, n)
        Binv = np.eye(m)
    else:
        b_ixs = np.array(basis, dtype=np.int64)
        Binv = np.linalg.inv(A[:, b_ixs])
    x_b = Binv @ b
    c_B = c[b_ixs].copy()
    y = c_B @ Binv
    basic = np.zeros(n, dtype=bool)
    basic[b_ixs] = True
    trace = []
    gap_row = gap_ratio = np.inf
    update_err = 0.0
    ties = {"row": 0, "ratio": 0}
    integral = True
    it = 0
    status = MAX_ITER
    while it < max_iter:
        # 1. leaving row: argmin -x_b^2 / w over x_b < -feas_tol (first index)
        w = row_norms2(Binv)
        rows = x_b < -feas_tol
        if not rows.any():
            status = OPTIMUM
            break
        rkey = np.where(rows, -(x_b * x_b) / w, np.inf)
        q = int(np.argmin(rkey))
        ties["row"] += int(tied(rkey))
        if rows.sum() > 1:
            two = np.partition(rkey, 1)[:2]
            gap_row = min(gap_row, _rel_gap(two[0], two[1]))
        # 2. pivot row
        rho = Binv[q].copy()
        # 3. dual ratio test over the non-basic columns
        a = rho @ A
        d = y @ A - c
        cand = (~basic) & (a < -piv_tol)
        if not cand.any():
            status = INFEASIBLE
            break
        key = np.where(cand, np.maximum(d, 0.0) / np.where(cand, -a, 1.0), np.inf)
        p = int(np.argmin(key))  # smallest column index on ties
        ties["ratio"] += int(tied(key))
        if cand.sum() > 1:
            two = np.partition(key, 1)[:2]
            gap_ratio = min(gap_ratio, _rel_gap(two[0], two[1]))
        # 4. FTRAN and update
        alpha = Binv @ A[:, p]
        aq = alpha[q]
        if check_update:
            w_next = update_weights(w, alpha, q, rho, Binv @ rho)
        theta = x_b[q] / aq
        x_b = x_b - theta * alpha
        x_b[q] = theta
        y = y - (d[p] / aq) * rho
        c_B[q] = c[p]
        basic[b_ixs[q]] = False
        basic[p] = True
        b_ixs[q] = p
        Binv = Binv - np.outer(alpha / aq, rho)
        Binv[q] = rho / aq
        if check_update:
            exact = row_norms2(Binv)
            update_err = max(update_err, float(np.max(np.abs(w_next - exact) / exact)))
        integral = integral and whole(x_b, y, Binv)
        if it < trace_cap:
            trace.append((p, q))
        it += 1
    return DualSEResult(status, float(c_B @ x_b), it, b_ixs.copy(), x_b.copy(), trace, float(gap_row),
                        float(gap_ratio), update_err, row_norms2(Binv), y.copy(), Binv.copy(), ties, integral)
