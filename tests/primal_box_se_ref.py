"""Dense numpy restatement of the bounded primal simplex loop with exact primal
steepest-edge pricing (include/simplex.h SPX_PRIMAL_PRICING_STEEPEST; DESIGN.md
§7h).  Everything but the entering rule is tests/primal_box_ref.py: explicit
B^-1, the two-sided ratio test with a pivot tolerance, bound flips, first index
on every tie, no reinversion; the LPs are primal_box_ref.boxed_primal's.

Weights: gamma_j = 1 + ||B^-1 A_j||^2 for the non-basic columns, independent of
the bound a column sits at; a flip pass changes none.

One pass:
  1. d_j = y.A_j - c_j, candidates are the non-basic sigma_j d_j < -eps (none:
     optimum), p = argmin of -d_j^2 / gamma_j over them, first column on ties.
  2. - 6. as primal_box_ref (FTRAN, ratio test, flip, unbounded, pivot).
  7. After a pivot on row q, with alpha = B^-1 A_p, rho = row q of B^-1 and tau =
     alpha^T B^-1 (both of the B^-1 before the pivot) and gamma_p = 1 +
     ||alpha||^2 recomputed exactly: for every j non-basic before the pivot and
     not p, g = (rho.A_j) / alpha_q and gamma_j = max(gamma_j - 2 g (tau.A_j) +
     g^2 gamma_p, 1 + g^2); the leaving column gets max(gamma_p / alpha_q^2, 1)
     (Goldfarb and Reid).

From the slack basis the weights start at 1 + ||A_j||^2, which is exact there;
from a given basis they start at `weights`, or at 1 + ||A_j||^2 again (a
reference framework, not the exact norm: what the library does where no pass
has kept the weights).

`gap_price` is taken on the steepest-edge key.  `drift` is the largest relative
difference between a recurrence weight and the exactly recomputed 1 + ||B^-1
A_j||^2, measured on each entering column during the solve and on all non-basic
columns at the end (only meaningful when the starting weights were exact).
"""
from dataclasses import dataclass

import numpy as np

from dual_ref import MAX_ITER, OPTIMUM, tied
from dual_se_ref import _rel_gap
from primal_box_ref import NOT_PRIMAL_FEASIBLE, UNBOUNDED, PrimalBoxResult, boxed_primal  # noqa: F401


@dataclass
class PrimalBoxSeResult(PrimalBoxResult):
    weights: np.ndarray = None      # n: the recurrence weights (non-basic entries live)
    drift: float = 0.0
    drift_enter: float = 0.0        # ... on the entering columns alone
    drift_final: float = 0.0        # ... on the non-basic columns at the end


def exact_weights(A, Binv, basic):
    """1 + ||B^-1 A_j||^2 for every column (basic entries are 2: a unit vector)."""
    W = Binv @ A
    g = 1.0 + np.einsum("ij,ij->j", W, W)
    return np.where(basic, 2.0, g)


def reference_weights(A):
    return 1.0 + np.einsum("ij,ij->j", A, A)


def primal_simplex_box_se(A, b, c, u, basis=None, at_upper=None, weights=None, eps=1e-7, feas_tol=1e-9,
                          piv_tol=1e-9, max_iter=1 << 62, trace_cap=200):
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
    gamma = reference_weights(A) if weights is None else np.array(weights, dtype=np.float64)
    up = np.zeros(n, dtype=bool) if at_upper is None else np.array(at_upper, dtype=bool)
    basic = np.zeros(n, dtype=bool)
    basic[b_ixs] = True
    up &= ~basic
    up &= np.isfinite(u)
    c_B = c[b_ixs].copy()
    y = c_B @ Binv
    beff = b.copy()
    for j in np.flatnonzero(up):  # ascending j
        beff = beff - u[j] * A[:, j]
    x_b = Binv @ beff

    trace = []
    gap_price = gap_ratio = gap_flip = np.inf
    flips = to_upper = 0
    ties = {"price": 0, "ratio": 0, "flip": 0}
    drift_enter = 0.0
    it = 0

    def result(status, **kw):
        z = float(c_B @ x_b)
        zu = 0.0
        for j in np.flatnonzero(up):  # ascending j
            zu += c[j] * u[j]
        ex = exact_weights(A, Binv, basic)
        nb = ~basic
        drift_final = float(np.max(np.abs(gamma[nb] - ex[nb]) / ex[nb])) if nb.any() else 0.0
        return PrimalBoxSeResult(status, z + zu, it, b_ixs.copy(), x_b.copy(), up.copy(), trace, float(gap_price),
                                 float(gap_ratio), float(gap_flip), flips, to_upper, y=y.copy(), Binv=Binv.copy(),
                                 ties=ties, weights=gamma.copy(), drift=max(drift_enter, drift_final),
                                 drift_enter=drift_enter, drift_final=drift_final, **kw)

    bad = np.flatnonzero((x_b < -feas_tol) | (x_b > u[b_ixs] + feas_tol))
    if len(bad):
        return result(NOT_PRIMAL_FEASIBLE, bad_row=int(bad[0]), bad_column=int(b_ixs[bad[0]]))

    status = MAX_ITER
    while it < max_iter:
        # 1. pricing
        d = y @ A - c
        sigma = np.where(up, -1.0, 1.0)
        cand = ~basic & (sigma * d < -eps)
        if not cand.any():
            status = OPTIMUM
            break
        key = np.where(cand, -(d * d) / gamma, np.inf)
        p = int(np.argmin(key))  # smallest column on ties
        ties["price"] += int(tied(key))
        if cand.sum() > 1:
            two = np.partition(key, 1)[:2]
            gap_price = min(gap_price, _rel_gap(two[0], two[1]))
        sp = sigma[p]
        # 2. FTRAN
        alpha = Binv @ A[:, p]
        ahat = sp * alpha
        gp = 1.0 + float(alpha @ alpha)
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
        # 4. flip: no weight changes
        if np.isfinite(u_p) and (q < 0 or u_p <= t[q]):
            x_b = x_b - u_p * ahat
            up[p] = not up[p]
            flips += 1
            continue
        # 5. unbounded
        if q < 0:
            status = UNBOUNDED
            break
        # 6. pivot
        drift_enter = max(drift_enter, abs(gamma[p] - gp) / gp)
        theta = t[q]
        rho = Binv[q].copy()
        tau = alpha @ Binv
        aq = alpha[q]
        x_b = x_b - theta * ahat
        x_b[q] = (u_p if up[p] else 0.0) + sp * theta
        y = y - (d[p] / aq) * rho
        c_B[q] = c[p]
        leave = b_ixs[q]
        # 7. the weights of the columns that were non-basic before the pivot, p excepted
        nbv = ~basic
        nbv[p] = False
        g = (rho @ A) / aq
        new = np.maximum(gamma - 2.0 * g * (tau @ A) + g * g * gp, 1.0 + g * g)
        gamma = np.where(nbv, new, gamma)
        gamma[leave] = max(gp / (aq * aq), 1.0)
        basic[leave] = False
        up[leave] = bool(hi[q])
        to_upper += int(hi[q])
        basic[p] = True
        up[p] = False
        b_ixs[q] = p
        Binv = Binv - np.outer(alpha / aq, rho)
        Binv[q] = rho / aq
        if it < trace_cap:
            trace.append((p, q))
        it += 1
    return result(status)
