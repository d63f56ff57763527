"""Dense numpy restatement of the bounded primal simplex loop with general bounds
l <= x <= u, free columns included, priced by exact steepest edge in both phases
(include/simplex.h: spx_set_bounds_lu under SPX_ALGO_PRIMAL_BOX with
SPX_PRIMAL_PRICING_STEEPEST and spx_set_primal_free_pricing(STEEPEST); with phase
1 also spx_set_primal_phase_one_pricing(STEEPEST)).

Everything but the entering column is tests/primal_lu_ref.py primal_simplex_lu:
the shift, the free rule (who is a candidate, sigma_p, which rows block), the
phase-aware ratio test, flips, the statuses, the counters and the readbacks.  The
candidates are its candidates (key below -eps, a free column's key being
-|d_j|); among them p = argmin -d_j^2 / gamma_j, first column on ties, in phase 1
(d_j = y1.A_j, no cost term) and in phase 2.

The weights are tests/primal_phase1_se_ref.py's: every pivot of either phase
recomputes gamma_p = 1 + ||alpha||^2, g = (rho.A_j) / alpha_q, gamma_j =
max(gamma_j - 2 g (tau.A_j) + g^2 gamma_p, 1 + g^2) for every j non-basic before
the pivot and not p, and the leaving column (never free) gets max(gamma_p /
alpha_q^2, 1).  A flip changes no weight, the switch to phase 2 keeps them.  They
start at `weights`, or at 1 + ||A_j||^2 (exact at the slack basis); no start looks
at a bound.

With no free column every line computes what primal_simplex_phase1_se computes on
the shifted LP, in the same order.  `gap_price` is taken on the steepest-edge
key; `drift_enter` / `drift_final` are primal_box_se_ref's.
"""
from dataclasses import dataclass

import numpy as np

from dual_ref import MAX_ITER, OPTIMUM, tied, whole
from dual_se_ref import _rel_gap
from primal_box_ref import UNBOUNDED, boxed_primal
from primal_box_se_ref import exact_weights, reference_weights
from primal_lu_ref import (BREAKDOWN, INFEASIBLE, LuResult, _classify, certificate_lu, general_lu,  # noqa: F401
                           tiny_unbounded_free)


def free_feasible(m, n, seed):
    """boxed_primal(m, n, seed) with free columns, returned as (A, b, c, l, u):
    structural column j with j % 5 == 2 is free with a cost of either sign, and
    every slack without a bound gets the wide one |b_i| + (n - m) / 4 (all rows
    ranged: the LP stays bounded).  The slack basis stays primal feasible, so the
    loop runs it with phase 1 off."""
    A, b, c, u = boxed_primal(m, n, seed)
    r = np.random.default_rng(seed + 9900)
    ns = n - m
    cf = r.uniform(-1.0, 1.0, ns)
    is_free = np.arange(ns) % 5 == 2
    l = np.zeros(n)
    u = u.copy()
    c = c.copy()
    l[:ns][is_free] = -np.inf
    u[:ns][is_free] = np.inf
    c[:ns][is_free] = cf[is_free]
    wide = ~np.isfinite(u[ns:])
    u[ns:][wide] = np.abs(b[wide]) + 0.25 * ns
    return A, b, c, l, u


def free_tie():
    """free_feasible(7, 20, 0) with its free column 2 duplicated in position 3
    (column, cost and bounds): the two are candidates together with d_j and
    gamma_j, so keys, that are the same bits, and the smaller index enters."""
    A, b, c, l, u = free_feasible(7, 20, 0)
    A[:, 3], c[3], l[3], u[3] = A[:, 2], c[2], l[2], u[2]
    return A, b, c, l, u


@dataclass
class LuSeResult(LuResult):
    weights: np.ndarray = None  # n: the recurrence weights (non-basic entries live)
    drift_enter: float = 0.0    # largest relative error of an entering column's weight against 1 + ||alpha||^2
    drift_final: float = 0.0    # ... of the non-basic columns' weights at the end against exact_weights


def primal_simplex_lu_se(A, b, c, l, u, basis=None, at_upper=None, weights=None, eps=1e-7, feas_tol=1e-9,
                         piv_tol=1e-9, max_iter=1 << 62, trace_cap=200):
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    l = np.asarray(l, dtype=np.float64)
    uu = np.asarray(u, dtype=np.float64)
    m, n = A.shape
    ns = n - m
    free = np.isneginf(l)
    assert not np.any(free & np.isfinite(uu)) and not np.any(l > uu) and not np.any(np.isposinf(l))
    lsh = np.where(free, 0.0, l)
    u = np.where(np.isfinite(uu), uu - lsh, np.inf)
    lo0 = np.where(free, -np.inf, 0.0)
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
    drift_enter = 0.0
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
        ex = exact_weights(A, Binv, basic)
        nb = ~basic
        drift_final = float(np.max(np.abs(gamma[nb] - ex[nb]) / ex[nb])) if nb.any() else 0.0
        return LuSeResult(status, z + (zu + zl), it, b_ixs.copy(), x_b + lsh[b_ixs], up.copy(),
                          trace, float(gap_price), float(gap_ratio), float(gap_flip), flips, to_upper, p1_passes,
                          p1_pivots, ninf0, ninf, hist, c_B @ Binv if y_stale else y.copy(), Binv.copy(), ties, integral,
                          x_b.copy(), free_entered, int(np.count_nonzero(free[b_ixs])), fixed_flips, ray_col,
                          weights=gamma.copy(), drift_enter=drift_enter, drift_final=drift_final)

    def tie(name, hit, ph1):
        ties[name] += int(hit)
        if ph1:
            ties["p1_" + name] += int(hit)

    status = MAX_ITER
    while it < max_iter:
        ph1 = ninf > 0
        hist.append(ninf)
        # 1. pricing: primal_simplex_lu's candidates, the steepest-edge key
        if ph1:
            d = (w @ Binv) @ A
        else:
            if y_stale:
                y = c_B @ Binv
                y_stale = False
            d = y @ A - c
        sigma = np.where(free, np.where(d < 0.0, 1.0, -1.0), np.where(up, -1.0, 1.0))
        cand = ~basic & (np.where(free, -np.abs(d), sigma * d) < -eps)
        if not cand.any():
            status = INFEASIBLE if ph1 else OPTIMUM
            break
        key = np.where(cand, -(d * d) / gamma, np.inf)
        p = int(np.argmin(key))  # smallest column on ties
        tie("price", tied(key), ph1)
        ties["free_price"] += int(tied(key) and bool(np.any(free & (key == key[p]))))
        if cand.sum() > 1:
            two = np.partition(key, 1)[:2]
            gap_price = min(gap_price, _rel_gap(two[0], two[1]))
        sp = sigma[p]
        # 2. FTRAN
        alpha = Binv @ A[:, p]
        ahat = sp * alpha
        gp = 1.0 + float(alpha @ alpha)
        # 3. ratio test (primal_simplex_lu's)
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
        # 4. flip: no weight changes
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
        drift_enter = max(drift_enter, abs(gamma[p] - gp) / gp)
        theta = t[q]
        rho = Binv[q].copy()
        tau = alpha @ Binv
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
        # 7. the weights of the columns that were non-basic before the pivot, p excepted: either phase, any bounds
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
