"""Dense numpy restatement of the bounded primal simplex loop with its composite
phase 1 priced by exact steepest edge (include/simplex.h: SPX_FLAG_PRIMAL_PHASE1
with SPX_PRIMAL_PRICING_STEEPEST and spx_set_primal_phase_one_pricing(STEEPEST);
DESIGN.md §7l).  Everything but the entering rule is tests/primal_phase1_ref.py
(its generators and its result type are used here), and the rule and the
weights are tests/primal_box_se_ref.py's:

  - a pass that starts with ninf > 0 is primal_phase1_ref's phase-1 pass (w, y1 =
    w.B^-1, d_j = y1.A_j without a cost term, candidates sigma_j d_j < -eps, the
    phase-aware ratio test, flips, INFEASIBLE on no candidate, BREAKDOWN on no
    row, y not maintained, rows classified again) except that p = argmin of
    -d_j^2 / gamma_j over the candidates, first column on ties;
  - a pass that starts with ninf == 0 is primal_box_se_ref's pass;
  - every pivot, in either phase, applies Goldfarb and Reid's update: gamma_p =
    1 + ||alpha||^2 recomputed, g = (rho.A_j) / alpha_q, gamma_j = max(gamma_j -
    2 g (tau.A_j) + g^2 gamma_p, 1 + g^2) for every j non-basic before the pivot
    and not p, the leaving column max(gamma_p / alpha_q^2, 1);
  - a flip changes no weight, and the switch to phase 2 keeps the weights.

The weights start at `weights`, or at 1 + ||A_j||^2 (exact at the slack basis, a
reference framework elsewhere); neither start depends on feasibility.
`gap_price` is taken on the steepest-edge key; `drift_enter` / `drift_final` are
primal_box_se_ref's (only meaningful when the starting weights were exact).
"""
from dataclasses import dataclass

import numpy as np

from dual_ref import MAX_ITER, OPTIMUM, tied, whole
from dual_se_ref import _rel_gap
from primal_box_se_ref import exact_weights, reference_weights
from primal_phase1_ref import (BREAKDOWN, INFEASIBLE, UNBOUNDED, Phase1Result, _classify,  # noqa: F401
                               boxed_general, certificate, contradict, rhs_variant, tiny_infeasible)


@dataclass
class Phase1SeResult(Phase1Result):
    weights: np.ndarray = None  # n: the recurrence weights (non-basic entries live)
    drift: float = 0.0
    drift_enter: float = 0.0    # ... on the entering columns alone
    drift_final: float = 0.0    # ... on the non-basic columns at the end


def primal_simplex_phase1_se(A, b, c, u, basis=None, at_upper=None, weights=None, eps=1e-7, feas_tol=1e-9,
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
    drift_enter = 0.0
    it = 0
    w = _classify(x_b, u[b_ixs], feas_tol)
    ninf = ninf0 = int(np.count_nonzero(w))

    def result(status):
        z = float(c_B @ x_b)
        zu = 0.0
        for j in np.flatnonzero(up):  # ascending j
            zu += c[j] * u[j]
        ex = exact_weights(A, Binv, basic)
        nb = ~basic
        drift_final = float(np.max(np.abs(gamma[nb] - ex[nb]) / ex[nb])) if nb.any() else 0.0
        return Phase1SeResult(status, z + zu, it, b_ixs.copy(), x_b.copy(), up.copy(), trace, float(gap_price),
                              float(gap_ratio), float(gap_flip), flips, to_upper, p1_passes, p1_pivots, ninf0, ninf, hist,
                              c_B @ Binv if y_stale else y.copy(), Binv.copy(), ties, integral,
                              weights=gamma.copy(), drift=max(drift_enter, drift_final), drift_enter=drift_enter,
                              drift_final=drift_final)

    def tie(name, hit, ph1):
        ties[name] += int(hit)
        if ph1:
            ties["p1_" + name] += int(hit)

    status = MAX_ITER
    while it < max_iter:
        ph1 = ninf > 0
        hist.append(ninf)
        # 1. pricing: the phase's reduced costs, the steepest-edge key
        if ph1:
            d = (w @ Binv) @ A
        else:
            if y_stale:
                y = c_B @ Binv
                y_stale = False
            d = y @ A - c
        sigma = np.where(up, -1.0, 1.0)
        cand = ~basic & (sigma * d < -eps)
        if not cand.any():
            status = INFEASIBLE if ph1 else OPTIMUM
            break
        key = np.where(cand, -(d * d) / gamma, np.inf)
        p = int(np.argmin(key))  # smallest column on ties
        tie("price", tied(key), ph1)
        if cand.sum() > 1:
            two = np.partition(key, 1)[:2]
            gap_price = min(gap_price, _rel_gap(two[0], two[1]))
        sp = sigma[p]
        # 2. FTRAN
        alpha = Binv @ A[:, p]
        ahat = sp * alpha
        gp = 1.0 + float(alpha @ alpha)
        # 3. ratio test (primal_phase1_ref's)
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
        # 4. flip: no weight changes
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
        # 7. the weights of the columns that were non-basic before the pivot, p excepted: either phase
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
        integral = integral and whole(x_b, y, Binv)
        if it < trace_cap:
            trace.append((p, q))
        it += 1
        if ph1:
            w = _classify(x_b, u[b_ixs], feas_tol)
            ninf = int(np.count_nonzero(w))
    return result(status)
