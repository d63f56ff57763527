"""Dense numpy restatement of the bounded primal simplex loop with general bounds
l <= x <= u under either entering rule and either phase-1 ratio test
(include/simplex.h: SPX_ALGO_PRIMAL_BOX with phase 1 on,
spx_set_primal_phase_one_ratio).

primal_simplex_long(A, b, c, l, u, pricing="dantzig" | "steepest", ratio=
"textbook" | "long").  With ratio="textbook" every line computes what
tests/primal_lu_ref.py primal_simplex_lu (dantzig) or tests/primal_lu_se_ref.py
primal_simplex_lu_se (steepest) computes, in the same order: the shift, the free
rule, the candidates, the weights' recurrence, flips, statuses and counters are
theirs.  ratio="long" changes the leaving row of a phase-1 pass only:

  soft breakpoint  an infeasible row reaches the bound it violates (the textbook
                   entry): a below row with ahat_i < -piv_tol at x_i / ahat_i,
                   side 0; an above row with ahat_i > piv_tol at (x_i - u_i) /
                   ahat_i, side 1.
  hard breakpoint  every entry of a feasible row (the textbook formulas, the free
                   rule included), and the far bound of a row with a soft
                   breakpoint: a below row with finite u_i at (x_i - u_i) /
                   ahat_i, side 1; an above row at x_i / ahat_i, side 0.
  h                the hard minimum in (t, 2 row + side) order.
  the walk         over the soft breakpoints before h in that order, from slope =
                   sigma_p d_p (< 0): slope += |ahat_i|; the first with slope >=
                   -eps leaves at its t and side, any other is passed.  No
                   leaving row: h leaves, or with no hard entry the last soft one.

The flip test u_p <= t_q, the commit and the classification are unchanged.

Recorded beside the neighbours' fields: `gap_walk`, the smallest relative gap
between a leaving breakpoint and its neighbours in the merged (soft and hard)
order; `gap_slope`, the smallest |slope + eps| / (|s0| + sum of |ahat| walked)
over the visited breakpoints; ties["p1_walk"], the long-step passes in which two
neighbours of the merged order, up to the entry after the leaving one, have the
same t; the walk counters; `walks`, per long-step pass the visited 2 row + side in
order and the leaving one; `sinf_hist` / `step_hist`, the sum of violations at the
start of every pass and whether the pass moved (theta or u_p > 0).
"""
from dataclasses import dataclass, field

import numpy as np

from dual_ref import MAX_ITER, OPTIMUM, tied, whole
from dual_se_ref import _rel_gap
from primal_box_ref import UNBOUNDED
from primal_box_se_ref import exact_weights, reference_weights
from primal_lu_ref import BREAKDOWN, INFEASIBLE, _classify, certificate_lu, general_lu  # noqa: F401
from primal_lu_se_ref import LuSeResult
from primal_phase1_ref import boxed_general, contradict  # noqa: F401


def lp_of(family, m, n, seed):
    """(A, b, c, l, u) of a golden family: `boxed_general` (lower bounds 0) or
    `general_lu` (general bounds, a fifth of the structural columns free)."""
    if family == "boxed_general":
        A, b, c, u = boxed_general(m, n, seed)
        return A, b, c, np.zeros(n), u
    assert family == "general_lu"
    return general_lu(m, n, seed)


def long_tie():
    """A hand-built integer LP (7 rows, 4 structural columns, lower bounds 0, no
    upper bound but one) whose first two passes from the slack basis walk through
    exact ties.  Returns (A, b, c, l, u).

    Pass 1: column 0 enters (d = -3, the most negative, under either rule); rows
    0 and 1 are below with soft breakpoints at the same t = 2 (-2 / -1 and -4 /
    -2).  Row 0 (2 row + side = 0) goes first and is passed (slope -3 -> -2), row 1
    (2) takes the slope to 0 and leaves: q = 1.  The other order would pass row 1
    (-1) and take row 0.
    Pass 2: column 1 enters (d = -2); row 4 is below with its soft breakpoint at
    t = 3 (2 row + side = 8) and row 5 is feasible with its hard breakpoint at
    the same t = 3 (10).  The soft one goes first and is passed (slope -2 -> -1),
    then h ends the walk and leaves: q = 5, one row passed.  The other order
    would pass nothing.
    Rows 3 and 6 stay out of their bounds until columns 2 and 3 enter, so the
    solve goes on to an optimum."""
    m, ns = 7, 4
    A = np.zeros((m, ns + m))
    A[:, ns:] = np.eye(m)
    A[0, 0], A[1, 0], A[2, 0], A[3, 0] = -1.0, -2.0, -1.0, 1.0
    A[3, 2] = -1.0
    A[4, 1], A[5, 1], A[6, 1] = -1.0, 1.0, -1.0
    A[6, 3] = -1.0
    b = np.array([-2.0, -4.0, -10.0, -1.0, -3.0, 3.0, -10.0])
    c = np.concatenate([[-1.0, -1.0, -1.0, -1.0], np.zeros(m)])
    l = np.zeros(ns + m)
    u = np.full(ns + m, np.inf)
    return A, b, c, l, u


@dataclass
class LongResult(LuSeResult):
    gap_walk: float = np.inf
    gap_slope: float = np.inf
    long_passed: int = 0   # rows the walk passed
    long_passes: int = 0   # passes that passed at least one
    long_max: int = 0      # the most in one pass
    walks: list = field(default_factory=list)      # per long-step pass: (visited 2 row + side in order, the leaving one)
    sinf_hist: list = field(default_factory=list)  # the sum of violations at the start of every pass
    step_hist: list = field(default_factory=list)  # per committed pass: (phase 1?, moved?)

    def long_counters(self, rule):
        return (self.long_passed, self.long_passes, self.long_max, rule)


def _sinf(x_b, lo, ub):
    below = np.where(np.isfinite(lo), np.maximum(lo - x_b, 0.0), 0.0)
    above = np.where(np.isfinite(ub), np.maximum(x_b - ub, 0.0), 0.0)
    return float(below.sum() + above.sum())


def primal_simplex_long(A, b, c, l, u, pricing="dantzig", ratio="textbook", switch_at=None, eps=1e-7, feas_tol=1e-9,
                        piv_tol=1e-9, max_iter=1 << 62, trace_cap=200):
    """`switch_at`: the ratio test is "textbook" until that many pivots are made,
    then `ratio`."""
    assert pricing in ("dantzig", "steepest") and ratio in ("textbook", "long")
    steep = pricing == "steepest"
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
    b_ixs = np.arange(ns, n)
    Binv = np.eye(m)
    gamma = reference_weights(A) if steep else np.ones(n)
    up = np.zeros(n, dtype=bool)
    basic = np.zeros(n, dtype=bool)
    basic[b_ixs] = True
    c_B = c[b_ixs].copy()
    y = c_B @ Binv
    y_stale = False
    beff = b.copy()
    for j in range(n):  # ascending j
        if lsh[j] != 0.0:
            beff = beff - lsh[j] * A[:, j]
    x_b = Binv @ beff

    trace = []
    gap_price = gap_ratio = gap_flip = gap_walk = gap_slope = np.inf
    flips = to_upper = p1_passes = p1_pivots = 0
    ties = {"price": 0, "ratio": 0, "flip": 0, "p1_price": 0, "p1_ratio": 0, "p1_flip": 0, "free_price": 0, "p1_walk": 0}
    free_entered = fixed_flips = 0
    long_passed = long_passes = long_max = 0
    walks, sinf_hist, step_hist = [], [], []
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
        drift_final = 0.0
        if steep:
            ex = exact_weights(A, Binv, basic)
            nb = ~basic
            drift_final = float(np.max(np.abs(gamma[nb] - ex[nb]) / ex[nb])) if nb.any() else 0.0
        return LongResult(status, z + (zu + zl), it, b_ixs.copy(), x_b + lsh[b_ixs], up.copy(),
                          trace, float(gap_price), float(gap_ratio), float(gap_flip), flips, to_upper, p1_passes,
                          p1_pivots, ninf0, ninf, hist, c_B @ Binv if y_stale else y.copy(), Binv.copy(), ties, integral,
                          x_b.copy(), free_entered, int(np.count_nonzero(free[b_ixs])), fixed_flips, ray_col,
                          weights=gamma.copy(), drift_enter=drift_enter, drift_final=drift_final,
                          gap_walk=float(gap_walk), gap_slope=float(gap_slope), long_passed=long_passed,
                          long_passes=long_passes, long_max=long_max, walks=walks, sinf_hist=sinf_hist,
                          step_hist=step_hist)

    def tie(name, hit, ph1):
        ties[name] += int(hit)
        if ph1:
            ties["p1_" + name] += int(hit)

    status = MAX_ITER
    while it < max_iter:
        ph1 = ninf > 0
        hist.append(ninf)
        sinf_hist.append(_sinf(x_b, lo0[b_ixs], u[b_ixs]))
        lng = ph1 and ratio == "long" and (switch_at is None or it >= switch_at)
        # 1. pricing
        if ph1:
            d = (w @ Binv) @ A
        else:
            if y_stale:
                y = c_B @ Binv
                y_stale = False
            d = y @ A - c
        sigma = np.where(free, np.where(d < 0.0, 1.0, -1.0), np.where(up, -1.0, 1.0))
        if steep:
            cand = ~basic & (np.where(free, -np.abs(d), sigma * d) < -eps)
            key = np.where(cand, -(d * d) / gamma, np.inf)
        else:
            key = np.where(~basic, np.where(free, -np.abs(d), sigma * d), np.inf)
            cand = key < -eps
            key = np.where(cand, key, np.inf)
        if not cand.any():
            status = INFEASIBLE if ph1 else OPTIMUM
            break
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
        # 3. ratio test: the textbook entries
        ub = u[b_ixs]
        lob = lo0[b_ixs]
        feas = w == 0.0 if ph1 else np.ones(m, dtype=bool)
        lo = feas & (ahat > piv_tol) & np.isfinite(lob)
        hi = feas & (ahat < -piv_tol) & np.isfinite(ub)
        t = np.full(m, np.inf)
        t[lo] = np.maximum(x_b[lo], 0.0) / ahat[lo]
        t[hi] = np.maximum(ub[hi] - x_b[hi], 0.0) / (-ahat[hi])
        bl = ab = np.zeros(m, dtype=bool)
        if ph1:
            bl = (w > 0.0) & (ahat < -piv_tol)  # rises to 0: leaves to its lower bound
            ab = (w < 0.0) & (ahat > piv_tol)   # falls to u_k: leaves to its upper bound
        if not lng:
            if ph1:
                t[bl] = x_b[bl] / ahat[bl]
                t[ab] = (x_b[ab] - ub[ab]) / ahat[ab]
                lo = lo | bl
                hi = hi | ab
            rows = lo | hi
            q = int(np.argmin(t)) if rows.any() else -1
            tq = t[q] if q >= 0 else np.inf
            side = bool(hi[q]) if q >= 0 else False
            if rows.sum() > 1:
                two = np.partition(t, 1)[:2]
                gap_ratio = min(gap_ratio, _rel_gap(two[0], two[1]))
            if q >= 0:
                tie("ratio", tied(t), ph1)
        else:
            # merged order of (t, 2 row + side, soft?, |ahat|)
            ent = []
            for i in np.flatnonzero(lo):
                ent.append((t[i], 2 * int(i), False, 0.0))
            for i in np.flatnonzero(hi):
                ent.append((t[i], 2 * int(i) + 1, False, 0.0))
            for i in np.flatnonzero(bl):
                ent.append((x_b[i] / ahat[i], 2 * int(i), True, abs(ahat[i])))
                if np.isfinite(ub[i]):
                    ent.append(((x_b[i] - ub[i]) / ahat[i], 2 * int(i) + 1, False, 0.0))
            for i in np.flatnonzero(ab):
                ent.append(((x_b[i] - ub[i]) / ahat[i], 2 * int(i) + 1, True, abs(ahat[i])))
                ent.append((x_b[i] / ahat[i], 2 * int(i), False, 0.0))
            ent.sort(key=lambda e: (e[0], e[1]))
            s0 = sp * d[p]
            slope = s0
            walked = abs(s0)
            leave = -1  # position in the merged order
            visited = []
            npass = 0
            last_soft = -1
            for k, e in enumerate(ent):
                if not e[2]:  # h
                    leave = k
                    break
                slope += e[3]
                walked += e[3]
                visited.append(e[1])
                gap_slope = min(gap_slope, abs(slope + eps) / walked)
                last_soft = k
                if slope >= -eps:
                    leave = k
                    break
                npass += 1
            if leave < 0 and last_soft >= 0:  # no hard entry: the last soft breakpoint leaves
                leave = last_soft
                npass -= 1
            if leave >= 0:
                tq, idx = ent[leave][0], ent[leave][1]
                q, side = idx >> 1, bool(idx & 1)
                for k in (leave - 1, leave + 1):
                    if 0 <= k < len(ent):
                        gap_walk = min(gap_walk, _rel_gap(tq, ent[k][0]))
                same = any(ent[k][0] == ent[k + 1][0] for k in range(min(leave + 1, len(ent) - 1)))
                ties["p1_walk"] += int(same)
            else:
                q, tq, side = -1, np.inf, False
            walks.append((visited, ent[leave][1] if leave >= 0 else -1))
            long_passed += npass
            long_passes += int(npass > 0)
            long_max = max(long_max, npass)
        u_p = u[p]
        if np.isfinite(u_p) and q >= 0:
            if u_p > 0.0:
                gap_flip = min(gap_flip, _rel_gap(u_p, tq))
            tie("flip", u_p == tq, ph1)
        p1_passes += int(ph1)
        # 4. flip: no weight changes
        if np.isfinite(u_p) and (q < 0 or u_p <= tq):
            x_b = x_b - u_p * ahat
            up[p] = not up[p]
            flips += 1
            fixed_flips += int(u_p == 0.0)
            integral = integral and whole(x_b)
            step_hist.append((ph1, u_p > 0.0))
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
        if steep:
            drift_enter = max(drift_enter, abs(gamma[p] - gp) / gp)
        theta = tq
        rho = Binv[q].copy()
        aq = alpha[q]
        x_b = x_b - theta * ahat
        x_b[q] = (u_p if up[p] else 0.0) + sp * theta
        step_hist.append((ph1, theta > 0.0))
        if ph1:
            y_stale = True
            p1_pivots += 1
        else:
            y = y - (d[p] / aq) * rho
        c_B[q] = c[p]
        leave_col = b_ixs[q]
        assert not free[leave_col]
        if steep:  # 7. the weights of the columns that were non-basic before the pivot, p excepted
            tau = alpha @ Binv
            nbv = ~basic
            nbv[p] = False
            g = (rho @ A) / aq
            new = np.maximum(gamma - 2.0 * g * (tau @ A) + g * g * gp, 1.0 + g * g)
            gamma = np.where(nbv, new, gamma)
            gamma[leave_col] = max(gp / (aq * aq), 1.0)
        basic[leave_col] = False
        up[leave_col] = side
        to_upper += int(side)
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
