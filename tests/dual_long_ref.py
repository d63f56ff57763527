"""Dense numpy restatement of the boxed dual simplex loop with the bound-flipping
(long-step) ratio test (include/simplex.h SPX_DUAL_RATIO_LONG_STEP; DESIGN.md
§7d).  Everything but step 2 is tests/dual_box_ref.py's pass, whose generator,
certificate and Farkas check are imported unchanged.

Step 2, with the candidates ahat_j = s sigma_j a_j < -piv_tol ordered by (key_j,
j), key_j = max(sigma_j d_j, 0) / -ahat_j, and slope = |delta_q|:
  walk the candidates; u_j = +inf: j enters; else slope' = slope - u_j (-ahat_j):
  slope' <= 0: j enters, otherwise j is flipped, slope = slope', go on.  No
  candidate, or all flipped: infeasible, nothing changed, no counter moved.
  (At slope' = 0 exactly the flips and j at its bound make row q feasible, so j
  must enter: flipping it and running out of candidates would call a feasible
  LP infeasible.  The slope therefore stays above 0 through a walk.)
Then with dx_j = +u_j for a flipped column at lower, -u_j at upper, v = sum (in
the walk's order) dx_j A_j: x_b -= B^-1 v, the flipped columns change side,
delta_q is taken again from the new x_b[q] with the same s, and the pivot is the
textbook one with the walk's d_p.  Flips are not pivots.

Besides DualBoxResult's fields the result carries the three flip counters and
two more gaps: `gap_walk`, the smallest relative key gap between consecutive
candidates of every walk (the entering column against the next candidate
included), and `gap_slope`, the smallest |slope'| / slope over every walk
decision.  Both say how far the walk is from depending on the fp64 summation
order.

`ties` counts the passes in which a decision met an exact tie: "row" and "ratio"
as in tests/dual_box_ref.py, "walk" (two consecutive candidates of the walk,
the entering column against the next one included, with equal keys) and
"slope0" (slope' == 0); `walk_run` is the longest run of equal keys among the
candidates one walk visited.
"""
from dataclasses import dataclass

import numpy as np

from dual_box_ref import (DANTZIG, NOT_DUAL_FEASIBLE, STEEPEST, DualBoxResult, boxed, certificate,  # noqa: F401
                          dual_simplex_box, farkas, tiny_box_infeasible)
from dual_ref import INFEASIBLE, MAX_ITER, OPTIMUM, tied, whole
from dual_se_ref import _rel_gap, row_norms2

TEXTBOOK, LONG_STEP = "textbook", "long"


@dataclass
class DualLongResult(DualBoxResult):
    flips: int = 0          # columns flipped
    flip_passes: int = 0    # passes with at least one flip
    max_flips: int = 0      # the largest flip count of one pass
    gap_walk: float = np.inf
    gap_slope: float = np.inf
    walk_run: int = 0       # the longest run of equal keys among the candidates one walk visited

    @property
    def counters(self):
        return (self.flips, self.flip_passes, self.max_flips)


def dual_simplex_long(A, b, c, u, rule=DANTZIG, ratio=LONG_STEP, basis=None, at_upper=None, eps=1e-7, feas_tol=1e-9,
                      piv_tol=1e-9, max_iter=1 << 62, trace_cap=200):
    """From the slack basis with every column at lower, or from `basis` and the
    placements `at_upper`.  ratio=TEXTBOOK stops every walk at its first
    candidate: tests/dual_box_ref.py's pass."""
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
                return DualLongResult(NOT_DUAL_FEASIBLE, np.nan, 0, b_ixs.copy(), x_basic(), up.copy(),
                                      bad_column=int(j))
            if not up[j]:
                up[j] = True
                placed += 1
        elif e[j] > eps and up[j]:
            up[j] = False
    x_b = x_basic()

    trace = []
    gap_row = gap_ratio = gap_walk = gap_slope = np.inf
    to_upper = flips = flip_passes = max_flips = walk_run = 0
    ties = {"row": 0, "ratio": 0, "walk": 0, "slope0": 0}
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
        # 2. pivot row and the walk
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
        cj = np.flatnonzero(cand)
        order = cj[np.lexsort((cj, key[cj]))]  # (key, column) ascending
        if len(order) > 1:
            gap_ratio = min(gap_ratio, _rel_gap(key[order[0]], key[order[1]]))
        ties["ratio"] += int(tied(key))
        slope = abs(delta[q])
        F = []
        p = -1
        gw, gs = np.inf, np.inf
        walk_tie = slope_tie = False
        run = 0
        for k, j in enumerate(order):
            j = int(j)
            run = run + 1 if k > 0 and key[j] == key[order[k - 1]] else 1
            walk_run = max(walk_run, run)
            if k + 1 < len(order) and ratio == LONG_STEP:  # (the entering column against the next one too)
                gw = min(gw, _rel_gap(key[j], key[order[k + 1]]))
                walk_tie = walk_tie or key[j] == key[order[k + 1]]
            if ratio == TEXTBOOK or not np.isfinite(u[j]):
                p = j
                break
            slope2 = slope - u[j] * (-ahat[j])
            gs = min(gs, abs(slope2) / slope)  # (slope > 0: it starts above feas_tol and a flip leaves it above 0)
            slope_tie = slope_tie or slope2 == 0.0
            if slope2 <= 0.0:
                p = j
                break
            F.append(j)
            slope = slope2
        if p < 0:  # every candidate flipped and none enters
            status = INFEASIBLE
            break
        gap_walk = min(gap_walk, gw)
        gap_slope = min(gap_slope, gs)
        ties["walk"] += int(walk_tie)
        ties["slope0"] += int(slope_tie)
        # 3. the flips
        if F:
            v = np.zeros(m)
            for j in F:  # the walk's order
                v = v + (-u[j] if up[j] else u[j]) * A[:, j]
            x_b = x_b - Binv @ v
            for j in F:
                up[j] = not up[j]
            flips += len(F)
            flip_passes += 1
            max_flips = max(max_flips, len(F))
        dq = x_b[q] if s > 0.0 else x_b[q] - ub[q]
        # 4. FTRAN and update
        alpha = Binv @ A[:, p]
        aq = alpha[q]
        theta = dq / aq
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
    return DualLongResult(status, z + zu, it, b_ixs.copy(), x_b.copy(), up.copy(), trace, float(gap_row),
                          float(gap_ratio), to_upper, placed, y=y.copy(), Binv=Binv.copy(), ties=ties,
                          integral=integral, flips=flips, flip_passes=flip_passes, max_flips=max_flips,
                          gap_walk=float(gap_walk), gap_slope=float(gap_slope), walk_run=walk_run)
