"""Dense numpy restatement of sensitivity ranging at the optimum (include/simplex.h
spx_ranging_cost / spx_ranging_rhs), in the bounded loops' own
conventions (primal_box_ref.py): maximise c.x, A x = b with A = [structural | I],
d = y.A - c, sigma_k = +1 for a non-basic column at its lower bound and -1 at its
upper bound, optimal means sigma_k d_k >= 0.  With tol the pivot tolerance and
s_k = max(sigma_k d_k, 0) every result is a non-negative delta, +inf where
nothing blocks, and the index of what blocks (-1: nothing).

Cost ranging, per column j.  Non-basic at lower: up = s_j, down = +inf; at upper:
down = s_j, up = +inf; free: both 0; the blocking column is j itself.  Basic in
row i: T_ik = rho_i.A_k (rho_i row i of B^-1, k non-basic), g_k = sigma_k T_ik;
up = min s_k / -g_k over g_k < -tol, down = min s_k / g_k over g_k > tol; a free
non-basic k with |T_ik| > tol blocks both at 0.  Ties: the smallest column k.

Right-hand-side ranging, per row r.  beta = column r of B^-1, x_i the basic values
clamped into [0, ub_B[i]].  beta_i > tol blocks down at x_i / beta_i and, ub_B[i]
finite, up at (ub_B[i] - x_i) / beta_i; beta_i < -tol blocks up at x_i / -beta_i
and, ub_B[i] finite, down at (ub_B[i] - x_i) / -beta_i; a row whose basic column
is free never blocks.  Key (ratio, 2 i + side), side 1 = leaves to its upper bound.

Everything is a function of the basis, the placements and the vectors handed in;
the arithmetic runs in `dtype` (the GPU tests pass np.longdouble and the device's
own B^-1, y and x_b).  Beside the answer the results carry what a comparison
needs: the runner-up ratios, and T, d, sigma, s over the non-basic columns.
"""
from dataclasses import dataclass

import numpy as np


@dataclass
class CostRef:
    down: np.ndarray        # n
    up: np.ndarray
    block_down: np.ndarray  # n int64, -1 none
    block_up: np.ndarray
    second_down: np.ndarray  # n: the runner-up ratio of a basic column's row (+inf: none; non-basic: +inf)
    second_up: np.ndarray
    nb: np.ndarray          # the non-basic columns, ascending
    T: np.ndarray           # m x len(nb): B^-1 A_N
    d: np.ndarray           # n: y.A - c
    sigma: np.ndarray       # n: +1 / -1 / 0 (free); basic columns 0
    s: np.ndarray           # n: max(sigma d, 0); free and basic columns 0
    row_of: np.ndarray      # n: the row a column is basic in, -1 non-basic


@dataclass
class RhsRef:
    down: np.ndarray        # m
    up: np.ndarray
    leave_down: np.ndarray  # m int64: 2 row + side, -1 none
    leave_up: np.ndarray
    second_down: np.ndarray
    second_up: np.ndarray
    x: np.ndarray           # m: x_b clamped


def _min2(R):
    """Per row of R (+inf = no candidate): the minimum, its first position (-1:
    none) and the second-smallest value."""
    rows, cols = R.shape
    if cols == 0:
        inf = np.full(rows, np.inf, dtype=R.dtype)
        return inf, np.full(rows, -1, dtype=np.int64), inf.copy()
    pos = np.argmin(R, axis=1)  # the first on ties
    best = R[np.arange(rows), pos]
    if cols > 1:
        R2 = R.copy()
        R2[np.arange(rows), pos] = np.inf
        second = R2.min(axis=1)
    else:
        second = np.full(rows, np.inf, dtype=R.dtype)
    pos = np.where(np.isfinite(best), pos, -1).astype(np.int64)
    return best, pos, second


def cost_ranging(A, c, b_ixs, at_upper, Binv, y, free=None, tol=1e-9, dtype=np.float64):
    A = np.asarray(A, dtype=dtype)
    c = np.asarray(c, dtype=dtype)
    Binv = np.asarray(Binv, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    m, n = A.shape
    b_ixs = np.asarray(b_ixs, dtype=np.int64)
    row_of = np.full(n, -1, dtype=np.int64)
    row_of[b_ixs] = np.arange(m)
    basic = row_of >= 0
    fr = np.zeros(n, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    upb = np.asarray(at_upper, dtype=bool) & ~basic & ~fr
    d = y @ A - c
    sigma = np.where(basic | fr, 0.0, np.where(upb, -1.0, 1.0)).astype(dtype)
    s = np.where(basic | fr, 0.0, np.maximum(sigma * d, 0.0)).astype(dtype)
    inf = np.array(np.inf, dtype=dtype)
    down = np.full(n, inf, dtype=dtype)
    up = np.full(n, inf, dtype=dtype)
    kd = np.full(n, -1, dtype=np.int64)
    ku = np.full(n, -1, dtype=np.int64)
    sd = np.full(n, inf, dtype=dtype)
    su = np.full(n, inf, dtype=dtype)
    nb = np.flatnonzero(~basic)  # ascending: the first minimum is the smallest column
    for j in nb:
        if fr[j]:
            down[j] = up[j] = 0.0
            kd[j] = ku[j] = j
        elif upb[j]:
            down[j] = s[j]
            kd[j] = j
        else:
            up[j] = s[j]
            ku[j] = j
    T = Binv @ A[:, nb]
    frn = fr[nb]
    g = np.where(frn, T, sigma[nb] * T)
    big = np.abs(g) > tol
    ratio = np.where(big, s[nb] / np.where(big, np.abs(g), 1.0), inf)
    Rup = np.where(big & (frn | (g < 0)), ratio, inf)
    Rdn = np.where(big & (frn | (g > 0)), ratio, inf)
    for R, out, k, sec in ((Rdn, down, kd, sd), (Rup, up, ku, su)):
        best, pos, second = _min2(R)
        out[b_ixs] = best
        k[b_ixs] = np.where(pos >= 0, nb[np.maximum(pos, 0)] if len(nb) else -1, -1)
        sec[b_ixs] = second
    return CostRef(down, up, kd, ku, sd, su, nb, T, d, sigma, s, row_of)


def rhs_ranging(Binv, x_b, ub_B, free_B=None, tol=1e-9, dtype=np.float64):
    Binv = np.asarray(Binv, dtype=dtype)
    m = Binv.shape[0]
    ub = np.asarray(ub_B, dtype=dtype)
    x = np.minimum(np.maximum(np.asarray(x_b, dtype=dtype), 0.0), ub)
    frB = np.zeros(m, dtype=bool) if free_B is None else np.asarray(free_B, dtype=bool)
    inf = np.array(np.inf, dtype=dtype)
    beta = Binv  # beta[i, r]
    a = np.abs(beta)
    big = (a > tol) & ~frB[:, None]
    den = np.where(big, a, 1.0)
    lo = np.where(big, x[:, None] / den, inf)                       # side 0
    fin = np.isfinite(ub)[:, None]
    room = np.where(np.isfinite(ub), ub - x, 0.0)
    hi = np.where(big & fin, room[:, None] / den, inf)              # side 1
    pos_b, neg_b = beta > 0, beta < 0
    # keyed by 2 i + side: rows interleaved
    Rdn = np.full((2 * m, m), inf, dtype=dtype)
    Rup = np.full((2 * m, m), inf, dtype=dtype)
    Rdn[0::2] = np.where(pos_b, lo, inf)
    Rdn[1::2] = np.where(neg_b, hi, inf)
    Rup[0::2] = np.where(neg_b, lo, inf)
    Rup[1::2] = np.where(pos_b, hi, inf)
    dn, kdn, sdn = _min2(np.ascontiguousarray(Rdn.T))
    up, kup, sup = _min2(np.ascontiguousarray(Rup.T))
    return RhsRef(dn, up, kdn, kup, sdn, sup, x)


GAP = 1e-6     # an index is compared only where the runner-up is at least (1 + GAP) x the minimum
SHARE = 0.05   # a case with more rows or columns than this under that exemption is refused


def exempt(best, second, gap=GAP):
    """Where the runner-up is less than (1 + gap) x the minimum, so that the
    index may depend on rounding.  (A tie at 0 is not exempt: 0 / |g| is 0 on
    both sides, and the index rule decides.)"""
    best = np.asarray(best, dtype=np.float64)
    second = np.asarray(second, dtype=np.float64)
    return np.isfinite(best) & np.isfinite(second) & (second < (1.0 + gap) * best)


def refuse_case(cost, rhs, Binv, tol=1e-9):
    """Why the comparison of a kernel against this restatement would depend on
    rounding (a list of reasons, empty: the case stands): an entry of T or of
    B^-1 within [tol / 2, 2 tol] in magnitude (the candidate sets could differ),
    or more than SHARE of the basic columns (cost) or rows (right-hand side)
    under the runner-up exemption."""
    why = []
    m = Binv.shape[0]
    for name, M in (("T", cost.T), ("B^-1", Binv)):
        a = np.abs(np.asarray(M, dtype=np.float64))
        k = int(np.sum((a >= tol / 2) & (a <= 2 * tol)))
        if k:
            why.append(f"{k} entries of {name} within [tol / 2, 2 tol]")
    ex_c = int(np.sum(exempt(cost.down, cost.second_down) | exempt(cost.up, cost.second_up)))
    ex_r = int(np.sum(exempt(rhs.down, rhs.second_down) | exempt(rhs.up, rhs.second_up)))
    if ex_c > SHARE * m:
        why.append(f"{ex_c} of {m} basic columns under the runner-up exemption")
    if ex_r > SHARE * m:
        why.append(f"{ex_r} of {m} rows under the runner-up exemption")
    return why


# the GPU tests' cases: (generator, m, n, seed); "primal" = primal_box_ref.boxed_primal under SPX_ALGO_PRIMAL_BOX,
# "dual" = dual_box_ref.boxed under SPX_ALGO_DUAL, "lu" = primal_lu_ref.general_lu (free and lower-shifted columns)
# under SPX_ALGO_PRIMAL_BOX with phase 1.  tests/test_ranging_cpu.py checks every one against refuse_case.
CASES = [("primal", 7, 20, 0), ("primal", 65, 200, 1), ("primal", 130, 390, 2), ("primal", 256, 1024, 3),
         ("dual", 7, 20, 0), ("dual", 65, 200, 1), ("dual", 130, 390, 2), ("dual", 256, 1024, 3),
         ("lu", 65, 200, 1), ("lu", 130, 390, 2)]


def build_lp(kind, m, n, seed):
    """(A, b, c, l, u): l is None for the two generators without lower bounds."""
    import dual_box_ref
    import primal_box_ref
    import primal_lu_ref
    if kind == "primal":
        A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
        return A, b, c, None, u
    if kind == "dual":
        A, b, c, u = dual_box_ref.boxed(m, n, seed)
        return A, b, c, None, u
    assert kind == "lu"
    return primal_lu_ref.general_lu(m, n, seed)


def solve_numpy(kind, A, b, c, l, u):
    """The numpy loop's optimum as ranging's input: (b_ixs, at_upper, Binv, y,
    x_b of the shifted problem, ranges, free)."""
    import dual_box_ref
    import primal_box_ref
    import primal_lu_ref
    n = A.shape[1]
    if kind == "primal":
        r = primal_box_ref.primal_simplex_box(A, b, c, u)
        xs, rng, fr = r.x_b, u, np.zeros(n, dtype=bool)
    elif kind == "dual":
        r = dual_box_ref.dual_simplex_box(A, b, c, u)
        xs, rng, fr = r.x_b, u, np.zeros(n, dtype=bool)
    else:
        r = primal_lu_ref.primal_simplex_lu(A, b, c, l, u)
        fr = np.isneginf(l)
        rng = np.where(np.isfinite(u), u - np.where(fr, 0.0, l), np.inf)
        xs = r.x_shifted
    assert r.status == "optimum", r.status
    return r.b_ixs, r.at_upper, r.Binv, r.y, xs, rng, fr


def both(A, c, b_ixs, at_upper, Binv, y, x_b, rng, free, tol=1e-9, dtype=np.float64):
    """(CostRef, RhsRef) of one optimum."""
    b_ixs = np.asarray(b_ixs, dtype=np.int64)
    cost = cost_ranging(A, c, b_ixs, at_upper, Binv, y, free=free, tol=tol, dtype=dtype)
    rhs = rhs_ranging(Binv, x_b, np.asarray(rng)[b_ixs], free_B=np.asarray(free, dtype=bool)[b_ixs], tol=tol,
                      dtype=dtype)
    return cost, rhs


def tiny_free():
    """tiny_tie with a free column 3 = (1, 1), cost 3, ahead of the slacks: at the
    optimum (x0 and s1 basic, y = (3, 0)) its reduced cost is exactly 0, so it
    stays non-basic at 0 with T = (1, 1): it blocks the cost of both basic
    columns in both directions at 0.  Returns (A, b, c, l, u, basis)."""
    A = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 0.0], [0.0, 1.0, 1.0, 1.0, 0.0, 1.0]])
    l = np.zeros(6)
    l[3] = -np.inf
    return A, np.array([4.0, 5.0]), np.array([3.0, 1.0, 1.0, 3.0, 0.0, 0.0]), l, np.full(6, np.inf), [0, 5]


def tiny_tie():
    """max 3 x0 + x1 + x2, x0 + x1 + x2 + s0 = 4, x1 + x2 + s1 = 5.  The optimum
    has x0 and s1 basic; columns 1 and 2 are identical, so in both rows their
    ratios tie exactly (2 = 2): the smaller column, 1, is reported.  Returns
    (A, b, c, u, basis)."""
    A = np.array([[1.0, 1.0, 1.0, 1.0, 0.0], [0.0, 1.0, 1.0, 0.0, 1.0]])
    return A, np.array([4.0, 5.0]), np.array([3.0, 1.0, 1.0, 0.0, 0.0]), np.full(5, np.inf), [0, 4]
