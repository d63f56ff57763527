"""Dense numpy restatement of bound ranging at the optimum and of the objective at
the range ends (include/simplex.h spx_ranging_bound / spx_ranging_objective;
DESIGN.md §7n), in the conventions of tests/ranging_ref.py: maximise c.x, A =
[structural | I], the shifted variables x' = x - l with ranges ub = u - l, x_i the
basic values clamped into [0, ub_B[i]], tol the pivot tolerance.  Every result
is a non-negative delta, +inf where nothing blocks, with what blocks: 2 row +
side of the row that leaves (side 1: to its upper bound), -1 nothing, OWN (-2)
the column's own other bound.

Non-basic column j, not free, at lower or at upper alike: the bound it sits at
moves by t and the column with it, x_B(t) = x_B - t alpha, alpha = B^-1 A_j.
  up   (t > 0): alpha_i > tol blocks at x_i / alpha_i (side 0); alpha_i < -tol with
       ub_B[i] finite at (ub_B[i] - x_i) / -alpha_i (side 1)
  down (t < 0): alpha_i < -tol blocks at x_i / -alpha_i (side 0); alpha_i > tol with
       ub_B[i] finite at (ub_B[i] - x_i) / alpha_i (side 1)
A row whose basic column is free never blocks.  Key (ratio, 2 i + side).  Then the
own other bound: at lower "up" is capped by ub_j, at upper "down" is, blocker OWN,
only where strictly smaller than every row's ratio (a fixed column, ub_j = 0, by
the same rule).  Non-basic and free: both +inf, -1.  Basic in row i: up = x_i (2
i; a free column +inf, -1), down = ub_B[i] - x_i (2 i + 1; +inf, -1 without an upper
bound).

Everything is a function of the basis, the placements and the vectors handed in;
the arithmetic runs in `dtype`.
"""
from dataclasses import dataclass

import numpy as np

import ranging_ref as rr

OWN = -2  # SPX_RANGING_OWN_BOUND


@dataclass
class BoundRef:
    down: np.ndarray         # n
    up: np.ndarray
    leave_down: np.ndarray   # n int64: 2 row + side, -1 none, OWN
    leave_up: np.ndarray
    second_down: np.ndarray  # n: the runner-up among the rows' ratios and the own bound (+inf: none; basic: +inf)
    second_up: np.ndarray
    nb: np.ndarray           # the non-basic columns, ascending
    T: np.ndarray            # m x len(nb): B^-1 A_N
    row_of: np.ndarray       # n: the row a column is basic in, -1 non-basic
    kind: np.ndarray         # n: 0 at lower, 1 at upper, 2 free, -1 basic
    x: np.ndarray            # m: x_b clamped


def bound_ranging(A, b_ixs, at_upper, Binv, x_b, rng, free=None, tol=1e-9, dtype=np.float64):
    A = np.asarray(A, dtype=dtype)
    Binv = np.asarray(Binv, dtype=dtype)
    m, n = A.shape
    b_ixs = np.asarray(b_ixs, dtype=np.int64)
    rng = np.asarray(rng, dtype=dtype)
    row_of = np.full(n, -1, dtype=np.int64)
    row_of[b_ixs] = np.arange(m)
    basic = row_of >= 0
    fr = np.zeros(n, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    upb = np.asarray(at_upper, dtype=bool) & ~basic & ~fr
    kind = np.where(basic, -1, np.where(fr, 2, np.where(upb, 1, 0))).astype(np.int64)
    ub = rng[b_ixs]
    x = np.minimum(np.maximum(np.asarray(x_b, dtype=dtype), 0.0), ub)
    frB = fr[b_ixs]
    inf = np.array(np.inf, dtype=dtype)
    down = np.full(n, inf, dtype=dtype)
    up = np.full(n, inf, dtype=dtype)
    kd = np.full(n, -1, dtype=np.int64)
    ku = np.full(n, -1, dtype=np.int64)
    sd = np.full(n, inf, dtype=dtype)
    su = np.full(n, inf, dtype=dtype)
    nb = np.flatnonzero(~basic)
    T = Binv @ A[:, nb]
    a = np.abs(T)
    big = (a > tol) & ~frB[:, None]
    den = np.where(big, a, 1.0)
    lo = np.where(big, x[:, None] / den, inf)                       # side 0
    fin = np.isfinite(ub)[:, None]
    room = np.where(np.isfinite(ub), ub - x, 0.0)
    hi = np.where(big & fin, room[:, None] / den, inf)              # side 1
    pos_a, neg_a = T > 0, T < 0
    cnt = len(nb)
    Rdn = np.full((2 * m, cnt), inf, dtype=dtype)                   # keyed by 2 i + side: rows interleaved
    Rup = np.full((2 * m, cnt), inf, dtype=dtype)
    Rup[0::2] = np.where(pos_a, lo, inf)
    Rup[1::2] = np.where(neg_a, hi, inf)
    Rdn[0::2] = np.where(neg_a, lo, inf)
    Rdn[1::2] = np.where(pos_a, hi, inf)
    for R, out, k, sec, capped in ((Rdn, down, kd, sd, 1), (Rup, up, ku, su, 0)):
        best, pos, second = rr._min2(np.ascontiguousarray(R.T))
        own = np.where(kind[nb] == capped, rng[nb], inf)
        wins = own < best  # strictly: on a tie the row is reported
        second = np.where(wins, best, np.minimum(second, own))
        pos = np.where(wins, OWN, pos)
        best = np.where(wins, own, best)
        isfr = kind[nb] == 2
        out[nb] = np.where(isfr, inf, best)
        k[nb] = np.where(isfr, -1, pos)
        sec[nb] = np.where(isfr, inf, second)
    rows = np.arange(m)
    up[b_ixs] = np.where(frB, inf, x)
    ku[b_ixs] = np.where(frB, -1, 2 * rows)
    finB = np.isfinite(ub)
    down[b_ixs] = np.where(finB, room, inf)
    kd[b_ixs] = np.where(finB, 2 * rows + 1, -1)
    return BoundRef(down, up, kd, ku, sd, su, nb, T, row_of, kind, x)


def refuse_case(ref, tol=1e-9):
    """Why the comparison of a kernel against this restatement would depend on
    rounding (a list of reasons, empty: the case stands): an entry of T within
    [tol / 2, 2 tol] in magnitude, or more than ranging_ref.SHARE of the non-basic
    columns under the runner-up exemption."""
    why = []
    a = np.abs(np.asarray(ref.T, dtype=np.float64))
    k = int(np.sum((a >= tol / 2) & (a <= 2 * tol)))
    if k:
        why.append(f"{k} entries of T within [tol / 2, 2 tol]")
    ex = exempt_columns(ref)
    if len(ex) > rr.SHARE * len(ref.nb):
        why.append(f"{len(ex)} of {len(ref.nb)} non-basic columns under the runner-up exemption")
    return why


def exempt_columns(ref):
    nb = ref.nb
    return nb[rr.exempt(ref.down[nb], ref.second_down[nb]) | rr.exempt(ref.up[nb], ref.second_up[nb])]


def objective_ends(what, z, down, up, mult, moves=None, dtype=np.float64):
    """(obj_down, obj_up).  what "cost": mult = x in the caller's variables, z -+
    delta x_j; "rhs": mult = y; "bound": mult = d = y.A - c, obj_up = z - up d_j and
    obj_down = z + down d_j where `moves` (non-basic and not free), z elsewhere.
    A multiplier that is exactly 0 gives z even where the delta is +inf."""
    z = dtype(z)
    down = np.asarray(down, dtype=dtype)
    up = np.asarray(up, dtype=dtype)
    mult = np.asarray(mult, dtype=dtype)
    sdn, sup = (1.0, -1.0) if what == "bound" else (-1.0, 1.0)
    zero = mult == 0.0
    if moves is not None:
        zero = zero | ~np.asarray(moves, dtype=bool)
    with np.errstate(invalid="ignore"):
        od = np.where(zero, z, z + sdn * down * np.where(zero, 1.0, mult))
        ou = np.where(zero, z, z + sup * up * np.where(zero, 1.0, mult))
    return od, ou


def tie_rows():
    """max x0 + x1, x0 + x2 + s0 = 4, x1 + x2 + s1 = 4, x2 non-basic at 0 with
    alpha = (1, 1) against x_B = (4, 4): the two rows tie exactly at 4 for "up",
    and the smaller key, row 0 side 0, is reported.  Returns (A, b, c, u, basis)."""
    A = np.array([[1.0, 0.0, 1.0, 1.0, 0.0], [0.0, 1.0, 1.0, 0.0, 1.0]])
    return A, np.array([4.0, 4.0]), np.array([1.0, 1.0, 1.0, 0.0, 0.0]), np.full(5, np.inf), [0, 1]


def tie_rows_far(m=6, tie=(1, 4)):
    """m rows x_i + a_i x_m + s_i = 4 with a_i = 1 in the two rows of `tie` and 1 / 2
    elsewhere, max sum x: x_0 .. x_{m-1} basic at 4, x_m non-basic at 0 (d_m = sum a -
    1 > 0).  "up" of column m ties exactly at 4 in the two rows (8 elsewhere) and
    the smaller row is reported: rows 1 and 4 sit in different lanes of the
    accumulator layout, in the order that a merge keeping its own on a tie gets
    wrong.  Returns (A, b, c, u, basis)."""
    a = np.full(m, 0.5)
    a[list(tie)] = 1.0
    A = np.hstack([np.eye(m), a[:, None], np.eye(m)])
    return A, np.full(m, 4.0), np.concatenate([np.ones(m + 1), np.zeros(m)]), np.full(2 * m + 1, np.inf), list(range(m))


def tie_own():
    """tie_rows with u_2 = 4: the own bound ties the two rows exactly, and the
    row is reported; with u_2 = 3 the own bound wins."""
    A, b, c, u, basis = tie_rows()
    u = u.copy()
    u[2] = 4.0
    return A, b, c, u, basis
