"""Seeded LPs on which every number a simplex pass computes is a small integer,
so that exact ties abound and still every implementation must agree bit for
bit: the generators of tests/golden/tied_optima.json (tests/test_tied_cpu.py,
tests/test_gpu_tied.py).

A = [+-U | I] with U an interval matrix: every column is one run of consecutive
ones.  Such a matrix is totally unimodular, and so is [+-U | I] with some rows
negated.  With integer b, c and u every basis has determinant +-1, B^-1 has
entries in {0, +-1}, every pivot element is +-1, and x_b, y, d_j, every ratio
key and every slope are integers far below 2^53; the steepest-edge weights are
integer row norms and the key -(delta^2) / w is one fp64 division of two exact
integers, so equal rationals round equal.  Neither the fma order, the order of
a reduction, the grid size nor a reinversion (pivoting preserves total
unimodularity) can change one bit: the first-index tie rules of
include/simplex.h are the only thing left that decides a pass.

Layout as in the other *_ref.py files: A is m x n with the slack identity in
its last m columns, maximise c.x, 0 <= x <= u (u has n entries, +inf = none);
tied_lu has general bounds l <= x <= u (l_j = -inf and u_j = +inf: free).
All values are float64 integers.
"""
import numpy as np

import dual_box_ref
import dual_long_ref
import dual_ref
import dual_se_ref
import primal_box_ref
import primal_lu_ref
import primal_phase1_ref

# the traced shapes of dual_ref.SHAPES
SHAPES = [(7, 20), (65, 200), (130, 390), (256, 1024)]
# loop variant -> the tie counters (the references' `ties`) that apply to it
VARIANTS = {
    "dual_dantzig": ("row", "ratio"),
    "dual_steepest": ("row", "ratio"),
    "box_dantzig": ("row", "ratio"),
    "box_steepest": ("row", "ratio"),
    "long_dantzig": ("row", "ratio", "walk", "slope0"),
    "long_steepest": ("row", "ratio", "walk", "slope0"),
    "pbox": ("price", "ratio", "flip"),
    "phase1": ("price", "ratio", "flip", "p1_price", "p1_ratio", "p1_flip"),
    "phase1_infeasible": ("p1_price", "p1_ratio", "p1_flip"),
    "free": ("price", "ratio", "flip", "free_price"),
    "free_unbounded": ("price", "free_price"),
}
# the general-bounds variants (l <= x <= u: case_lp returns (A, b, c, l, u)); free_unbounded has one case only
LU_VARIANTS = ("free", "free_unbounded")
UNBOUNDED_SHAPES = [(65, 200)]


def shapes(variant):
    """The shapes at which the golden file holds a case of the variant."""
    return UNBOUNDED_SHAPES if variant == "free_unbounded" else SHAPES


def case_lp(variant, m, n, seed, mixed=False):
    """(A, b, c, u) of one golden case; (A, b, c, l, u) for the LU_VARIANTS."""
    if variant in LU_VARIANTS:
        return tied_lu(m, n, seed, disjoint=variant == "free")
    if variant.startswith("dual_"):
        return tied_covering(m, n, seed, False)
    if variant.startswith(("box_", "long_")):
        return tied_covering(m, n, seed, True, mixed)
    if variant == "pbox":
        return tied_primal(m, n, seed)
    return tied_general(m, n, seed, infeasible=variant == "phase1_infeasible")


def case_ref(variant, lp, **kw):
    """The numpy reference of the variant's loop on (A, b, c, u)."""
    if variant in LU_VARIANTS:
        return primal_lu_ref.primal_simplex_lu(*lp, **kw)
    A, b, c, u = lp
    rule = dual_box_ref.STEEPEST if variant.endswith("steepest") else dual_box_ref.DANTZIG
    if variant == "dual_dantzig":
        return dual_ref.dual_simplex(A, b, c, **kw)
    if variant == "dual_steepest":
        return dual_se_ref.dual_simplex_se(A, b, c, **kw)
    if variant.startswith("box_"):
        return dual_box_ref.dual_simplex_box(A, b, c, u, rule=rule, **kw)
    if variant.startswith("long_"):
        return dual_long_ref.dual_simplex_long(A, b, c, u, rule=rule, **kw)
    if variant == "pbox":
        return primal_box_ref.primal_simplex_box(A, b, c, u, **kw)
    return primal_phase1_ref.primal_simplex_phase1(A, b, c, u, **kw)


def interval(m, ns, rng):
    """m x ns: column j has ones on rows a .. min(m, a + l) - 1, a ~ U{0..m-1},
    l ~ U{1..max(2, m // 4)}."""
    U = np.zeros((m, ns))
    a = rng.integers(0, m, ns)
    ln = rng.integers(1, max(2, m // 4) + 1, ns)
    for j in range(ns):
        U[a[j]:min(m, a[j] + ln[j]), j] = 1.0
    return U


def tied_covering(m, n, seed, boxed, mixed=False):
    """min cost.x, U x >= h, 0 <= x <= u for the dual loops: A = [-U | I], b =
    -h, c = -cost with cost_j in {1, 2, 3}.  u_j in {1, 2} on the structural
    columns (all +inf when `boxed` is false), slacks +inf.  h = max(U x0 - r, 0)
    with integer 0 <= x0 <= u (0..2 without bounds) and r in {0, 1}: feasible by
    construction, and zeros in b.  `mixed` (boxed only) flips the sign of about
    20 % of the structural c_j: those columns are dual feasible only at their
    upper bound, where the entry normalisation puts them.  Returns (A, b, c, u)."""
    ns = n - m
    r = np.random.default_rng(seed + 6000)
    U = interval(m, ns, r)
    us = r.integers(1, 3, ns).astype(np.float64)
    x0 = np.floor(r.uniform(0, 1, ns) * (us + 1.0)) if boxed else r.integers(0, 3, ns).astype(np.float64)
    slack = r.integers(0, 2, m).astype(np.float64)
    cost = r.integers(1, 4, ns).astype(np.float64)
    flip = r.uniform(0, 1, ns) < 0.2
    A = np.hstack([-U, np.eye(m)])
    b = -np.maximum(U @ x0 - slack, 0.0)
    c = np.concatenate([-cost, np.zeros(m)])
    u = np.full(n, np.inf)
    if boxed:
        u[:ns] = us
        if mixed:
            c[:ns] = np.where(flip, -c[:ns], c[:ns])
    return A, b, c, u


def tied_primal(m, n, seed):
    """max c.x, U x <= b, 0 <= x <= u for the bounded primal loop: A = [U | I],
    b in {0..5} (zeros: a degenerate slack basis), c_j in {1, 2, 3}, u_j in {1,
    2} with probability 0.6 and +inf otherwise, slacks +inf."""
    ns = n - m
    r = np.random.default_rng(seed + 7000)
    U = interval(m, ns, r)
    b = r.integers(0, 6, m).astype(np.float64)
    c = np.concatenate([r.integers(1, 4, ns).astype(np.float64), np.zeros(m)])
    us = r.integers(1, 3, ns).astype(np.float64)
    us[r.uniform(0, 1, ns) >= 0.6] = np.inf
    u = np.concatenate([us, np.full(m, np.inf)])
    return np.hstack([U, np.eye(m)]), b, c, u


def tied_general(m, n, seed, infeasible=False):
    """tied_primal's A, c and u with about 30 % of the rows negated into >= rows
    (-U_i x + s_i = b_i <= 0), whose slack starts below 0: phase 1 has work to
    do.  b comes from an integer x0 within the bounds (0..2 where there is
    none): U_i x0 + r_i on a <= row, -max(U_i x0 - r_i, 0) on a >= row, r in {0,
    1}, so the LP is feasible.  `infeasible` takes 40 off the >= rows' b."""
    ns = n - m
    A, _, c, u = tied_primal(m, n, seed)
    r = np.random.default_rng(seed + 8000)
    ge = r.uniform(0, 1, m) < 0.3
    fin = np.isfinite(u[:ns])
    x0 = np.floor(r.uniform(0, 1, ns) * (np.where(fin, u[:ns], 2.0) + 1.0))
    slack = r.integers(0, 2, m).astype(np.float64)
    ax = A[:, :ns] @ x0
    A = A.copy()
    A[ge, :ns] *= -1.0
    b = np.where(ge, -np.maximum(ax - slack, 0.0), ax + slack)
    if infeasible:
        b = np.where(ge, b - 40.0, b)
    return A, b, c, u


def tied_lu(m, n, seed, disjoint=True):
    """tied_general with general integer bounds l <= x <= u, returned as (A, b,
    c, l, u).  Structural column j: j % 5 == 2 is free with a cost in {-3..3};
    else j % 11 == 3 is fixed at an integer in {-2..2}; else it has a finite
    integer range (tied_general's u_j, or 1..3 where that is +inf) and, with
    probability 1/3, a lower bound in {-2..2} that its range sits on.  Every
    slack gets an upper bound in {1..4}: all rows are ranged.  With `disjoint`
    the free columns' runs of rows are replaced by pairwise disjoint runs (1..4
    rows each, in the rows' own signs): a free column then cannot cancel
    against another column along its run, and with every other column and every
    row bounded the LP is bounded.  Without it the free columns keep
    tied_general's overlapping runs and the LP is almost always unbounded.  A
    is still an interval matrix with rows negated next to the identity, so
    totally unimodular.  b = A x0 for an integer x0 within the bounds (a free
    column's x0 in {-2..2}, the slacks' within theirs): feasible, and all of b,
    c, l, u are integers."""
    ns = n - m
    A, _, c, u = tied_general(m, n, seed)
    r = np.random.default_rng(seed + 8500)
    A = A.copy()
    c = c.copy()
    u = u.copy()
    j = np.arange(ns)
    is_free = j % 5 == 2
    is_fixed = ~is_free & (j % 11 == 3)
    rng_ = np.where(np.isfinite(u[:ns]), u[:ns], r.integers(1, 4, ns).astype(np.float64))
    lo = r.integers(-2, 3, ns).astype(np.float64)
    has_lo = r.uniform(0, 1, ns) < 1.0 / 3.0
    fx = r.integers(-2, 3, ns).astype(np.float64)
    cf = r.integers(-3, 4, ns).astype(np.float64)
    su = r.integers(1, 5, m).astype(np.float64)
    nf = int(is_free.sum())
    start = np.sort(r.choice(m, size=nf, replace=False))
    ln = r.integers(1, 5, nf)
    order = r.permutation(nf)
    xf = r.integers(-2, 3, ns).astype(np.float64)
    frac = r.uniform(0, 1, n)
    l = np.zeros(n)
    l[:ns] = np.where(is_fixed, fx, np.where(has_lo, lo, 0.0))
    u[:ns] = np.where(is_fixed, fx, l[:ns] + rng_)
    x0 = np.empty(n)
    x0[:ns] = np.where(is_free, xf, l[:ns] + np.floor(frac[:ns] * (u[:ns] - l[:ns] + 1.0)))
    x0[ns:] = np.floor(frac[ns:] * (su + 1.0))
    l[:ns][is_free] = -np.inf
    u[:ns][is_free] = np.inf
    u[ns:] = su
    c[:ns][is_free] = cf[is_free]
    if disjoint:
        sign = A[:, :ns].sum(axis=1)  # a >= row's entries are -1
        sign = np.where(sign < 0, -1.0, 1.0)
        end = np.minimum(np.append(start[1:], m), start + ln)
        for k, col in enumerate(np.flatnonzero(is_free)):
            a, e = start[order[k]], end[order[k]]
            A[:, col] = 0.0
            A[a:e, col] = sign[a:e]
    return A, A @ x0, c, l, u


def exact_capacity():
    """min x1 + 2 x2, x1 + x2 >= 3, x1 <= 1, x2 <= 2.  The long-step walk meets
    slope 3 -> 2 -> 0: at slope' = 0 exactly x2 enters at its bound after x1
    is flipped.  Optimum x = (1, 2), z = -5, one flip, one pivot."""
    A = np.array([[-1.0, -1.0, 1.0]])
    return A, np.array([-3.0]), np.array([-1.0, -2.0, 0.0]), np.array([1.0, 2.0, np.inf])


def short_capacity():
    """exact_capacity with x1 + x2 >= 4: infeasible (both candidates are flipped
    and the slope is still 1)."""
    A, _, c, u = exact_capacity()
    return A, np.array([-4.0]), c, u


def flip_tie():
    """max 2 x0 + x1, x0 + x1 + s = 3, x0 <= 3, x1 <= 1 for the bounded primal
    loop.  Pass 1: x0 enters, the slack's ratio is t_q = 3 = u_0 exactly: the
    rule u_p <= t_q flips (x0 to its bound, s = 0).  Pass 2: x1 enters and the
    slack leaves at t = 0: a degenerate pivot.  x = (3, 0), z = 6."""
    A = np.array([[1.0, 1.0, 1.0]])
    return A, np.array([3.0]), np.array([2.0, 1.0, 0.0]), np.array([3.0, 1.0, np.inf])
