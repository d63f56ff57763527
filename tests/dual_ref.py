"""Dense numpy restatement of the dual simplex loop (include/simplex.h,
SPX_ALGO_DUAL): explicit B^-1, Dantzig dual pricing (most negative x_b), the
textbook dual ratio test with a pivot tolerance, first index on every tie, no
reinversion.  Conventions are the library's: maximise c.x, A is m x n with
the slack identity in its last m columns, e_j = y.A_j - c_j.

Also the covering-LP generator the dual tests share (`covering`): the order of
the draws fixes the golden values in tests/golden/dual_optima.json.
"""
from dataclasses import dataclass, field

import numpy as np

OPTIMUM, INFEASIBLE, MAX_ITER = "optimum", "infeasible", "max_iter"

# (m, n, seed) of the golden instances; the first four also carry the
# reference's pivot trace
SHAPES = [(7, 20, 0), (65, 200, 1), (130, 390, 2), (256, 1024, 3), (1024, 4096, 4)]
TRACED = SHAPES[:4]


def covering(m: int, n: int, seed: int):
    """min cost.x, G x >= h, x >= 0 in the library's form: max -cost.x,
    -G x + s = -h.  Returns (A m x n row-major, b, c)."""
    ns = n - m
    r = np.random.default_rng(seed)
    G = r.uniform(0, 1, (m, ns))
    h = r.uniform(1, 2, m) * ns / 8
    cost = r.uniform(1, 2, ns)
    A = np.hstack([-G, np.eye(m)])
    b = -h
    c = np.concatenate([-cost, np.zeros(m)])
    return A, b, c


def tiny_infeasible():
    """x1 + x2 <= 1 and x1 + x2 >= 2: infeasible after one dual pivot."""
    A = np.array([[1.0, 1.0, 1.0, 0.0], [-1.0, -1.0, 0.0, 1.0]])
    return A, np.array([1.0, -2.0]), np.array([-1.0, -1.0, 0.0, 0.0])


@dataclass
class DualResult:
    status: str
    z: float
    pivots: int
    b_ixs: np.ndarray
    x_b: np.ndarray
    trace: list = field(default_factory=list)
    y: np.ndarray = None     # final duals and inverse (the exact-tie tests compare them bit for bit)
    Binv: np.ndarray = None
    ties: dict = field(default_factory=dict)  # passes whose argmin met an exact tie: "row", "ratio"
    integral: bool = True    # x_b, y and B^-1 held integers only after every pass


def tied(key):
    """Whether the smallest finite entry of `key` occurs more than once."""
    k = float(np.min(key))
    return bool(np.isfinite(k) and np.count_nonzero(key == k) > 1)


def whole(*arrays):
    return all(bool(np.all(v == np.rint(v))) for v in arrays)


def dual_simplex(A, b, c, feas_tol=1e-9, piv_tol=1e-9, max_iter=1 << 62, trace_cap=200):
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    ns = n - m
    Binv = np.eye(m)
    b_ixs = np.arange(ns, n)
    x_b = np.array(b, dtype=np.float64)
    c_B = np.array(c[ns:], dtype=np.float64)
    y = c_B.copy()
    basic = np.zeros(n, dtype=bool)
    basic[b_ixs] = True
    trace = []
    ties = {"row": 0, "ratio": 0}
    integral = True
    it = 0
    status = MAX_ITER
    while it < max_iter:
        # 1. leaving row: most negative x_b below -feas_tol (argmin: first index)
        q = int(np.argmin(x_b))
        if not x_b[q] < -feas_tol:
            status = OPTIMUM
            break
        ties["row"] += int(tied(x_b))
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
        # 4. FTRAN and update
        alpha = Binv @ A[:, p]
        aq = alpha[q]
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
        integral = integral and whole(x_b, y, Binv)
        if it < trace_cap:
            trace.append((p, q))
        it += 1
    return DualResult(status, float(c_B @ x_b), it, b_ixs.copy(), x_b.copy(), trace, y.copy(), Binv.copy(), ties,
                      integral)
