"""Plain numpy reference for a basis of A = [N | I] with few basic structural
columns, in np.longdouble with matmuls only (no m x m factorisation): what the
tests of the dual and the bounded primal loop at m = 6401 and m = 9601 compare
the device state with (tests/test_gpu_lds_cap.py, tests/golden/make_golden_lds_cap.py).

The block structure.  b_ixs lists the basic columns in basis order; position i
holds either a structural column j < ns or the slack of row r (column ns + r).
Write
  pos_c, cols   the k positions that hold structural columns, and those columns,
  pos_t, rows_t the m - k positions that hold slacks, and those slacks' rows,
  S             the k rows whose slack is not basic,
  U = N[S, cols] (k x k),  Nt = N[rows_t, cols] ((m - k) x k).
Row r of B x = v reads, for r in S, U x[pos_c] = v[S], and for r = rows_t[i],
x[pos_t[i]] + Nt[i] x[pos_c] = v[r].  So with U^-1 alone
  B^-1 v :  x[pos_c] = U^-1 v[S],  x[pos_t] = v[rows_t] - Nt x[pos_c]
  w B^-1 :  y[rows_t] = w[pos_t],  y[S] = (w[pos_c] - w[pos_t] Nt) U^-1
and B^-1 itself is zero outside the columns S except for a 1 at (pos_t[i],
rows_t[i]): the column of B^-1 that belongs to a basic slack is a unit vector,
exactly so in fp64 as long as that slack has never left the basis, because a
rank-1 update then only ever adds products with an exact zero to it.

U^-1 is numpy's fp64 inverse refined by three Newton steps in longdouble (X <-
X + X (I - U X)); with k <= 64 that is a few thousand operations, and its error
is far below the fp64 rounding the comparisons are about.
"""
import numpy as np

LD = np.longdouble
MAX_K = 64


def _inv_ld(U):
    k = U.shape[0]
    if k == 0:
        return np.zeros((0, 0), dtype=LD)
    X = np.linalg.inv(U.astype(np.float64)).astype(LD)
    eye = np.eye(k, dtype=LD)
    for _ in range(3):
        X = X + X @ (eye - U @ X)
    return X


def _rel(got, want):
    """max |got - want| over max |want| (normwise: one small entry sets no scale)."""
    scale = float(np.max(np.abs(want))) if want.size else 0.0
    err = float(np.max(np.abs(got.astype(LD) - want))) if want.size else 0.0
    return err / scale if scale > 0.0 else err


class Block:
    def __init__(self, N, b_ixs):
        """N: the m x ns structural columns (fp64), b_ixs: the basis in basis order."""
        N = np.asarray(N, dtype=np.float64)
        m, ns = N.shape
        b_ixs = np.asarray(b_ixs, dtype=np.int64)
        assert b_ixs.shape == (m,) and len(set(b_ixs.tolist())) == m
        self.N, self.m, self.ns, self.b_ixs = N, m, ns, b_ixs
        self.pos_c = np.flatnonzero(b_ixs < ns)
        self.cols = b_ixs[self.pos_c]
        self.pos_t = np.flatnonzero(b_ixs >= ns)
        self.rows_t = b_ixs[self.pos_t] - ns
        in_t = np.zeros(m, dtype=bool)
        in_t[self.rows_t] = True
        self.S = np.flatnonzero(~in_t)
        self.k = len(self.pos_c)
        assert len(self.S) == self.k <= MAX_K, self.k
        self.U = N[np.ix_(self.S, self.cols)].astype(LD)
        self.Nt = N[np.ix_(self.rows_t, self.cols)].astype(LD)
        self.Uinv = _inv_ld(self.U)
        self.basic = np.zeros(ns + m, dtype=bool)
        self.basic[b_ixs] = True

    # -- the two solves
    def solve(self, V):
        """B^-1 V for V of m rows (a vector or a matrix), longdouble."""
        V = np.asarray(V, dtype=LD)
        out = np.zeros(V.shape, dtype=LD)
        xc = self.Uinv @ V[self.S]
        out[self.pos_c] = xc
        out[self.pos_t] = V[self.rows_t] - self.Nt @ xc
        return out

    def solve_t(self, w):
        """w B^-1 for w in basis order, longdouble."""
        w = np.asarray(w, dtype=LD)
        y = np.zeros(self.m, dtype=LD)
        y[self.rows_t] = w[self.pos_t]
        y[self.S] = (w[self.pos_c] - w[self.pos_t] @ self.Nt) @ self.Uinv
        return y

    # -- the right-hand side of a boxed state
    def b_eff(self, b, u=None, at_upper=None):
        """b - sum over the non-basic columns at upper of u_j A_j."""
        v = np.asarray(b, dtype=LD).copy()
        if at_upper is None or u is None:
            return v
        up = np.asarray(at_upper, dtype=bool) & ~self.basic
        js = np.flatnonzero(up[:self.ns])
        if len(js):
            v -= self.N[:, js].astype(LD) @ np.asarray(u, dtype=LD)[js]
        rs = np.flatnonzero(up[self.ns:])
        v[rs] -= np.asarray(u, dtype=LD)[self.ns + rs]
        return v

    # -- residuals of a state read back from the device or kept by a restatement
    def binv_residual(self, binv):
        """(max |B^-1 B - I|, columns of basic slacks that are not exact unit
        vectors).  A basic slack's column of B^-1 B is that slack's column of
        binv; the structural positions' columns are binv[:, S] N[S, cols] plus
        what the unit columns pick out of N (computed that way for the exact
        ones, by the product for the others)."""
        m, k = self.m, self.k
        assert binv.shape == (m, m)
        nnz = np.count_nonzero(binv, axis=0)
        bad = (nnz[self.rows_t] != 1) | (binv[self.pos_t, self.rows_t] != 1.0)
        res = 0.0
        if bad.any():
            E = binv[:, self.rows_t[bad]].astype(LD)
            E[self.pos_t[bad], np.arange(int(bad.sum()))] -= 1.0
            res = float(np.max(np.abs(E)))
        if k:
            G = np.concatenate([self.S, self.rows_t[bad]])
            R = binv[:, G].astype(LD) @ self.N[np.ix_(G, self.cols)].astype(LD)
            R[self.pos_t[~bad]] += self.Nt[~bad]
            R[self.pos_c, np.arange(k)] -= 1.0
            res = max(res, float(np.max(np.abs(R))))
        return res, int(bad.sum())

    def xb_residual(self, x_b, b_eff):
        return _rel(np.asarray(x_b), self.solve(b_eff))

    def y_residual(self, y, c):
        """y against c_B B^-1, c: the n costs."""
        return _rel(np.asarray(y), self.solve_t(np.asarray(c, dtype=LD)[self.b_ixs]))

    def dual_weights(self):
        """||row_i(B^-1)||^2 in basis order."""
        w = np.zeros(self.m, dtype=LD)
        w[self.pos_c] = np.einsum("ij,ij->i", self.Uinv, self.Uinv)
        T = self.Nt @ self.Uinv
        w[self.pos_t] = 1.0 + np.einsum("ij,ij->i", T, T)
        return w

    def primal_weights(self):
        """(non-basic columns ascending, 1 + ||B^-1 A_j||^2 for them)."""
        nb = np.flatnonzero(~self.basic)
        V = np.zeros((self.m, len(nb)), dtype=LD)
        for t, j in enumerate(nb):
            if j < self.ns:
                V[:, t] = self.N[:, j]
            else:
                V[j - self.ns, t] = 1.0
        X = self.solve(V)
        return nb, 1.0 + np.einsum("ij,ij->j", X, X)

    def dual_weight_residual(self, w):
        want = self.dual_weights()
        return float(np.max(np.abs(np.asarray(w).astype(LD) - want) / want))

    def primal_weight_residual(self, w):
        nb, want = self.primal_weights()
        return float(np.max(np.abs(np.asarray(w)[nb].astype(LD) - want) / want))

    def residuals(self, binv, x_b, y, b_eff, c):
        r, nonunit = self.binv_residual(binv)
        return {"binv": r, "nonunit": nonunit, "x_b": self.xb_residual(x_b, b_eff), "y": self.y_residual(y, c)}

    # -- the certificate of a basis and placements
    def certificate(self, b, c, u=None, at_upper=None):
        """(worst bound violation of x, worst sign violation of the reduced
        costs, z), the quantities of tests/dual_box_ref.py certificate()."""
        n = self.ns + self.m
        u = np.full(n, np.inf) if u is None else np.asarray(u, dtype=np.float64)
        up = np.zeros(n, dtype=bool) if at_upper is None else np.asarray(at_upper, dtype=bool) & ~self.basic
        c = np.asarray(c, dtype=LD)
        x = np.where(up, np.where(np.isfinite(u), u, 0.0), 0.0).astype(LD)
        x[self.b_ixs] = self.solve(self.b_eff(b, u, up))
        viol = max(float(np.max(-x)), float(np.max(x - u)), 0.0)
        y = self.solve_t(c[self.b_ixs])
        e = np.concatenate([y @ self.N.astype(LD), y]) - c
        nb = ~self.basic
        dviol = max(float(np.max(np.where(nb & ~up, -e, 0.0))), float(np.max(np.where(nb & up, e, 0.0))), 0.0)
        return viol, dviol, float(c @ x)
