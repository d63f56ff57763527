"""Generate tests/golden/lds_cap_optima.json: the golden values of the dual and
the bounded primal loop's tests at the two heights where their vectors outgrow
LDS (tests/test_gpu_lds_cap.py): m = 6401 (L = 6528, 24 L
bytes no longer fit 150 KiB) and m = 9601 (L = 9728, 16 L no longer fit), n = m
+ 64.

The LPs are the neighbouring tests' generators at those shapes (CASES below; the
boxed dual LP is dual_box_ref.boxed_tall, boxed() with wider slack bounds, since
boxed() itself is infeasible this far from square, and the phase-1 LP is
primal_phase1_ref.boxed_general_tall, which starts with tens of rows out of their
bounds, not thousands); the runs are the existing numpy restatements, once to 24
pivots and once to the optimum.  Stored per case: the first 24 (p, q), the pivot count, the flip and
phase-1 counters after 24 pivots and at the optimum, HiGHS's optimum, the
restatement's smallest gaps, and the restatement's own residuals after 24 pivots
and at the optimum measured with tests/block_ref.py (B^-1 B - I, x_b, y, the
weights where the rule keeps some).  The GPU tests allow 100 x those residuals.
A case is refused ("pick another seed") when a gap is below MIN_GAP or z is off
HiGHS by more than Z_REL relative.

The unboxed dual loop with Dantzig pricing runs through tests/dual_box_ref.py
with no finite bound (tests/dual_ref.py's pass, which records no gaps).

    python tests/golden/make_golden_lds_cap.py [case ...]

Cases named on the command line are (re)computed and merged into the file, so
the seven can run side by side; each takes minutes and a few GB.
"""
from __future__ import annotations

import fcntl
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
from scipy.optimize import linprog

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import block_ref  # noqa: E402
import dual_box_ref  # noqa: E402
import dual_long_ref  # noqa: E402
import dual_ref  # noqa: E402
import dual_se_ref  # noqa: E402
import primal_box_ref  # noqa: E402
import primal_box_se_ref  # noqa: E402
import primal_phase1_ref  # noqa: E402

HEAD = 24
MIN_GAP = 1e-6
Z_REL = 1e-9
NS = 64
PATH = os.path.join(HERE, "lds_cap_optima.json")

# name: (kind, m, seed, rule, flipc)
CASES = {
    "dual_se_6401": ("dual", 6401, 11, "steepest", 0),
    "long_se_6401": ("long", 6401, 12, "steepest", 1),
    "pbox_se_6401": ("pbox_se", 6401, 13, "steepest", 0),
    "dual_9601": ("dual", 9601, 14, "dantzig", 0),
    "long_9601": ("long", 9601, 15, "dantzig", 0),
    "pbox_9601": ("pbox", 9601, 16, "dantzig", 0),
    "pbox_p1_9601": ("phase1", 9601, 17, "dantzig", 0),
}


def lp(kind, m, seed, flipc):
    """(A, b, c, u) of the case; u is None for the unboxed dual loop."""
    n = m + NS
    if kind == "dual":
        return (*dual_ref.covering(m, n, seed), None)
    if kind == "long":
        return dual_box_ref.boxed_tall(m, n, seed, bool(flipc))
    if kind in ("pbox", "pbox_se"):
        return primal_box_ref.boxed_primal(m, n, seed)
    return primal_phase1_ref.boxed_general_tall(m, n, seed)


def run(kind, rule, A, b, c, u, max_iter):
    if kind == "dual" and rule == "steepest":
        return dual_se_ref.dual_simplex_se(A, b, c, max_iter=max_iter, trace_cap=HEAD)
    if kind == "dual":
        return dual_box_ref.dual_simplex_box(A, b, c, np.full(A.shape[1], np.inf), rule=dual_box_ref.DANTZIG,
                                             max_iter=max_iter, trace_cap=HEAD)
    if kind == "long":
        return dual_long_ref.dual_simplex_long(A, b, c, u, rule=rule, max_iter=max_iter, trace_cap=HEAD)
    if kind == "pbox":
        return primal_box_ref.primal_simplex_box(A, b, c, u, max_iter=max_iter, trace_cap=HEAD)
    if kind == "pbox_se":
        return primal_box_se_ref.primal_simplex_box_se(A, b, c, u, max_iter=max_iter, trace_cap=HEAD)
    return primal_phase1_ref.primal_simplex_phase1(A, b, c, u, max_iter=max_iter, trace_cap=HEAD)


def highs(A, b, c, u):
    n = A.shape[1]
    bounds = [(0.0, None if u is None or not np.isfinite(u[j]) else float(u[j])) for j in range(n)]
    r = linprog(-c, A_eq=sp.csr_matrix(A), b_eq=b, bounds=bounds, method="highs")
    assert r.status == 0, r.status
    return -float(r.fun)


def counters(kind, r):
    if kind == "dual":
        return {}
    if kind == "long":
        return {"flips": r.flips, "flip_passes": r.flip_passes, "max_flips": r.max_flips, "to_upper": r.to_upper,
                "placed": r.placed}
    out = {"flips": r.flips, "to_upper": r.to_upper}
    if kind == "phase1":
        out.update({"p1_passes": r.p1_passes, "p1_pivots": r.p1_pivots, "ninf0": r.ninf0, "ninf": r.ninf})
    return out


def gaps(kind, r):
    if kind == "dual":
        return {"row": r.gap_row, "ratio": r.gap_ratio}
    if kind == "long":
        return {"row": r.gap_row, "ratio": r.gap_ratio, "walk": r.gap_walk, "slope": r.gap_slope}
    return {"price": r.gap_price, "ratio": r.gap_ratio, "flip": r.gap_flip}


def residuals(kind, rule, r, A, b, c, u):
    ns = A.shape[1] - A.shape[0]
    blk = block_ref.Block(A[:, :ns], r.b_ixs)
    up = getattr(r, "at_upper", None)
    out = blk.residuals(r.Binv, r.x_b, r.y, blk.b_eff(b, u, up), c)
    out["k"] = blk.k
    if kind in ("dual", "long") and rule == "steepest":
        out["w"] = blk.dual_weight_residual(dual_se_ref.row_norms2(r.Binv))
    if kind == "pbox_se":
        out["w"] = blk.primal_weight_residual(r.weights)  # the recurrence's weights
        out["w_exact"] = blk.primal_weight_residual(primal_box_se_ref.exact_weights(A, r.Binv, blk.basic))
    return out


def case(name):
    kind, m, seed, rule, flipc = CASES[name]
    n = m + NS
    t0 = time.time()
    A, b, c, u = lp(kind, m, seed, flipc)
    hz = highs(A, b, c, u)
    head = run(kind, rule, A, b, c, u, HEAD)
    assert head.pivots == HEAD, (name, head.status, head.pivots)
    res_head = residuals(kind, rule, head, A, b, c, u)
    cnt_head = counters(kind, head)
    del head
    r = run(kind, rule, A, b, c, u, 1 << 62)
    if r.status != dual_ref.OPTIMUM:
        raise SystemExit(f"{name}: status {r.status}: pick another seed")
    g = gaps(kind, r)
    rel = abs(r.z - hz) / abs(hz)
    print(f"{name}: {m}x{n} seed {seed}: z={hz:.13g} (HiGHS rel {rel:.1e}) pivots={r.pivots} counters={counters(kind, r)} "
          f"gaps={g} ({time.time() - t0:.0f} s)", flush=True)
    if rel > Z_REL:
        raise SystemExit(f"{name}: z differs from HiGHS by {rel:.1e} relative: pick another seed")
    if min(g.values()) < MIN_GAP:
        raise SystemExit(f"{name}: a gap of {min(g.values()):.1e} is below {MIN_GAP:g}: pick another seed")
    res_opt = residuals(kind, rule, r, A, b, c, u)
    print(f"{name}: residuals after {HEAD}: {res_head}; at the optimum: {res_opt}", flush=True)
    return {"name": name, "kind": kind, "m": m, "n": n, "seed": seed, "rule": rule, "flipc": flipc, "highs_z": hz,
            "ref_pivots": r.pivots, "ref_trace_p": [int(p) for p, _ in r.trace[:HEAD]],
            "ref_trace_q": [int(q) for _, q in r.trace[:HEAD]], "counters_head": cnt_head,
            "counters": counters(kind, r), "gaps": g, "res_head": res_head, "res_opt": res_opt}


def main():
    names = sys.argv[1:] or list(CASES)
    done = [case(name) for name in names]
    out = {"generator": "dual_ref.covering / dual_box_ref.boxed_tall / primal_box_ref.boxed_primal / "
                        "primal_phase1_ref.boxed_general_tall at (m, m + 64, seed)",
           "reference": "the numpy restatements of tests/*_ref.py (first index on ties); residuals: tests/block_ref.py",
           "solver": "scipy %s linprog(method='highs')" % __import__("scipy").__version__,
           "head": HEAD, "min_gap": MIN_GAP, "cases": []}
    lock = os.open(HERE, os.O_RDONLY)  # (runs side by side merge one at a time)
    fcntl.flock(lock, fcntl.LOCK_EX)
    if os.path.exists(PATH):
        with open(PATH) as f:
            out["cases"] = [c for c in json.load(f)["cases"] if c["name"] not in names]
    out["cases"] = sorted(out["cases"] + done, key=lambda c: list(CASES).index(c["name"]))
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1)
    os.close(lock)


if __name__ == "__main__":
    main()
