"""Generate tests/golden/primal_phase1_long_optima.json: the golden values of the
tests of phase 1's long-step ratio test in the bounded primal loop
(tests/test_primal_phase1_long_cpu.py, tests/test_gpu_primal_phase1_long.py;
DESIGN.md §7o).

Families `boxed_general` (tests/primal_phase1_ref.py) and `general_lu`
(tests/primal_lu_ref.py, a fifth of the structural columns free) at SHAPES from the
slack basis, under both entering rules, with ratio="long": the numpy
restatement's (tests/primal_phase1_long_ref.py primal_simplex_long) optimum, pivot
count, first 200 (p, q) pairs, final basis and at-upper set, the flip and
to-upper counts, the phase-1 counters, the walk's counters and the smallest gaps.
`highs_z` and the textbook solve's pivot and phase-1 pass counts are copied from
the neighbouring golden files of the same LP (the optimum does not depend on the
ratio test): primal_phase1_optima.json / primal_phase1_se_optima.json for
`boxed_general`, primal_lu_optima.json / primal_lu_se_optima.json for `general_lu`.
One more case, `cut`: boxed_general 1100 x 2300 (more rows than k_pbox_long1 has
threads) under Dantzig, stopped after its first 30 pivots, with the restatement's
x_b.

A case is refused when a price, ratio, flip or walk gap is below MIN_GAP, when the
slope gap is below MIN_SLOPE_GAP (the rounding of the slope's sum is of order m
2^-53, about 1e-13 here), when z differs from HiGHS by more than Z_REL relative,
when ninf rises, when the certificate is not clean, or when the walk passed
nothing: change the seed, never the bar.

    python tests/golden/make_golden_primal_phase1_long.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import dual_ref  # noqa: E402
import primal_phase1_long_ref as ref  # noqa: E402

TRACE = 200
MIN_GAP = 1e-6
MIN_SLOPE_GAP = 1e-10
Z_REL = 1e-9
SHAPES = [(7, 20, 0), (65, 200, 1), (130, 390, 2), (256, 1024, 3)]
CUT = ("boxed_general", 1100, 2300, 5, 30)
NEIGHBOURS = {("boxed_general", "dantzig"): ("primal_phase1_optima.json", "cases"),
              ("boxed_general", "steepest"): ("primal_phase1_se_optima.json", "cases"),
              ("general_lu", "dantzig"): ("primal_lu_optima.json", "cases"),
              ("general_lu", "steepest"): ("primal_lu_se_optima.json", "general")}


def neighbour(family, pricing, m, n, seed):
    file, key = NEIGHBOURS[(family, pricing)]
    with open(os.path.join(HERE, file)) as f:
        g = json.load(f)
    for c in g[key]:
        if (c["m"], c["n"], c["seed"]) == (m, n, seed):
            return c
    raise SystemExit(f"{file}: no case {m} x {n} seed {seed}")


def check_gaps(tag, r):
    gap = min(r.gap_price, r.gap_ratio, r.gap_flip, r.gap_walk)
    if gap < MIN_GAP:
        raise SystemExit(f"{tag}: smallest gap {gap:.2e} below {MIN_GAP:.0e}: change the seed")
    if r.gap_slope < MIN_SLOPE_GAP:
        raise SystemExit(f"{tag}: slope gap {r.gap_slope:.2e} below {MIN_SLOPE_GAP:.0e}: change the seed")
    if any(a < b for a, b in zip(r.ninf_hist, r.ninf_hist[1:])):
        raise SystemExit(f"{tag}: ninf rises")
    if r.long_passed <= 0:
        raise SystemExit(f"{tag}: the walk passed nothing")


def fields(r):
    return {"ref_pivots": r.pivots, "ref_trace_p": [int(p) for p, _ in r.trace], "ref_trace_q": [int(q) for _, q in r.trace],
            "ref_b_ixs": [int(j) for j in r.b_ixs], "ref_at_upper": [int(j) for j in np.flatnonzero(r.at_upper)],
            "flips": r.flips, "to_upper": r.to_upper, "p1_passes": r.p1_passes, "p1_pivots": r.p1_pivots,
            "ninf0": r.ninf0, "ninf": r.ninf, "long_passed": r.long_passed, "long_passes": r.long_passes,
            "long_max": r.long_max, "gap_price": r.gap_price, "gap_ratio": r.gap_ratio, "gap_flip": r.gap_flip,
            "gap_walk": r.gap_walk, "gap_slope": r.gap_slope, "ties": {k: int(v) for k, v in r.ties.items()}}


def one(family, pricing, m, n, seed):
    lp = ref.lp_of(family, m, n, seed)
    nb = neighbour(family, pricing, m, n, seed)
    hz = nb["highs_z"]
    r = ref.primal_simplex_long(*lp, pricing=pricing, ratio="long", trace_cap=TRACE)
    tag = f"{family} {pricing} m={m}"
    print(f"{tag} n={n} seed={seed}: {r.status} z={r.z:.13g} (HiGHS {hz:.13g}, rel {abs(r.z - hz) / abs(hz):.1e}) pivots="
          f"{r.pivots} (textbook {nb['ref_pivots']}) p1 {r.p1_passes}/{r.p1_pivots} (textbook {nb['p1_passes']}) walk "
          f"{r.long_passed}/{r.long_passes}/{r.long_max} gaps {r.gap_price:.2e} {r.gap_ratio:.2e} {r.gap_flip:.2e} "
          f"{r.gap_walk:.2e} slope {r.gap_slope:.2e}", flush=True)
    if r.status != dual_ref.OPTIMUM:
        raise SystemExit(f"{tag}: status {r.status}")
    if abs(r.z - hz) > Z_REL * abs(hz):
        raise SystemExit(f"{tag}: z {r.z!r} differs from HiGHS {hz!r}")
    check_gaps(tag, r)
    viol, dviol, _ = ref.certificate_lu(*lp, r.b_ixs, r.at_upper)
    if viol > 1e-9 or dviol > 1e-7:
        raise SystemExit(f"{tag}: certificate {viol:.2e} {dviol:.2e}")
    out = {"family": family, "pricing": pricing, "m": m, "n": n, "seed": seed, "highs_z": hz, "ref_z": r.z,
           "textbook_pivots": nb["ref_pivots"], "textbook_p1_passes": nb["p1_passes"]}
    out.update(fields(r))
    return out


def cut():
    family, m, n, seed, k = CUT
    lp = ref.lp_of(family, m, n, seed)
    r = ref.primal_simplex_long(*lp, pricing="dantzig", ratio="long", max_iter=k, trace_cap=TRACE)
    tag = f"cut {family} m={m}"
    print(f"{tag} n={n} seed={seed}: {r.status} after {r.pivots} pivots, p1 {r.p1_passes}/{r.p1_pivots} ninf {r.ninf0} -> "
          f"{r.ninf} walk {r.long_passed}/{r.long_passes}/{r.long_max} gaps {r.gap_price:.2e} {r.gap_ratio:.2e} "
          f"{r.gap_flip:.2e} {r.gap_walk:.2e} slope {r.gap_slope:.2e}", flush=True)
    if r.status != dual_ref.MAX_ITER or r.pivots != k or r.ninf <= 0:
        raise SystemExit(f"{tag}: {r.status} after {r.pivots} pivots, ninf {r.ninf}")
    check_gaps(tag, r)
    out = {"family": family, "pricing": "dantzig", "m": m, "n": n, "seed": seed, "pivots": k,
           "ref_x_b": [float(v) for v in r.x_b]}
    out.update(fields(r))
    return out


def main():
    out = {"generators": {"boxed_general": "tests/primal_phase1_ref.py boxed_general(m, n, seed), lower bounds 0",
                          "general_lu": "tests/primal_lu_ref.py general_lu(m, n, seed)"},
           "reference": "tests/primal_phase1_long_ref.py primal_simplex_long(ratio='long') (first index on ties)",
           "min_gap": MIN_GAP, "min_slope_gap": MIN_SLOPE_GAP, "cases": []}
    for family in ("boxed_general", "general_lu"):
        for pricing in ("dantzig", "steepest"):
            for (m, n, seed) in SHAPES:
                out["cases"].append(one(family, pricing, m, n, seed))
    out["cut"] = cut()
    with open(os.path.join(HERE, "primal_phase1_long_optima.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
