"""Lower-bound twins of the neighbouring golden cases (DESIGN.md §7j "Tests"),
shared by tests/test_lower_twins_cpu.py and tests/test_gpu_lower_twins.py.

A twin is a neighbour's LP (A, b, c, 0 <= x <= u) moved by
primal_lu_ref.lower_twin: l on about 40 % of all columns, b2 = b + A.l, u2 = u +
l.  Its shifted problem is the neighbour's own LP up to rounding of order
1e-14, and the neighbour's golden file was generated under a gap rule (every
argmin separated by at least 1e-6), so under l <= x <= u2 every loop must walk
the neighbour's golden passes: the same pivot count, (p, q) trace, basis,
at-upper set and counters, and HiGHS's optimum plus sum_j c_j l_j.

FAMILIES names, per family, the golden file, the generator, the numpy
restatement and its gap fields and counters; `cases()` lists the twins, at 65 x
200 and 130 x 390 only.
"""
import json
import os

import numpy as np

import dual_box_ref
import dual_long_ref
import primal_box_ref
import primal_box_se_ref
import primal_lu_ref
import primal_phase1_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(65, 200, 1), (130, 390, 2)]
RESOLVE_SHAPE = (130, 390, 2)
MIN_GAP = 1e-6
DUAL_COMBOS = [(flipc, rule) for flipc in (0, 1) for rule in (dual_box_ref.DANTZIG, dual_box_ref.STEEPEST)]


class Family:
    def __init__(self, name, golden, lp, run, gaps, counters, combos=((None, None),)):
        self.name, self.golden, self.lp, self.run = name, golden, lp, run
        self.gaps, self.counters, self.combos = gaps, counters, combos

    @property
    def dual(self):
        return self.name in ("box", "long")


def _boxed(m, n, seed, flipc):
    return dual_box_ref.boxed(m, n, seed, bool(flipc))


def _primal(m, n, seed, flipc):
    return primal_box_ref.boxed_primal(m, n, seed)


def _general(m, n, seed, flipc):
    return primal_phase1_ref.boxed_general(m, n, seed)


FAMILIES = {f.name: f for f in (
    Family("box", "dual_box_optima.json", _boxed,
           lambda A, b, c, u, rule: dual_box_ref.dual_simplex_box(A, b, c, u, rule=rule, trace_cap=200),
           ("gap_row", "gap_ratio"), ("to_upper", "placed"), DUAL_COMBOS),
    Family("long", "dual_long_optima.json", _boxed,
           lambda A, b, c, u, rule: dual_long_ref.dual_simplex_long(A, b, c, u, rule=rule, trace_cap=200),
           ("gap_row", "gap_walk", "gap_slope"), ("to_upper", "placed", "flips", "flip_passes", "max_flips"),
           DUAL_COMBOS),
    Family("pbox", "primal_box_optima.json", _primal,
           lambda A, b, c, u, rule: primal_box_ref.primal_simplex_box(A, b, c, u, trace_cap=200),
           ("gap_price", "gap_ratio", "gap_flip"), ("flips", "to_upper")),
    Family("pbox_se", "primal_box_se_optima.json", _primal,
           lambda A, b, c, u, rule: primal_box_se_ref.primal_simplex_box_se(A, b, c, u, trace_cap=200),
           ("gap_price", "gap_ratio", "gap_flip"), ("flips", "to_upper")),
    Family("phase1", "primal_phase1_optima.json", _general,
           lambda A, b, c, u, rule: primal_phase1_ref.primal_simplex_phase1(A, b, c, u, trace_cap=200),
           ("gap_price", "gap_ratio", "gap_flip"), ("flips", "to_upper", "p1_passes", "p1_pivots", "ninf0")),
)}

_GOLD = {}


def gold(name):
    if name not in _GOLD:
        with open(os.path.join(ROOT, "tests", "golden", name)) as f:
            _GOLD[name] = json.load(f)
    return _GOLD[name]


def golden_case(fam, m, n, seed, flipc, rule):
    for g in gold(fam.golden)["cases"]:
        if (g["m"], g["n"], g["seed"], g.get("flipc"), g.get("rule")) == (m, n, seed, flipc, rule):
            return g
    raise KeyError((fam.name, m, n, seed, flipc, rule))


def cases():
    """(family name, m, n, seed, flipc, rule) of every twin."""
    return [(f.name, m, n, seed, flipc, rule) for f in FAMILIES.values() for (m, n, seed) in SHAPES
            for (flipc, rule) in f.combos]


def case_id(k):
    name, m, n, seed, flipc, rule = k
    return f"{name}-{m}x{n}" + ("" if rule is None else f"-flipc{flipc}-{rule}")


_TWINS = {}


def twin(name, m, n, seed, flipc):
    """(A, b, c, u, l, b2, u2) of a twin: the neighbour's LP and its moved
    bounds and right-hand side, built once."""
    fam = FAMILIES[name]
    k = (fam.lp, m, n, seed, flipc)
    if k not in _TWINS:
        A, b, c, u = fam.lp(m, n, seed, flipc)
        l, b2, u2 = primal_lu_ref.lower_twin(A, b, u, seed)
        assert np.all(np.isfinite(l)) and not np.any(l == u2) and np.count_nonzero(l) > 0.3 * n
        assert np.any(l[n - m:] != 0.0) and np.any(l[:n - m] != 0.0)
        _TWINS[k] = (A, b, c, u, l, b2, u2)
    return _TWINS[k]


def resolve_golden(flipc):
    """primal_box_wexact_optima.json's `resolve` record at RESOLVE_SHAPE."""
    case = {(c["m"], c["n"], c["seed"]): c for c in gold("primal_box_wexact_optima.json")["resolve"]}[RESOLVE_SHAPE]
    g = case["flipc"][flipc]
    assert g["flipc"] == flipc
    return g


def shift_sum(c, l):
    """sum_j c_j l_j in np.longdouble, and sum_j |c_j l_j| (what cancels)."""
    t = np.asarray(c, dtype=np.longdouble) * np.asarray(l, dtype=np.longdouble)
    return float(np.sum(t)), float(np.sum(np.abs(t)))
