"""CPU: the lower-bound twins of tests/lower_twins.py meet the condition that
makes a GPU failure on them the device's fault (DESIGN.md §7j "Tests").

For every twin tests/test_gpu_lower_twins.py runs, the shifted problem is formed
as the device forms it (primal_lu_ref.shifted: b_eff = b2 - sum l_j A_j in
ascending j, range = fl(u2 - l)) and the neighbour's numpy restatement runs on
it: it must reproduce the neighbour's golden pivot count, (p, q) trace, basis,
at-upper set and counters, and every one of its own gaps must be >= 1e-6.  The
shifted data differ from the neighbour's by rounding of order 1e-14, ten
orders below the gap, so neither the order of the device's sums nor its fma can
move an argmin.  The smallest gap over all twins is the golden cases' own
(test_smallest_gap): 2.7e-6, primal_box_se_optima.json's at 130 x 390; over the
dual families 1.25e-5.
"""
import numpy as np
import pytest

import dual_box_ref
import dual_ref
import lower_twins as lt
import primal_box_ref
import primal_box_se_ref
import primal_lu_ref

CASES = lt.cases()
_RUNS = {}


def _run(k):
    """(restatement's result on the shifted problem, b_eff, range), once per twin."""
    if k not in _RUNS:
        name, m, n, seed, flipc, rule = k
        A, b, c, u, l, b2, u2 = lt.twin(name, m, n, seed, flipc)
        beff, rng = primal_lu_ref.shifted(A, b2, l, u2)
        _RUNS[k] = (lt.FAMILIES[name].run(A, beff, c, rng, rule), beff, rng)
    return _RUNS[k]


def _resolve(flipc):
    """make_golden_primal_box_wexact.py's resolve() on the boxed dual twin's shifted problem."""
    if ("resolve", flipc) not in _RUNS:
        m, n, seed = lt.RESOLVE_SHAPE
        A, b, c, u, l, b2, u2 = lt.twin("box", m, n, seed, flipc)
        beff, rng = primal_lu_ref.shifted(A, b2, l, u2)
        first = dual_box_ref.dual_simplex_box(A, beff, c, rng, rule=dual_box_ref.STEEPEST, trace_cap=0)
        c2 = primal_box_ref.cost_variant(c, n - m, seed)
        basic = np.zeros(n, dtype=bool)
        basic[first.b_ixs] = True
        w = primal_box_se_ref.exact_weights(A, np.linalg.inv(A[:, first.b_ixs]), basic)
        r = primal_box_se_ref.primal_simplex_box_se(A, beff, c2, rng, basis=first.b_ixs, at_upper=first.at_upper,
                                                    weights=w, trace_cap=200)
        _RUNS[("resolve", flipc)] = (first, r)
    return _RUNS[("resolve", flipc)]


@pytest.mark.parametrize("k", CASES, ids=[lt.case_id(k) for k in CASES])
def test_restatement_walks_the_golden_passes_on_the_shifted_problem(k):
    name, m, n, seed, flipc, rule = k
    fam = lt.FAMILIES[name]
    g = lt.golden_case(fam, m, n, seed, flipc, rule)
    A, b, c, u, l, b2, u2 = lt.twin(name, m, n, seed, flipc)
    r, beff, rng = _run(k)
    # the neighbour's LP up to rounding
    assert np.max(np.abs(beff - b)) <= 1e-13 * max(1.0, np.max(np.abs(b)))
    fin = np.isfinite(u)
    assert np.array_equal(fin, np.isfinite(rng))
    assert np.all(np.abs(rng[fin] - u[fin]) <= 2.0 ** -51 * (np.abs(u[fin]) + 1.0))  # two roundings: u + l, then - l
    if name in ("pbox", "pbox_se"):
        assert np.min(beff) >= 0.0  # the slack basis stays primal feasible: no phase 1 needed
    gaps = {a: getattr(r, a) for a in fam.gaps}
    print(f"{lt.case_id(k)}: pivots {r.pivots} (golden {g['ref_pivots']}) gaps {gaps} "
          f"counters {[getattr(r, a) for a in fam.counters]}")
    assert r.status == dual_ref.OPTIMUM
    assert r.pivots == g["ref_pivots"]
    assert [p for p, _ in r.trace] == g["ref_trace_p"][:200]
    assert [q for _, q in r.trace] == g["ref_trace_q"][:200]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(r.at_upper).tolist() == g["ref_at_upper"]
    for a in fam.counters:
        assert getattr(r, a) == g[a], a
    assert min(gaps.values()) >= lt.MIN_GAP, gaps
    z = g["highs_z"]
    zl, zabs = lt.shift_sum(c, l)
    assert abs(r.z - z) <= 1e-9 * abs(z)  # (the shifted problem's z; the caller's is z + sum c_j l_j)
    # the unshifted certificate of the restatement's basis: the twin's LP is what it claims to be
    viol, dviol, zc = primal_lu_ref.certificate_lu(A, b2, c, l, u2, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - (z + zl)) <= 1e-9 * max(abs(z), zabs)


@pytest.mark.parametrize("flipc", [0, 1])
def test_warm_resolve_twin(flipc):
    """tests/golden/make_golden_primal_box_wexact.py's resolve() on the shifted
    problem of the boxed dual twin: dual steepest solve, new cost, bounded
    primal steepest edge from that basis with exact weights."""
    m, n, seed = lt.RESOLVE_SHAPE
    g = lt.resolve_golden(flipc)
    first, r = _resolve(flipc)
    assert first.status == dual_ref.OPTIMUM and min(first.gap_row, first.gap_ratio) >= lt.MIN_GAP
    gaps = (r.gap_price, r.gap_ratio, r.gap_flip)
    print(f"re-solve twin flipc={flipc}: pivots {r.pivots} (golden {g['ref_pivots']}) flips {r.flips} to upper "
          f"{r.to_upper} gaps {gaps}")
    assert r.status == dual_ref.OPTIMUM
    assert (r.pivots, r.flips, r.to_upper) == (g["ref_pivots"], g["flips"], g["to_upper"])
    assert [p for p, _ in r.trace] == g["ref_trace_p"] and [q for _, q in r.trace] == g["ref_trace_q"]
    assert min(gaps) >= lt.MIN_GAP, gaps
    assert abs(r.z - g["highs_z"]) <= 1e-9 * abs(g["highs_z"])


def test_smallest_gap():
    """The smallest gap any twin's restatement met is the golden cases' own
    smallest, not a new one."""
    own, got = [], []
    for k in CASES:
        fam = lt.FAMILIES[k[0]]
        g = lt.golden_case(fam, *k[1:])
        own.append(min(g[a] for a in fam.gaps))
        got.append(min(getattr(_run(k)[0], a) for a in fam.gaps))
    for flipc in (0, 1):
        g = lt.resolve_golden(flipc)
        own.append(min(g["gap_price"], g["gap_ratio"], g["gap_flip"]))
        r = _resolve(flipc)[1]
        got.append(min(r.gap_price, r.gap_ratio, r.gap_flip))
    print(f"smallest gap over the twins {min(got):.3e}, over their golden cases {min(own):.3e}")
    assert min(got) >= lt.MIN_GAP
    assert min(got) == pytest.approx(min(own), rel=1e-6)
