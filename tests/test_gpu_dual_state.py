"""GPU: who invalidates the dual loop's two host flags (DualState, csrc/spx_ctx.h:
`w_stale`, the steepest-edge weights are not the current basis's, and `checked`,
the basis passed the dual feasibility check), pinned through the public
interface.

Weights: on the covering LP 65 x 200 seed 1 (m no multiple of 64: the padded
rows 65..127 are in play) `dual_weights()` must be the squared row norms of
numpy's inverse of the basis matrix after every event of the table, at the
relative 1e-9 of tests/test_gpu_dual_se.py (which holds there after reinvert and
set_basis at 130 x 390 and 256 x 1024; the basis matrices here are smaller and
no worse conditioned).  A stale flag left unset shows as the weights of an
earlier basis, a flag set where the passes keep the weights would not show here
but costs a k_dual_norms launch and nothing else.  The solve that follows the
reset must then walk the golden pivots of test_gpu_dual_se.py::test_trace_parity.

Checked: a failed check must not count as a check.
"""
import json
import os

import numpy as np
import pytest

import dual_ref
import dual_se_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9


def _case(name, key):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return {(c["m"], c["n"], c["seed"]): c for c in json.load(f)["cases"]}[key]


def _check_weights(ctx, A_cols, what):
    w = ctx.dual_weights()
    B = np.ascontiguousarray(A_cols[np.asarray(ctx.state()["b_ixs"], dtype=np.int64)].T)
    ref = dual_se_ref.row_norms2(np.linalg.inv(B))
    err = float(np.max(np.abs(w - ref) / ref))
    print(f"{what}: largest relative weight error {err:.2e}")
    assert err <= REL, (what, err)
    return w


def test_weights_follow_every_event(spx):
    m, n, seed = dual_ref.SHAPES[1]
    assert (m, n, seed) == (65, 200, 1)
    g = _case("dual_se_optima.json", (m, n, seed))
    z = _case("dual_optima.json", (m, n, seed))["highs_z"]
    A, b, c = dual_ref.covering(m, n, seed)
    A = np.ascontiguousarray(A.T)
    with spx.Context(A, b, c, window=-1, trace=200, algorithm=spx.ALGO_DUAL,
                     dual_pricing=spx.DUAL_PRICING_STEEPEST) as ctx:
        st, piv = ctx.iterate(10)
        assert st == spx.SolveStatus.MaxIter and piv == 10
        _check_weights(ctx, A, "iterate(10)")
        ctx.set_rhs(1.05 * b)
        st, piv = ctx.iterate(3)
        assert piv == 13
        _check_weights(ctx, A, "set_rhs(1.05 b), iterate(3)")
        ctx.set_rhs(b)
        kept = _check_weights(ctx, A, "set_rhs(b)")
        ctx.set_dual_pricing(spx.DUAL_PRICING_DANTZIG)
        st, piv = ctx.iterate(3)
        assert piv == 16
        ctx.set_dual_pricing(spx.DUAL_PRICING_STEEPEST)
        w = _check_weights(ctx, A, "3 Dantzig pivots between two rule changes")
        assert not np.allclose(w, kept, rtol=1e-6, atol=0.0)  # (three pivots later: not the weights kept before them)
        ctx.set_algorithm(spx.ALGO_PRIMAL)
        ctx.set_algorithm(spx.ALGO_DUAL)
        _check_weights(ctx, A, "set_algorithm(PRIMAL), set_algorithm(DUAL)")
        ctx.set_bounds(np.full(n, np.inf))
        _check_weights(ctx, A, "set_bounds(+inf)")
        ctx.reset()
        w = _check_weights(ctx, A, "reset")
        assert w.tolist() == [1.0] * m  # the slack basis: B^-1 = I
        r = ctx.solve()
        tp, tq = ctx.trace()
    print(f"after the reset: z={r.z:.13g} pivots={r.pivots} (golden {g['ref_pivots']})")
    assert g["ref_pivots"] == 34
    assert r.status == spx.SolveStatus.OptimumFound
    assert r.pivots == g["ref_pivots"], (r.pivots, g["ref_pivots"])
    assert tp.tolist() == g["ref_trace_p"][:34]
    assert tq.tolist() == g["ref_trace_q"][:34]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert abs(r.z - z) <= REL * abs(z), (r.z, z)


def test_a_failed_check_is_no_check(spx, oracle):
    """The basis of tests/test_gpu_dual.py::test_not_dual_feasible_then_primal
    (some c_j > 0 at the slack basis): refused on every call, and again after
    spx_set_basis of that same basis."""
    A, b, c = oracle.generate(64, 256, 0)
    with spx.Context(A, b, c, window=-1, algorithm=spx.ALGO_DUAL) as ctx:
        basis = ctx.state()["b_ixs"]
        for what in ("first", "second", "after set_basis"):
            if what == "after set_basis":
                ctx.set_basis(basis)
            with pytest.raises(spx.SimplexError) as ei:
                ctx.iterate(1)
            assert ei.value.code == -5 and "basis is not dual feasible" in str(ei.value), what
            assert ctx.state()["pivots"] == 0
