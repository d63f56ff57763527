"""CPU: tests/block_ref.py against numpy's dense inverse at a small shape, the
golden file of tests/test_gpu_lds_cap.py, and spx_loop_layout's declaration."""
import json
import os
import re

import numpy as np

import block_ref
import dual_box_ref
import dual_ref
import primal_box_ref
import primal_box_se_ref
import primal_phase1_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_ref_against_the_dense_inverse():
    """A basis with re-entered slacks (their columns of B^-1 are not unit
    vectors) and columns at their upper bounds, after a whole steepest-edge
    solve of 301 x 365."""
    m, n, seed = 301, 365, 13
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    r = primal_box_se_ref.primal_simplex_box_se(A, b, c, u, trace_cap=0)
    assert r.status == dual_ref.OPTIMUM and r.at_upper.any()
    blk = block_ref.Block(A[:, :n - m], r.b_ixs)
    assert 0 < blk.k <= 64
    Bi = np.linalg.inv(A[:, r.b_ixs])
    beff = b - A[:, r.at_upper] @ u[r.at_upper]
    assert np.allclose(blk.b_eff(b, u, r.at_upper).astype(float), beff, rtol=0, atol=1e-13)
    x = Bi @ beff
    assert np.max(np.abs(blk.solve(beff).astype(float) - x)) <= 1e-11 * np.max(np.abs(x))
    y = c[r.b_ixs] @ Bi
    assert np.max(np.abs(blk.solve_t(c[r.b_ixs]).astype(float) - y)) <= 1e-11 * np.max(np.abs(y))
    w = np.einsum("ij,ij->i", Bi, Bi)
    assert np.max(np.abs(blk.dual_weights().astype(float) - w) / w) <= 1e-10
    nb, g = blk.primal_weights()
    ex = primal_box_se_ref.exact_weights(A, Bi, blk.basic)[nb]
    assert np.max(np.abs(g.astype(float) - ex) / ex) <= 1e-10
    # the restatement's state: small residuals, some non-unit slack columns; a damaged entry shows
    res = blk.residuals(r.Binv, r.x_b, r.y, blk.b_eff(b, u, r.at_upper), c)
    assert res["binv"] <= 1e-11 and res["x_b"] <= 1e-11 and res["y"] <= 1e-11 and res["nonunit"] > 0
    bad = r.Binv.copy()
    bad[5, blk.S[0]] += 1e-6
    assert blk.binv_residual(bad)[0] >= 1e-7
    bad = r.Binv.copy()
    good = np.flatnonzero(np.count_nonzero(r.Binv[:, blk.rows_t], axis=0) == 1)[0]
    bad[7, blk.rows_t[good]] += 1e-6  # a unit column that is one no longer
    res2, nonunit2 = blk.binv_residual(bad)
    assert nonunit2 == res["nonunit"] + 1 and res2 >= 9e-7
    viol, dviol, z = blk.certificate(b, c, u, r.at_upper)
    v0, d0, z0 = dual_box_ref.certificate(A, b, c, u, r.b_ixs, r.at_upper)
    assert abs(viol - v0) <= 1e-12 and abs(dviol - d0) <= 1e-12 and abs(z - z0) <= 1e-11 * abs(z0)


def test_tall_generators_are_feasible_where_the_square_ones_are_not():
    m, n, seed = 301, 365, 12
    A, b, c, u = dual_box_ref.boxed_tall(m, n, seed, True)
    r = dual_box_ref.dual_simplex_box(A, b, c, u, trace_cap=0)
    assert r.status == dual_ref.OPTIMUM
    A0, b0, c0, u0 = dual_box_ref.boxed(m, n, seed, True)
    assert np.array_equal(A, A0) and np.array_equal(u[:n - m], u0[:n - m]) and np.array_equal(u[n - m:], 16 * u0[n - m:])
    A, b, c, u = primal_phase1_ref.boxed_general_tall(m, n, 17, every=30)
    r = primal_phase1_ref.primal_simplex_phase1(A, b, c, u, trace_cap=0)
    assert r.status == dual_ref.OPTIMUM and 0 < r.ninf0 < m // 10 and r.p1_pivots > 0


def test_golden_file():
    with open(os.path.join(ROOT, "tests", "golden", "lds_cap_optima.json")) as f:
        g = json.load(f)
    names = [c["name"] for c in g["cases"]]
    assert names == ["dual_se_6401", "long_se_6401", "pbox_se_6401", "dual_9601", "long_9601", "pbox_9601",
                     "pbox_p1_9601"]
    for c in g["cases"]:
        assert c["n"] == c["m"] + 64 and c["m"] in (6401, 9601)
        assert min(c["gaps"].values()) >= g["min_gap"] == 1e-6, c["name"]
        assert len(c["ref_trace_p"]) == len(c["ref_trace_q"]) == g["head"] == 24 <= c["ref_pivots"]
        for part in ("res_head", "res_opt"):
            assert all(0.0 < c[part][k] < 1e-9 for k in ("binv", "x_b", "y")), (c["name"], part)
            assert ("w" in c[part]) == (c["rule"] == "steepest")


def test_loop_layout_is_declared_and_additive(spx):
    txt = open(os.path.join(ROOT, "include", "simplex.h")).read()
    assert re.search(r"int\s+spx_loop_layout\(spx_ctx\*\s*ctx,\s*int32_t\s+out\[SPX_LOOP_LAYOUT_FIELDS\]\);", txt)
    assert re.search(r"#define\s+SPX_LOOP_LAYOUT_FIELDS\s+8\b", txt)
    assert re.search(r"#define\s+SPX_ABI_VERSION\s+8\b", txt)  # additive: the version stays
    L = spx._lib.load()
    assert "spx_loop_layout" in spx._lib.SIGNATURES and hasattr(L, "spx_loop_layout")
    assert hasattr(spx.Context, "loop_layout")
    import ctypes
    out = (ctypes.c_int32 * 8)()
    assert L.spx_loop_layout(None, out) == -1  # SPX_ERR_ARG, not a crash
