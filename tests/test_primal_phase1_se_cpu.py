"""CPU: steepest-edge pricing through phase 1 of the bounded primal loop
(SPX_FLAG_PRIMAL_PHASE1_STEEPEST, spx_set_primal_phase_one_pricing; DESIGN.md
§7l).  The numpy restatement tests/primal_phase1_se_ref.py against its golden
file (tests/golden/primal_phase1_se_optima.json, written by
tests/golden/make_golden_primal_phase1_se.py) at the four shapes it shares with
the Dantzig golden, on the contradictory rows and on the warm start (the two
larger golden shapes take the restatement a minute and are checked for
consistency only); fewer pivots than Dantzig's phase 1; and the additions to
the C-ABI, the Python package and the CLI that need no device."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dual_ref
import primal_box_ref
import primal_box_se_ref
import primal_phase1_se_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = [(7, 20, 0), (65, 200, 1), (130, 390, 2), (256, 1024, 3)]
SETTER = "spx_set_primal_phase_one_pricing"


def _load(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden():
    g = _load("primal_phase1_se_optima.json")
    g["by_shape"] = {(c["m"], c["n"], c["seed"]): c for c in g["cases"]}
    return g


@pytest.fixture(scope="module")
def dantzig():
    g = _load("primal_phase1_optima.json")
    g["by_shape"] = {(c["m"], c["n"], c["seed"]): c for c in g["cases"]}
    return g


def _same_counts(r, g):
    assert r.pivots == g["ref_pivots"]
    assert (r.flips, r.to_upper) == (g["flips"], g["to_upper"])
    assert (r.p1_passes, r.p1_pivots, r.ninf0) == (g["p1_passes"], g["p1_pivots"], g["ninf0"])
    assert g["p1_flips"] == g["p1_passes"] - g["p1_pivots"]
    assert (r.gap_price, r.gap_ratio, r.gap_flip) == (g["gap_price"], g["gap_ratio"], g["gap_flip"])
    assert {k: int(v) for k, v in r.ties.items()} == g["ties"]
    assert (r.drift_enter, r.drift_final) == (g["drift_enter"], g["drift_final"])


@pytest.mark.parametrize("m,n,seed", SHARED)
def test_ref_reproduces_golden(golden, dantzig, m, n, seed):
    g = golden["by_shape"][(m, n, seed)]
    d = dantzig["by_shape"][(m, n, seed)]
    A, b, c, u = ref.boxed_general(m, n, seed)
    r = ref.primal_simplex_phase1_se(A, b, c, u, trace_cap=200)
    print(f"{m}x{n}: pivots={r.pivots} (Dantzig {d['ref_pivots']}) flips={r.flips} to_upper={r.to_upper} phase 1 "
          f"{r.p1_passes}/{r.p1_pivots} ninf0={r.ninf0} z={r.z:.13g} gaps {r.gap_price:.2e} {r.gap_ratio:.2e} "
          f"{r.gap_flip:.2e} drift {r.drift_enter:.1e} {r.drift_final:.1e}")
    assert r.status == dual_ref.OPTIMUM and r.ninf == 0
    _same_counts(r, g)
    assert [p for p, _ in r.trace] == g["ref_trace_p"]
    assert [q for _, q in r.trace] == g["ref_trace_q"]
    assert r.b_ixs.tolist() == g["ref_b_ixs"]
    assert np.flatnonzero(r.at_upper).tolist() == g["ref_at_upper"]
    assert r.p1_pivots > 0 and r.ninf0 == d["ninf0"]  # the same entry
    z = g["highs_z"]
    assert z == d["highs_z"]
    assert abs(r.z - z) <= 1e-9 * abs(z), (r.z, z)
    # the point of the rule: strictly fewer pivots than Dantzig's phase 1 and phase 2
    assert r.pivots < d["ref_pivots"] == g["dantzig_pivots"]
    # ninf is monotone non-increasing over every pass, and phase 1 is one prefix of the passes
    h = r.ninf_hist
    assert h[0] == r.ninf0 and all(h[i + 1] <= h[i] for i in range(len(h) - 1))
    assert sum(1 for v in h if v > 0) == r.p1_passes
    viol, dviol, zc = ref.certificate(A, b, c, u, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7, (viol, dviol)
    assert abs(zc - z) <= 1e-9 * abs(z)
    # the recurrence weights against the exact norms at the end: what drift_final records
    basic = np.zeros(n, dtype=bool)
    basic[r.b_ixs] = True
    ex = primal_box_se_ref.exact_weights(A, r.Binv, basic)
    assert np.max(np.abs(r.weights[~basic] - ex[~basic]) / ex[~basic]) == r.drift_final <= 1e-8


def test_golden_is_consistent(golden):
    assert golden["min_gap"] == 1e-6
    shapes = [(c["m"], c["n"], c["seed"]) for c in golden["cases"]]
    assert shapes == SHARED + [(512, 2048, 4), (1024, 4096, 4)]
    for c in golden["cases"] + [golden["infeasible"], golden["stuck"]]:
        gap = min(c["gap_price"], c["gap_ratio"], c["gap_flip"])
        assert c["traced"] == (gap >= golden["min_gap"]) or c is golden["stuck"], (c["m"], gap)
        assert all(v == 0 for v in c["ties"].values())
        assert c["p1_pivots"] > 0 and c["p1_passes"] >= c["p1_pivots"]
    by = {s: c for s, c in zip(shapes, golden["cases"])}
    assert not by[(256, 1024, 3)]["traced"]  # a pricing gap below 1e-6: compared by optimum and certificate only
    for s in [(7, 20, 0), (65, 200, 1), (130, 390, 2), (512, 2048, 4), (1024, 4096, 4)]:
        assert by[s]["traced"], s
    for c in golden["cases"][-2:]:
        assert abs(c["ref_z"] - c["highs_z"]) <= 1e-9 * abs(c["highs_z"])


def test_mid_phase1_cut(golden):
    """max_iter inside phase 1: the prefix of the trace, rows still out, y as
    the library reads it back (c_B.B^-1)."""
    m, n, seed = 65, 200, 1
    g = golden["by_shape"][(m, n, seed)]
    A, b, c, u = ref.boxed_general(m, n, seed)
    k = g["p1_pivots"] // 2
    r = ref.primal_simplex_phase1_se(A, b, c, u, max_iter=k)
    assert r.status == dual_ref.MAX_ITER and r.pivots == r.p1_pivots == k and r.ninf > 0
    assert [p for p, _ in r.trace] == g["ref_trace_p"][:k]
    assert np.allclose(r.y, c[r.b_ixs] @ r.Binv, rtol=0, atol=1e-12)


def test_infeasible(golden, dantzig):
    g = golden["infeasible"]
    m, n, seed = g["m"], g["n"], g["seed"]
    A, b, c, u = ref.boxed_general(m, n, seed)
    A2, b2, u2 = ref.contradict(A, b, u)
    r = ref.primal_simplex_phase1_se(A2, b2, c, u2, trace_cap=0)
    assert r.status == ref.INFEASIBLE and r.ninf == g["ninf_end"] > 0
    _same_counts(r, g)
    assert r.pivots < dantzig["infeasible"]["ref_pivots"] == g["dantzig_pivots"]
    assert r.p1_passes == r.pivots + r.flips  # every committed pass was a phase-1 pass
    A, b, c, u = ref.tiny_infeasible()
    r = ref.primal_simplex_phase1_se(A, b, c, u)
    assert r.status == ref.INFEASIBLE and r.pivots == 0 == golden["tiny_infeasible"]["ref_pivots"]


def test_stuck_warm_start(golden, dantzig):
    g = golden["stuck"]
    m, n, seed = g["m"], g["n"], g["seed"]
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    first = primal_box_se_ref.primal_simplex_box_se(A, b, c, u, trace_cap=0)
    assert first.status == dual_ref.OPTIMUM and first.pivots == g["first_pivots"]
    c2 = primal_box_ref.cost_variant(c, n - m, seed)
    b2 = ref.rhs_variant(b, seed)
    r = ref.primal_simplex_phase1_se(A, b2, c2, u, basis=first.b_ixs, at_upper=first.at_upper, weights=first.weights,
                                     trace_cap=0)
    assert r.status == dual_ref.OPTIMUM
    _same_counts(r, g)
    z = g["highs_z"]
    assert z == dantzig["stuck"]["highs_z"] and abs(r.z - z) <= 1e-9 * abs(z)
    assert r.ninf0 == dantzig["stuck"]["ninf0"]


def test_feasible_entry_is_the_plain_steepest_edge_loop():
    """ninf == 0 at entry: primal_box_se_ref's loop pass for pass, bit for bit."""
    m, n, seed = 65, 200, 1
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    a = ref.primal_simplex_phase1_se(A, b, c, u)
    w = primal_box_se_ref.primal_simplex_box_se(A, b, c, u)
    assert a.trace == w.trace and a.pivots == w.pivots and a.z == w.z and a.p1_passes == 0
    assert np.array_equal(a.weights, w.weights)


def test_header_and_bindings():
    with open(os.path.join(ROOT, "include", "simplex.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+SPX_FLAG_PRIMAL_PHASE1_STEEPEST\s+65536\b", h)
    assert re.search(r"#define\s+SPX_ABI_VERSION\s+8\b", h)  # additive: the version stays
    txt = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"int\s+%s\(spx_ctx\*\s*ctx,\s*int32_t\s+rule\);" % SETTER, txt)
    assert not re.search(r"\d", SETTER)  # tests/test_abi.py's scan reads [a-z_] names
    import simplex_method_gpu_amd as spx
    from simplex_method_gpu_amd import _lib

    assert spx.FLAG_PRIMAL_PHASE1_STEEPEST == 65536 and "FLAG_PRIMAL_PHASE1_STEEPEST" in spx.__all__
    # the next free bit: no other FLAG_* of the package holds it or a higher one
    others = [getattr(spx, k) for k in dir(spx) if k.startswith("FLAG_") and k != "FLAG_PRIMAL_PHASE1_STEEPEST"]
    assert all(v < 65536 for v in others)
    assert SETTER in _lib.SIGNATURES and SETTER not in _lib.SIGNATURES_NUMBERED
    assert callable(spx.Context.set_primal_phase1_pricing)
    import inspect

    par = inspect.signature(spx.Context.__init__).parameters
    assert par["primal_phase1_pricing"].default == spx.PRIMAL_PRICING_DANTZIG
    lib = _lib.load()
    assert lib.spx_abi_version() == 8 and hasattr(lib, SETTER)
    fn = getattr(lib, SETTER)
    assert fn(None, spx.PRIMAL_PRICING_STEEPEST) == -1  # SPX_ERR_ARG
    assert b"NULL" in lib.spx_last_error()
    with pytest.raises(ValueError):
        spx.Context(m=8, n=16, seed=0, primal_phase1_pricing=7)


def test_cli_usage_and_refusals():
    solver = os.path.join(ROOT, "solver")
    r = subprocess.run([solver, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "[--phase1-pricing dantzig|steepest]" in r.stderr
    r = subprocess.run([solver, "--phase1-pricing", "steepest", "--gen", "8", "16", "0"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "--phase1-pricing needs --primal-box" in r.stderr
    r = subprocess.run([solver, "--primal-box", "--phase1-pricing", "devex", "--gen", "8", "16", "0"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--phase1-pricing devex: dantzig or steepest" in r.stderr
