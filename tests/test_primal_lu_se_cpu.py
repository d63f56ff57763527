"""CPU: steepest-edge pricing with free columns in the bounded primal loop
(SPX_FLAG_PRIMAL_FREE_STEEPEST, spx_set_primal_free_pricing).  The
numpy restatement tests/primal_lu_se_ref.py against its golden file
(tests/golden/primal_lu_se_optima.json, written by
tests/golden/make_golden_primal_lu_se.py) on both generators; without free
columns against the restatements it is built from, pass for pass; its weights
against the exact norms; and the additions to the C-ABI, the Python package and
the CLI that need no device."""
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dual_ref
import primal_box_ref
import primal_box_se_ref
import primal_lu_ref
import primal_lu_se_ref as ref
import primal_phase1_se_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7, 20, 0), (65, 200, 1), (130, 390, 2), (256, 1024, 3)]
KINDS = ("general", "feasible")
SETTER = "spx_set_primal_free_pricing"
FLAG = 131072


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "primal_lu_se_optima.json")) as f:
        g = json.load(f)
    g["by_shape"] = {(k, c["m"], c["n"], c["seed"]): c for k in KINDS for c in g[k]}
    return g


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_ref_reproduces_golden(golden, kind, m, n, seed):
    g = golden["by_shape"][(kind, m, n, seed)]
    A, b, c, l, u = (ref.general_lu if kind == "general" else ref.free_feasible)(m, n, seed)
    r = ref.primal_simplex_lu_se(A, b, c, l, u, trace_cap=200)
    print(f"{kind} {m}x{n}: pivots={r.pivots} (Dantzig {g['dantzig_pivots']}) flips={r.flips} to_upper={r.to_upper} phase 1 "
          f"{r.p1_passes}/{r.p1_pivots} ninf0={r.ninf0} free entered {r.free_entered} basic {r.free_basic} z={r.z:.13g} "
          f"gaps {r.gap_price:.2e} {r.gap_ratio:.2e} {r.gap_flip:.2e} drift {r.drift_enter:.1e} {r.drift_final:.1e}")
    assert r.status == dual_ref.OPTIMUM and r.ninf == 0
    assert r.pivots == g["ref_pivots"] and r.z == g["ref_z"]
    assert [p for p, _ in r.trace] == g["ref_trace_p"] and [q for _, q in r.trace] == g["ref_trace_q"]
    assert r.b_ixs.tolist() == g["ref_b_ixs"] and np.flatnonzero(r.at_upper).tolist() == g["ref_at_upper"]
    assert (r.flips, r.to_upper, r.fixed_flips) == (g["flips"], g["to_upper"], g["fixed_flips"])
    assert (r.p1_passes, r.p1_pivots, r.ninf0) == (g["p1_passes"], g["p1_pivots"], g["ninf0"])
    assert (r.free_entered, r.free_basic) == (g["free_entered"], g["free_basic"])
    assert (r.gap_price, r.gap_ratio, r.gap_flip) == (g["gap_price"], g["gap_ratio"], g["gap_flip"])
    assert (r.drift_enter, r.drift_final) == (g["drift_enter"], g["drift_final"])
    assert {k: int(v) for k, v in r.ties.items()} == g["ties"]
    # what the generator demands of every case
    assert min(r.gap_price, r.gap_ratio, r.gap_flip) >= golden["min_gap"] == 1e-6
    assert r.free_entered > 0 and r.free_basic > 0 and r.pivots < g["dantzig_pivots"]
    assert (r.p1_pivots > 0) == (kind == "general") and (r.ninf0 == 0) == (kind == "feasible")
    assert all(v == 0 for v in r.ties.values())
    z = g["highs_z"]
    assert abs(r.z - z) <= 1e-9 * abs(z), (r.z, z)
    viol, dviol, zc = ref.certificate_lu(A, b, c, l, u, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7 and abs(zc - z) <= 1e-9 * abs(z), (viol, dviol, zc)
    # ninf never grows, and phase 1 is one prefix of the passes
    h = r.ninf_hist
    assert all(h[i + 1] <= h[i] for i in range(len(h) - 1)) and sum(1 for v in h if v > 0) == r.p1_passes
    # the recurrence weights against the exact norms at the end: what drift_final records
    basic = np.zeros(n, dtype=bool)
    basic[r.b_ixs] = True
    ex = primal_box_se_ref.exact_weights(A, r.Binv, basic)
    assert np.max(np.abs(r.weights[~basic] - ex[~basic]) / ex[~basic]) == r.drift_final <= 1e-9
    assert r.drift_enter <= 1e-9


@pytest.mark.parametrize("m,n,seed", SHAPES[:3])
def test_dantzig_count_is_the_lu_restatement(golden, m, n, seed):
    for kind in KINDS:
        g = golden["by_shape"][(kind, m, n, seed)]
        A, b, c, l, u = (ref.general_lu if kind == "general" else ref.free_feasible)(m, n, seed)
        d = primal_lu_ref.primal_simplex_lu(A, b, c, l, u, trace_cap=0)
        assert d.status == dual_ref.OPTIMUM and d.pivots == g["dantzig_pivots"]
        assert abs(d.z - g["highs_z"]) <= 1e-9 * abs(g["highs_z"])


def test_weights_half_way(golden):
    """Cut half-way through phase 1 and half-way through the feasible solve: the
    weights are the exact norms of that basis within the recorded drift."""
    m, n, seed = 130, 390, 2
    for kind in KINDS:
        g = golden["by_shape"][(kind, m, n, seed)]
        A, b, c, l, u = (ref.general_lu if kind == "general" else ref.free_feasible)(m, n, seed)
        k = (g["p1_pivots"] if kind == "general" else g["ref_pivots"]) // 2
        r = ref.primal_simplex_lu_se(A, b, c, l, u, max_iter=k)
        assert r.status == dual_ref.MAX_ITER and r.pivots == k and (kind != "general" or r.ninf > 0)
        assert [p for p, _ in r.trace] == g["ref_trace_p"][:k]
        assert r.drift_final <= max(g["drift_enter"], g["drift_final"])


def test_no_free_column_walks_the_parents():
    """Without a free column: primal_simplex_phase1_se's passes on boxed_general
    (through phase 1) and primal_simplex_box_se's on boxed_primal, bit for bit."""
    m, n, seed = 65, 200, 1
    A, b, c, u = primal_phase1_se_ref.boxed_general(m, n, seed)
    a = ref.primal_simplex_lu_se(A, b, c, np.zeros(n), u)
    w = primal_phase1_se_ref.primal_simplex_phase1_se(A, b, c, u)
    assert a.p1_pivots > 0 and a.free_entered == 0
    assert a.trace == w.trace and a.pivots == w.pivots and a.z == w.z
    assert (a.flips, a.to_upper, a.p1_passes, a.p1_pivots, a.ninf0) == (w.flips, w.to_upper, w.p1_passes, w.p1_pivots,
                                                                       w.ninf0)
    assert np.array_equal(a.weights, w.weights) and np.array_equal(a.x_b, w.x_b) and np.array_equal(a.Binv, w.Binv)
    A, b, c, u = primal_box_ref.boxed_primal(m, n, seed)
    a = ref.primal_simplex_lu_se(A, b, c, np.zeros(n), u)
    w = primal_box_se_ref.primal_simplex_box_se(A, b, c, u)
    assert a.trace == w.trace and a.pivots == w.pivots and a.z == w.z and a.p1_passes == 0
    assert np.array_equal(a.weights, w.weights) and np.array_equal(a.x_b, w.x_b)


def test_free_feasible_generator():
    for m, n, seed in SHAPES[:3]:
        A, b, c, l, u = ref.free_feasible(m, n, seed)
        A0, b0, c0, u0 = primal_box_ref.boxed_primal(m, n, seed)
        ns = n - m
        fr = np.isneginf(l)
        assert np.array_equal(A, A0) and np.array_equal(b, b0)
        assert np.array_equal(np.flatnonzero(fr), np.arange(2, ns, 5)) and np.all(np.isposinf(u[fr]))
        assert np.array_equal(l[~fr], np.zeros(n - fr.sum())) and np.array_equal(c[~fr], c0[~fr])
        assert np.all(np.abs(c[fr]) <= 1.0) and (m == 7 or (np.any(c[fr] < 0) and np.any(c[fr] > 0)))
        assert np.all(np.isfinite(u[ns:]))
        wide = ~np.isfinite(u0[ns:])
        assert np.array_equal(u[ns:][wide], np.abs(b[wide]) + 0.25 * ns) and np.array_equal(u[ns:][~wide], u0[ns:][~wide])
        assert np.all(b >= 0) and np.all(b <= u[ns:])  # the slack basis is within its bounds


def test_exact_tie_and_unbounded():
    A, b, c, l, u = ref.free_tie()
    r = ref.primal_simplex_lu_se(A, b, c, l, u)
    ent = [p for p, _ in r.trace]
    assert r.status == dual_ref.OPTIMUM and r.ties["free_price"] > 0 and r.gap_price == 0.0
    assert 2 in ent and 3 not in ent  # the smaller index enters; its twin then prices at 0
    k = ent.index(2)
    cut = ref.primal_simplex_lu_se(A, b, c, l, u, max_iter=k)
    w0 = primal_box_se_ref.reference_weights(A)
    assert cut.weights[2] == cut.weights[3] != w0[2] and w0[2] == w0[3]  # the recurrence moved both alike
    A, b, c, l, u = ref.tiny_unbounded_free()
    r = ref.primal_simplex_lu_se(A, b, c, l, u)
    assert r.status == primal_box_ref.UNBOUNDED and r.ray_col == 0 and r.pivots == 0


def test_header_and_bindings():
    with open(os.path.join(ROOT, "include", "simplex.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+SPX_FLAG_PRIMAL_FREE_STEEPEST\s+%d\b" % FLAG, h)
    assert re.search(r"#define\s+SPX_ABI_VERSION\s+8\b", h)  # additive: the version stays
    flags = {k: int(v) for k, v in re.findall(r"#define\s+(SPX_FLAG_[A-Z0-9_]+)\s+(\d+)\b", h)}
    assert max(v for k, v in flags.items() if k != "SPX_FLAG_PRIMAL_FREE_STEEPEST") == FLAG // 2  # the next unused bit
    assert len(set(flags.values())) == len(flags)
    txt = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"int\s+%s\(spx_ctx\*\s*ctx,\s*int32_t\s+rule\);" % SETTER, txt)
    assert not re.search(r"\d", SETTER)  # tests/test_abi.py's scan reads [a-z_] names
    import simplex_method_gpu_amd as spx
    from simplex_method_gpu_amd import _lib

    assert SETTER in _lib.SIGNATURES and SETTER not in _lib.SIGNATURES_NUMBERED
    assert callable(spx.Context.set_primal_free_pricing)
    par = inspect.signature(spx.Context.__init__).parameters
    assert par["primal_free_pricing"].default == spx.PRIMAL_PRICING_DANTZIG
    assert list(par)[-1] == "primal_free_pricing"  # appended: no earlier keyword moved
    lib = _lib.load()
    assert lib.spx_abi_version() == 8 and hasattr(lib, SETTER)
    fn = getattr(lib, SETTER)
    assert fn(None, spx.PRIMAL_PRICING_STEEPEST) == -1  # SPX_ERR_ARG
    assert b"NULL" in lib.spx_last_error()
    with pytest.raises(ValueError):
        spx.Context(m=8, n=16, seed=0, primal_free_pricing=7)


def test_cli_usage_and_refusals():
    solver = os.path.join(ROOT, "solver")
    r = subprocess.run([solver, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "[--free-pricing dantzig|steepest]" in r.stderr
    # the options that were there keep their places in the usage text
    assert ("[--primal-box [--phase1] [--primal-pricing dantzig|steepest] [--phase1-pricing dantzig|steepest] "
            "[--free-pricing dantzig|steepest] [--primal-weights reference|exact]]") in r.stderr
    assert "[--bounds F] [--lower F] [--ranging PREFIX]" in r.stderr
    r = subprocess.run([solver, "--free-pricing", "steepest", "--gen", "8", "16", "0"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "--free-pricing needs --primal-box" in r.stderr
    r = subprocess.run([solver, "--primal-box", "--free-pricing", "devex", "--gen", "8", "16", "0"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--free-pricing devex: dantzig or steepest" in r.stderr
    r = subprocess.run([solver, "--primal-box", "--free-pricing"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr  # the option without its argument
    # the refusals that were there keep their words and exit codes
    r = subprocess.run([solver, "--primal-pricing", "steepest", "--gen", "8", "16", "0"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "--primal-pricing needs --primal-box" in r.stderr and "usage" in r.stderr
    r = subprocess.run([solver, "--phase1-pricing", "steepest", "--gen", "8", "16", "0"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "--phase1-pricing needs --primal-box" in r.stderr
    r = subprocess.run([solver, "--lower", "nowhere.txt", "--gen", "8", "16", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--lower needs --dual or --primal-box" in r.stderr
    with open(os.path.join(ROOT, "simplex_method_gpu_amd", "csrc", "solver_main.cpp")) as f:
        head = f.read().split("#include", 1)[0]
    assert "//   --free-pricing R" in head and "SPX_FLAG_PRIMAL_FREE_STEEPEST" in head
