"""CPU: the long-step ratio test of the bounded primal loop's phase 1
(SPX_PRIMAL_RATIO_LONG_STEP, spx_set_primal_phase_one_ratio).  The
numpy restatement tests/primal_phase1_long_ref.py: with ratio="textbook" against
the restatements it is built from, pass for pass; with ratio="long" its
invariants (ninf never rises, the sum of violations falls at every phase-1 pass
that moves, the textbook optimum with a clean certificate, fewer phase-1 passes)
and its golden file (tests/golden/primal_phase1_long_optima.json, written by
tests/golden/make_golden_primal_phase1_long.py); the exact ties of long_tie();
and the additions to the C-ABI, the Python package and the CLI that need no
device."""
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dual_ref
import primal_lu_ref
import primal_lu_se_ref
import primal_phase1_long_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("boxed_general", "general_lu")
RULES = ("dantzig", "steepest")
SMALL = [(7, 20, 0), (65, 200, 1)]
SETTER = "spx_set_primal_phase_one_ratio"
GETTER = "spx_get_primal_long_steps"


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "primal_phase1_long_optima.json")) as f:
        g = json.load(f)
    g["by_case"] = {(c["family"], c["pricing"], c["m"], c["n"], c["seed"]): c for c in g["cases"]}
    return g


_RUNS = {}


def _run(family, pricing, ratio, m, n, seed):
    """One solve of the restatement per case, shared by the tests below."""
    k = (family, pricing, ratio, m, n, seed)
    if k not in _RUNS:
        _RUNS[k] = ref.primal_simplex_long(*ref.lp_of(family, m, n, seed), pricing=pricing, ratio=ratio, trace_cap=200)
    return _RUNS[k]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("pricing", RULES)
@pytest.mark.parametrize("m,n,seed", SMALL)
def test_textbook_is_the_existing_restatement(family, pricing, m, n, seed):
    lp = ref.lp_of(family, m, n, seed)
    r = _run(family, pricing, "textbook", m, n, seed)
    old = (primal_lu_ref.primal_simplex_lu if pricing == "dantzig" else primal_lu_se_ref.primal_simplex_lu_se)(
        *lp, trace_cap=200)
    assert r.status == old.status == dual_ref.OPTIMUM
    assert r.trace == old.trace and r.pivots == old.pivots and r.ninf_hist == old.ninf_hist
    assert (r.flips, r.to_upper, r.p1_passes, r.p1_pivots, r.ninf0) == (old.flips, old.to_upper, old.p1_passes,
                                                                         old.p1_pivots, old.ninf0)
    assert r.z == old.z and np.array_equal(r.x_b, old.x_b) and np.array_equal(r.Binv, old.Binv)
    assert np.array_equal(r.b_ixs, old.b_ixs) and np.array_equal(r.at_upper, old.at_upper)
    assert (r.gap_price, r.gap_ratio, r.gap_flip) == (old.gap_price, old.gap_ratio, old.gap_flip)
    if pricing == "steepest":
        assert np.array_equal(r.weights, old.weights)
    assert r.long_counters(0) == (0, 0, 0, 0) and r.walks == [] and r.gap_walk == np.inf


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("pricing", RULES)
@pytest.mark.parametrize("m,n,seed", SMALL)
def test_long_invariants_and_golden(golden, family, pricing, m, n, seed):
    g = golden["by_case"][(family, pricing, m, n, seed)]
    lp = ref.lp_of(family, m, n, seed)
    r = _run(family, pricing, "long", m, n, seed)
    t = _run(family, pricing, "textbook", m, n, seed)
    print(f"{family} {pricing} {m}x{n}: pivots {t.pivots} -> {r.pivots}, phase-1 passes {t.p1_passes} -> {r.p1_passes}, walk "
          f"{r.long_counters(1)} gaps {r.gap_price:.2e} {r.gap_ratio:.2e} {r.gap_flip:.2e} {r.gap_walk:.2e} slope "
          f"{r.gap_slope:.2e}")
    assert r.status == dual_ref.OPTIMUM and r.ninf == 0
    # ninf never rises; the sum of violations falls at every phase-1 pass that moves
    assert all(a >= b for a, b in zip(r.ninf_hist, r.ninf_hist[1:]))
    moved = 0
    for k, (ph1, mv) in enumerate(r.step_hist):
        if ph1 and mv:
            assert r.sinf_hist[k + 1] < r.sinf_hist[k], (k, r.sinf_hist[k], r.sinf_hist[k + 1])
            moved += 1
    assert moved > 0
    # the textbook optimum, a clean certificate
    assert abs(r.z - t.z) <= 1e-9 * abs(t.z) and abs(r.z - g["highs_z"]) <= 1e-9 * abs(g["highs_z"])
    viol, dviol, zc = ref.certificate_lu(*lp, r.b_ixs, r.at_upper)
    assert viol <= 1e-9 and dviol <= 1e-7 and abs(zc - t.z) <= 1e-9 * abs(t.z)
    if m >= 65:
        assert r.p1_passes < t.p1_passes
    assert (t.pivots, t.p1_passes) == (g["textbook_pivots"], g["textbook_p1_passes"])
    # the golden file
    assert r.pivots == g["ref_pivots"] and r.z == g["ref_z"]
    assert [p for p, _ in r.trace] == g["ref_trace_p"] and [q for _, q in r.trace] == g["ref_trace_q"]
    assert r.b_ixs.tolist() == g["ref_b_ixs"] and np.flatnonzero(r.at_upper).tolist() == g["ref_at_upper"]
    assert (r.flips, r.to_upper) == (g["flips"], g["to_upper"])
    assert (r.p1_passes, r.p1_pivots, r.ninf0) == (g["p1_passes"], g["p1_pivots"], g["ninf0"])
    assert r.long_counters(1) == (g["long_passed"], g["long_passes"], g["long_max"], 1)
    assert (r.gap_price, r.gap_ratio, r.gap_flip, r.gap_walk, r.gap_slope) == (
        g["gap_price"], g["gap_ratio"], g["gap_flip"], g["gap_walk"], g["gap_slope"])
    assert {k: int(v) for k, v in r.ties.items()} == g["ties"]


def test_golden_file_meets_the_generators_bars(golden):
    """Every committed case: the gaps the generator demands, fewer phase-1
    passes than the textbook solve from 65 x 200 up, a walk that passed rows."""
    assert golden["min_gap"] == 1e-6 and golden["min_slope_gap"] == 1e-10
    assert len(golden["cases"]) == 16
    for g in golden["cases"] + [golden["cut"]]:
        assert min(g["gap_price"], g["gap_ratio"], g["gap_flip"], g["gap_walk"]) >= 1e-6, g["m"]
        assert g["gap_slope"] >= 1e-10 and g["long_passed"] > 0 and g["ties"]["p1_walk"] == 0
    for g in golden["cases"]:
        if g["m"] >= 65:
            assert g["p1_passes"] < g["textbook_p1_passes"], (g["family"], g["pricing"], g["m"])
    c = golden["cut"]
    assert c["m"] == 1100 > 1024 and c["pivots"] == c["ref_pivots"] == 30 and c["ninf"] > 0 and len(c["ref_x_b"]) == 1100


@pytest.mark.parametrize("pricing", RULES)
def test_long_tie(pricing):
    """Two soft breakpoints at one t, then a soft and a hard one at one t: the
    smaller 2 row + side goes first."""
    lp = ref.long_tie()
    r = ref.primal_simplex_long(*lp, pricing=pricing, ratio="long")
    t = ref.primal_simplex_long(*lp, pricing=pricing, ratio="textbook")
    assert r.status == t.status == dual_ref.OPTIMUM and r.z == t.z == -31.0
    assert r.ties["p1_walk"] >= 2 and r.gap_walk == 0.0
    assert r.walks[0] == ([0, 2], 2)   # rows 0 and 1 at t = 2: row 0 is passed, row 1 leaves
    assert r.walks[1] == ([8], 10)     # row 4 (soft) and row 5 (hard) at t = 3: the soft one is passed, h leaves
    assert r.trace[:2] == [(0, 1), (1, 5)] and t.trace[:2] == [(0, 0), (1, 4)]
    assert r.long_counters(1)[:3] == (2, 2, 1)
    viol, dviol, _ = ref.certificate_lu(*lp, r.b_ixs, r.at_upper)
    assert viol == 0.0 and dviol == 0.0


def test_switch_at_is_textbook_until_then():
    family, m, n, seed = "boxed_general", 65, 200, 1
    t = _run(family, "dantzig", "textbook", m, n, seed)
    r = ref.primal_simplex_long(*ref.lp_of(family, m, n, seed), ratio="long", switch_at=20, trace_cap=200)
    assert r.trace[:20] == t.trace[:20] and r.status == dual_ref.OPTIMUM and r.long_passed > 0
    assert abs(r.z - t.z) <= 1e-9 * abs(t.z)


def test_header_and_bindings():
    with open(os.path.join(ROOT, "include", "simplex.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+SPX_PRIMAL_RATIO_TEXTBOOK\s+0\b", h)
    assert re.search(r"#define\s+SPX_PRIMAL_RATIO_LONG_STEP\s+1\b", h)
    assert re.search(r"#define\s+SPX_ABI_VERSION\s+8\b", h) and re.search(r"#define\s+SPX_CONFIG_FIELDS\s+17\b", h)
    flags = {k: int(v) for k, v in re.findall(r"#define\s+(SPX_FLAG_[A-Z0-9_]+)\s+(\d+)\b", h)}
    assert max(flags.values()) == 131072 and not any("RATIO" in k and "PRIMAL" in k for k in flags)  # no new flag
    txt = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"int\s+%s\(spx_ctx\*\s*ctx,\s*int32_t\s+rule\);" % SETTER, txt)
    assert re.search(r"int\s+%s\(spx_ctx\*\s*ctx,\s*int64_t\s+out\[4\]\);" % GETTER, txt)
    assert re.fullmatch(r"[a-z_]+", SETTER) and re.fullmatch(r"[a-z_]+", GETTER)
    assert "Still out: a long-step phase 1" not in h
    import simplex_method_gpu_amd as spx
    from simplex_method_gpu_amd import _lib

    for name in (SETTER, GETTER):
        assert name in _lib.SIGNATURES and name not in _lib.SIGNATURES_NUMBERED
    assert (spx.PRIMAL_RATIO_TEXTBOOK, spx.PRIMAL_RATIO_LONG_STEP) == (0, 1)
    assert "PRIMAL_RATIO_TEXTBOOK" in spx.__all__ and "PRIMAL_RATIO_LONG_STEP" in spx.__all__
    assert callable(spx.Context.set_primal_phase1_ratio) and callable(spx.Context.primal_long_steps)
    par = inspect.signature(spx.Context.__init__).parameters
    assert list(par)[-1] == "primal_free_pricing" and not any("ratio" in k and "primal" in k for k in par)
    assert not [k for k in dir(spx) if k.startswith("FLAG_") and "RATIO" in k]
    lib = _lib.load()
    assert lib.spx_abi_version() == 8 and hasattr(lib, SETTER) and hasattr(lib, GETTER)
    assert getattr(lib, SETTER)(None, spx.PRIMAL_RATIO_LONG_STEP) == -1  # SPX_ERR_ARG
    assert b"NULL" in lib.spx_last_error()
    assert getattr(lib, GETTER)(None, None) == -1


def test_cli_usage_and_refusals():
    solver = os.path.join(ROOT, "solver")
    r = subprocess.run([solver, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "[--ranging PREFIX] [--bound-ranging PREFIX] [--phase1-ratio textbook|long]" in r.stderr
    # the options that were there keep their places in the usage text
    assert ("[--primal-box [--phase1] [--primal-pricing dantzig|steepest] [--phase1-pricing dantzig|steepest] "
            "[--free-pricing dantzig|steepest] [--primal-weights reference|exact]]") in r.stderr
    assert "[--dual-pricing dantzig|steepest] [--dual-ratio textbook|long] [--bounds F] [--lower F]" in r.stderr
    r = subprocess.run([solver, "--phase1-ratio", "long", "--gen", "8", "16", "0"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "--phase1-ratio needs --primal-box" in r.stderr
    r = subprocess.run([solver, "--primal-box", "--phase1-ratio", "harris", "--gen", "8", "16", "0"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--phase1-ratio harris: textbook or long" in r.stderr
    r = subprocess.run([solver, "--primal-box", "--phase1-ratio"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr  # the option without its argument
    with open(os.path.join(ROOT, "simplex_method_gpu_amd", "csrc", "solver_main.cpp")) as f:
        head = f.read().split("#include", 1)[0]
    assert "//   --phase1-ratio R" in head and "SPX_PRIMAL_RATIO_LONG_STEP" in head


def test_docs_no_longer_list_it_as_out():
    for name in ("README.md", "DESIGN.md"):
        with open(os.path.join(ROOT, name)) as f:
            txt = f.read()
        assert "long-step phase 1 that walks past breakpoints" not in txt, name
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert re.search(r"^## 7o\. ", f.read(), flags=re.M)
