"""CPU: sensitivity ranging at the optimum (spx_ranging_cost, spx_ranging_rhs,
spx_ranging_times).  The additions to the C-ABI, the Python
package and the CLI that need no device, and the numpy restatement
(tests/ranging_ref.py) itself: against brute force (move one c_j or one b_r to
0.999 and 1.001 of every sampled finite limit and look at the optimality and
feasibility conditions), on two hand-made LPs (an exact tie, a free non-basic
column), and the GPU tests' cases against the case builder's refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

import ranging_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "simplex.h")
NEW_FUNCTIONS = ("spx_ranging_cost", "spx_ranging_rhs", "spx_ranging_times")


def test_header_prototypes():
    txt = open(HEADER).read()
    assert re.search(r"#define\s+SPX_ABI_VERSION\s+8\b", txt)
    assert re.search(r"int\s+spx_ranging_cost\(spx_ctx\*\s*ctx,\s*double\*\s*down,\s*double\*\s*up,\s*int64_t\*\s*"
                     r"block_down,\s*int64_t\*\s*block_up\);", txt)
    assert re.search(r"int\s+spx_ranging_rhs\(spx_ctx\*\s*ctx,\s*double\*\s*down,\s*double\*\s*up,\s*int64_t\*\s*"
                     r"leave_down,\s*int64_t\*\s*leave_up\);", txt)
    assert re.search(r"int\s+spx_ranging_times\(spx_ctx\*\s*ctx,\s*double\s+ms\[2\],\s*int64_t\s+launches\[2\]\);", txt)
    for name in NEW_FUNCTIONS:
        assert not re.search(r"\d", name)


def test_binding_and_package(spx):
    L = spx._lib.load()
    assert L.spx_abi_version() == 8
    for name in NEW_FUNCTIONS:
        assert name in spx._lib.SIGNATURES and name not in spx._lib.SIGNATURES_NUMBERED and hasattr(L, name), name
    for name in ("cost_ranging", "rhs_ranging", "ranging_times"):
        assert callable(getattr(spx.Context, name)), name
    assert spx.CostRanging._fields == ("down", "up", "block_down", "block_up")
    assert spx.RhsRanging._fields == ("down", "up", "leave_down", "leave_up")
    # NULL contexts and result arrays are refused before anything touches a device
    assert L.spx_ranging_cost(None, None, None, None, None) == -1
    assert L.spx_ranging_rhs(None, None, None, None, None) == -1
    assert L.spx_ranging_times(None, None, None) == -1


def test_cli_refuses_ranging_without_a_bounded_loop(tmp_path):
    solver = os.path.join(ROOT, "solver")
    lp = os.path.join(ROOT, "tests", "golden", "sample.txt")
    prefix = str(tmp_path / "r")
    r = subprocess.run([solver, "--ranging", prefix, lp], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--ranging" in r.stderr and "--dual" in r.stderr and "--primal-box" in r.stderr
    assert not os.path.exists(prefix + ".cost.txt") and not os.path.exists(prefix + ".rhs.txt")
    r = subprocess.run([solver, "--dual", lp, "--ranging"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr  # the option without its argument


# ---------------------------------------------------------------------------------------------------------------------
# brute force

def _optimum(kind, m, n, seed):
    A, b, c, l, u = rr.build_lp(kind, m, n, seed)
    bix, up, Binv, y, xs, rng, fr = rr.solve_numpy(kind, A, b, c, l, u)
    cost, rhs = rr.both(A, c, bix, up, Binv, y, xs, rng, fr)
    return A, c, bix, up, Binv, xs, rng, fr, cost, rhs


@pytest.mark.parametrize("kind,m,n,seed", [("primal", 7, 20, 0), ("primal", 65, 200, 1), ("dual", 7, 20, 0),
                                           ("dual", 65, 200, 1), ("lu", 65, 200, 1)])
def test_cost_ranges_against_brute_force(kind, m, n, seed):
    """c_j moved to 0.999 of a finite limit: every non-basic sigma_k d_k stays >=
    0; to 1.001: the reported blocker's turns negative.  d is recomputed from
    scratch (y = c_B B^-1) each time."""
    A, c, bix, up, Binv, _, _, fr, cost, _ = _optimum(kind, m, n, seed)
    basic = cost.row_of >= 0
    sig = cost.sigma
    cols = range(n) if m == 7 else list(range(0, n, 5)) + [int(j) for j in bix[::4]]
    probes = 0
    for j in cols:
        for sign, lim, blk in ((-1.0, cost.down[j], cost.block_down[j]), (1.0, cost.up[j], cost.block_up[j])):
            if not np.isfinite(lim):
                assert blk == -1
                continue
            assert lim >= 0.0 and blk >= 0 and not basic[blk]
            if lim <= 1e-6:
                continue
            probes += 1
            for f, inside in ((0.999, True), (1.001, False)):
                c2 = c.copy()
                c2[j] += sign * f * lim
                d2 = (c2[bix] @ Binv) @ A - c2
                sd = np.where(basic | fr, 0.0, sig * d2)
                if inside:
                    assert sd.min() >= -1e-12, (j, sign, sd.min())
                else:
                    assert sig[blk] * d2[blk] < 0.0, (j, sign, blk, sig[blk] * d2[blk])
                    # nothing else gives way first: the blocker's is the ratio that was minimal
                    assert np.sum(sd < -1e-12) >= 1
    print(f"{kind} {m}x{n}: {probes} finite cost limits probed on both sides")
    assert probes >= (10 if m == 7 else 40)


@pytest.mark.parametrize("kind,m,n,seed", [("primal", 7, 20, 0), ("primal", 65, 200, 1), ("dual", 7, 20, 0),
                                           ("dual", 65, 200, 1), ("lu", 65, 200, 1)])
def test_rhs_ranges_against_brute_force(kind, m, n, seed):
    """b_r moved to 0.999 of a finite limit: 0 <= x_b <= ub_B still holds; to
    1.001: the reported row is past the reported bound."""
    _, _, bix, _, Binv, xs, rng, fr, _, rhs = _optimum(kind, m, n, seed)
    ub = rng[bix]
    frB = fr[bix]
    probes = 0
    for r in (range(m) if m == 7 else range(0, m, 2)):
        for sign, lim, key in ((-1.0, rhs.down[r], rhs.leave_down[r]), (1.0, rhs.up[r], rhs.leave_up[r])):
            if not np.isfinite(lim):
                assert key == -1
                continue
            i, side = int(key) // 2, int(key) % 2
            assert lim >= 0.0 and 0 <= i < m and not frB[i]
            if lim <= 1e-6:
                continue
            probes += 1
            for f, inside in ((0.999, True), (1.001, False)):
                x2 = rhs.x + sign * f * lim * Binv[:, r]
                if inside:
                    assert np.all(frB | ((x2 >= -1e-12) & (x2 <= ub + 1e-12))), (r, sign)
                elif side:
                    assert x2[i] > ub[i], (r, sign, i, x2[i], ub[i])
                else:
                    assert x2[i] < 0.0, (r, sign, i, x2[i])
    print(f"{kind} {m}x{n}: {probes} finite right-hand-side limits probed on both sides")
    assert probes >= (6 if m == 7 else 20)


def test_exact_tie_goes_to_the_smaller_column():
    A, b, c, u, basis = rr.tiny_tie()
    Binv = np.linalg.inv(A[:, basis])
    y = c[basis] @ Binv
    cost = rr.cost_ranging(A, c, basis, np.zeros(5, dtype=bool), Binv, y)
    assert np.array_equal(cost.T[:, :2], np.ones((2, 2)))  # columns 1 and 2: the same entry in every row
    assert cost.down[0] == 2.0 and cost.down[4] == 2.0
    assert cost.block_down[0] == 1 and cost.block_down[4] == 1  # not 2
    assert cost.second_down[0] == 2.0 and cost.second_down[4] == 2.0  # the tie is exact
    assert np.isinf(cost.up[0]) and cost.block_up[0] == -1
    # the non-basic columns: at lower, up = d_j, blocked by themselves
    assert cost.up[1:4].tolist() == [2.0, 2.0, 3.0] and cost.block_up[1:4].tolist() == [1, 2, 3]
    assert np.all(np.isinf(cost.down[1:4])) and cost.block_down[1:4].tolist() == [-1, -1, -1]
    rhs = rr.rhs_ranging(Binv, Binv @ b, u[basis])
    # b_0: x0 = 4 falls to 0 at -4; b_1: s1 = 5 falls to 0 at -5; nothing blocks upwards
    assert rhs.down.tolist() == [4.0, 5.0] and rhs.leave_down.tolist() == [0, 2]
    assert np.all(np.isinf(rhs.up)) and rhs.leave_up.tolist() == [-1, -1]


def test_free_nonbasic_column_blocks_both_ways():
    A, b, c, l, u, basis = rr.tiny_free()
    fr = np.isneginf(l)
    Binv = np.linalg.inv(A[:, basis])
    y = c[basis] @ Binv
    cost = rr.cost_ranging(A, c, basis, np.zeros(6, dtype=bool), Binv, y, free=fr)
    assert cost.d[3] == 0.0
    for j in basis:
        assert cost.down[j] == 0.0 and cost.up[j] == 0.0 and cost.block_down[j] == 3 and cost.block_up[j] == 3
    assert cost.down[3] == 0.0 and cost.up[3] == 0.0 and cost.block_down[3] == 3 and cost.block_up[3] == 3
    # a free basic column's row never blocks a right-hand side
    rhs = rr.rhs_ranging(Binv, Binv @ b, u[basis], free_B=np.array([True, False]))
    assert np.isinf(rhs.down[0]) and rhs.down[1] == 5.0 and rhs.leave_down.tolist() == [-1, 2]


@pytest.mark.parametrize("kind,m,n,seed", rr.CASES)
def test_gpu_cases_pass_the_case_builder(kind, m, n, seed):
    """No entry of T or B^-1 near the tolerance, at most 5 % of the rows or
    columns under the runner-up exemption, at the numpy loop's optimum (the
    GPU tests check the device's optimum again)."""
    A, b, c, l, u = rr.build_lp(kind, m, n, seed)
    bix, up, Binv, y, xs, rng, fr = rr.solve_numpy(kind, A, b, c, l, u)
    cost, rhs = rr.both(A, c, bix, up, Binv, y, xs, rng, fr)
    assert rr.refuse_case(cost, rhs, Binv) == []
    # the refusals do refuse: an entry of B^-1 moved to the tolerance
    B2 = Binv.copy()
    B2[0, 0] = 1e-9
    assert any("B^-1" in w for w in rr.refuse_case(cost, rhs, B2))
