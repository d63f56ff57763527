"""CPU: bound ranging and the objective at the range ends (spx_ranging_bound,
spx_ranging_objective, spx_ranging_bound_times).  The additions
to the C-ABI, the Python package and the CLI that need no device, and the numpy
restatement (tests/bound_ranging_ref.py) itself: against brute force (move one
bound to 0.999 and 1.001 of every sampled finite limit and look at x_B(t)), on
hand-made LPs (an exact tie of two rows, an own bound tying a row, a free
non-basic column and a free basic row, a fixed column), and the GPU tests'
cases against the case builder's refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

import bound_ranging_ref as br
import ranging_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "simplex.h")
NEW_FUNCTIONS = ("spx_ranging_bound", "spx_ranging_objective", "spx_ranging_bound_times")


def test_header_prototypes():
    txt = open(HEADER).read()
    assert re.search(r"#define\s+SPX_ABI_VERSION\s+8\b", txt)
    assert re.search(r"#define\s+SPX_RANGING_OWN_BOUND\s+\(-2\)", txt)
    for k, name in enumerate(("COST", "RHS", "BOUND")):
        assert re.search(rf"#define\s+SPX_RANGING_{name}\s+{k}\b", txt)
    assert re.search(r"int\s+spx_ranging_bound\(spx_ctx\*\s*ctx,\s*double\*\s*down,\s*double\*\s*up,\s*int64_t\*\s*"
                     r"leave_down,\s*int64_t\*\s*leave_up\);", txt)
    assert re.search(r"int\s+spx_ranging_objective\(spx_ctx\*\s*ctx,\s*int32_t\s+what,\s*const\s+double\*\s*down,\s*"
                     r"const\s+double\*\s*up,\s*double\*\s*obj_down,\s*double\*\s*obj_up\);", txt)
    assert re.search(r"int\s+spx_ranging_bound_times\(spx_ctx\*\s*ctx,\s*double\*\s*ms,\s*int64_t\*\s*launches\);", txt)
    # spx_ranging_times keeps its two slots
    assert re.search(r"int\s+spx_ranging_times\(spx_ctx\*\s*ctx,\s*double\s+ms\[2\],\s*int64_t\s+launches\[2\]\);", txt)
    for name in NEW_FUNCTIONS:
        assert not re.search(r"\d", name)


def test_binding_and_package(spx):
    L = spx._lib.load()
    assert L.spx_abi_version() == 8
    for name in NEW_FUNCTIONS:
        assert name in spx._lib.SIGNATURES and name not in spx._lib.SIGNATURES_NUMBERED and hasattr(L, name), name
    for name in ("bound_ranging", "ranging_objective", "bound_ranging_times"):
        assert callable(getattr(spx.Context, name)), name
    assert spx.BoundRanging._fields == ("down", "up", "leave_down", "leave_up")
    assert spx.RangeEnds._fields == ("down", "up")
    assert spx.RANGING_OWN_BOUND == br.OWN == -2
    for name in ("BoundRanging", "RangeEnds", "RANGING_OWN_BOUND"):
        assert name in spx.__all__
    # NULL contexts and result arrays are refused before anything touches a device
    assert L.spx_ranging_bound(None, None, None, None, None) == -1
    assert L.spx_ranging_objective(None, 2, None, None, None, None) == -1
    assert L.spx_ranging_bound_times(None, None, None) == -1


def test_cli_refuses_bound_ranging_without_a_bounded_loop(tmp_path):
    solver = os.path.join(ROOT, "solver")
    lp = os.path.join(ROOT, "tests", "golden", "sample.txt")
    prefix = str(tmp_path / "r")
    r = subprocess.run([solver, "--bound-ranging", prefix, lp], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--bound-ranging" in r.stderr and "--dual" in r.stderr and "--primal-box" in r.stderr
    assert not os.path.exists(prefix + ".bound.txt")
    r = subprocess.run([solver, "--dual", lp, "--bound-ranging"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr  # the option without its argument


# ---------------------------------------------------------------------------------------------------------------------
# brute force

_OPT = {}


def _optimum(kind, m, n, seed):
    k = (kind, m, n, seed)
    if k not in _OPT:
        A, b, c, l, u = rr.build_lp(kind, m, n, seed)
        bix, up, Binv, y, xs, rng, fr = rr.solve_numpy(kind, A, b, c, l, u)
        bix = np.asarray(bix, dtype=np.int64)
        ref = br.bound_ranging(A, bix, up, Binv, xs, rng, free=fr)
        _OPT[k] = (A, c, bix, np.asarray(up, dtype=bool), Binv, y, xs, rng, fr, ref)
    return _OPT[k]


@pytest.mark.parametrize("kind,m,n,seed", [("primal", 7, 20, 0), ("primal", 65, 200, 1), ("dual", 7, 20, 0),
                                           ("dual", 65, 200, 1), ("lu", 65, 200, 1)])
def test_bound_ranges_against_brute_force(kind, m, n, seed):
    """A non-basic column's bound moved by 0.999 of a finite limit: 0 <= x_B(t) <=
    ub_B still holds in every row that is not free; by 1.001: the reported row is
    past the reported bound, or (own bound) the moved bound has crossed the other
    one, l > u.  A basic column's bound moved by 0.999 of its slack stays on its
    side of x_i; by 1.001 it has passed it."""
    A, _, bix, upb, Binv, _, _, rng, fr, ref = _optimum(kind, m, n, seed)
    ub = rng[bix]
    frB = fr[bix]
    probes = own = 0
    cols = range(n) if m == 7 else list(range(0, n, 3)) + [int(j) for j in bix[::4]]
    for j in cols:
        i = ref.row_of[j]
        for sign, lim, key in ((-1.0, ref.down[j], ref.leave_down[j]), (1.0, ref.up[j], ref.leave_up[j])):
            if not np.isfinite(lim):
                assert key == -1
                continue
            assert lim >= 0.0 and key != -1
            if i >= 0:  # basic: its own slacks
                assert key == 2 * i + (0 if sign > 0 else 1) and not (sign > 0 and frB[i])
                gap = ref.x[i] if sign > 0 else ub[i] - ref.x[i]
                assert lim == gap and 0.999 * lim <= gap and (lim == 0.0 or 1.001 * lim > gap)
                continue
            assert ref.kind[j] in (0, 1)
            alpha = Binv @ A[:, j]
            if lim <= 1e-6:
                continue
            probes += 1
            for f, inside in ((0.999, True), (1.001, False)):
                t = sign * f * lim
                x2 = ref.x - t * alpha
                if inside:
                    assert np.all(frB | ((x2 >= -1e-12) & (x2 <= ub + 1e-12))), (j, sign)
                    assert abs(t) <= rng[j] or (ref.kind[j] == 0) != (sign > 0)
                elif key == br.OWN:
                    # at lower the lower bound rose past the upper one; at upper the upper one fell past the lower
                    assert (ref.kind[j] == 0) == (sign > 0) and lim == rng[j] and abs(t) > rng[j]
                    own += 1
                else:
                    r, side = int(key) // 2, int(key) % 2
                    assert 0 <= r < m and not frB[r]
                    if side:
                        assert x2[r] > ub[r], (j, sign, r, x2[r], ub[r])
                    else:
                        assert x2[r] < 0.0, (j, sign, r, x2[r])
    print(f"{kind} {m}x{n}: {probes} finite bound limits of non-basic columns probed on both sides, {own} own-bound caps")
    assert probes >= (6 if m == 7 else 40)


def _tiny(A, b, c, u, basis, up=None, free=None):
    A = np.asarray(A)
    n = A.shape[1]
    Binv = np.linalg.inv(A[:, basis])
    up = np.zeros(n, dtype=bool) if up is None else up
    xb = Binv @ (b - A[:, up] @ u[up])
    return br.bound_ranging(A, basis, up, Binv, xb, u, free=free)


def test_exact_tie_of_two_rows_goes_to_the_smaller_key():
    A, b, c, u, basis = br.tie_rows()
    ref = _tiny(A, b, c, u, basis)
    assert np.array_equal(ref.T[:, 0], [1.0, 1.0]) and ref.x.tolist() == [4.0, 4.0]
    assert ref.up[2] == 4.0 and ref.leave_up[2] == 0 and ref.second_up[2] == 4.0  # row 0 side 0, not row 1 (key 2)
    assert np.isinf(ref.down[2]) and ref.leave_down[2] == -1
    # the non-basic slacks against right-hand-side ranging: up = rhs.down, down = rhs.up
    rhs = rr.rhs_ranging(np.linalg.inv(A[:, basis]), ref.x, u[basis])
    for r in range(2):
        j = 3 + r
        assert ref.up[j] == rhs.down[r] and ref.leave_up[j] == rhs.leave_down[r]
        assert ref.down[j] == rhs.up[r] and ref.leave_down[j] == rhs.leave_up[r]
    # the basic columns: their own slacks
    assert ref.up[:2].tolist() == [4.0, 4.0] and ref.leave_up[:2].tolist() == [0, 2]
    assert np.all(np.isinf(ref.down[:2])) and ref.leave_down[:2].tolist() == [-1, -1]


def test_exact_tie_of_two_far_rows():
    A, b, c, u, basis = br.tie_rows_far()
    ref = _tiny(A, b, c, u, basis)
    assert ref.up[6] == 4.0 and ref.leave_up[6] == 2 and ref.second_up[6] == 4.0  # row 1, not row 4 (key 8)
    y = c[basis] @ np.linalg.inv(A[:, basis])
    assert np.all((y @ A - c)[6:] >= 0.0)  # the basis is optimal


def test_own_bound_tying_a_row_reports_the_row():
    A, b, c, u, basis = br.tie_own()
    ref = _tiny(A, b, c, u, basis)
    assert ref.up[2] == 4.0 and ref.leave_up[2] == 0  # the own bound 4 ties the rows' 4: the row
    u3 = u.copy()
    u3[2] = 3.0
    ref = _tiny(A, b, c, u3, basis)
    assert ref.up[2] == 3.0 and ref.leave_up[2] == br.OWN and ref.second_up[2] == 4.0
    # the same column at its upper bound 3: x_B = (1, 1); down is capped by the own bound (3 < +inf: nothing else
    # blocks downwards, alpha > 0 and no upper bound on a basic column), up is blocked by the rows at 1
    upp = np.zeros(5, dtype=bool)
    upp[2] = True
    ref = _tiny(A, b, c, u3, basis, up=upp)
    assert ref.x.tolist() == [1.0, 1.0]
    assert ref.down[2] == 3.0 and ref.leave_down[2] == br.OWN and ref.up[2] == 1.0 and ref.leave_up[2] == 0


def test_fixed_nonbasic_column_follows_the_same_rule():
    A, b, c, u, basis = br.tie_rows()
    u0 = u.copy()
    u0[2] = 0.0
    ref = _tiny(A, b, c, u0, basis)
    assert ref.up[2] == 0.0 and ref.leave_up[2] == br.OWN  # 0 < 4: strictly smaller
    assert np.isinf(ref.down[2]) and ref.leave_down[2] == -1
    # where a row's ratio is 0 too, the row is reported
    ref = _tiny(A, np.array([0.0, 4.0]), c, u0, basis)
    assert ref.up[2] == 0.0 and ref.leave_up[2] == 0


def test_free_column_and_free_row():
    A, b, c, l, u, basis = rr.tiny_free()
    fr = np.isneginf(l)
    Binv = np.linalg.inv(A[:, basis])
    ref = br.bound_ranging(A, basis, np.zeros(6, dtype=bool), Binv, Binv @ b, u, free=fr)
    assert np.isinf(ref.down[3]) and np.isinf(ref.up[3]) and ref.leave_down[3] == -1 and ref.leave_up[3] == -1
    # column 1, alpha = (1, 1) against x_B = (4, 5): row 0 blocks at 4
    assert ref.up[1] == 4.0 and ref.leave_up[1] == 0
    # the same LP with the basic column 0 declared free: its row never blocks, row 1 does at 5; and its own lower
    # bound has nothing to move
    fr0 = fr.copy()
    fr0[0] = True
    ref = br.bound_ranging(A, basis, np.zeros(6, dtype=bool), Binv, Binv @ b, u, free=fr0)
    assert ref.up[1] == 5.0 and ref.leave_up[1] == 2
    assert np.isinf(ref.up[0]) and ref.leave_up[0] == -1 and np.isinf(ref.down[0]) and ref.leave_down[0] == -1


def test_objective_ends_rule():
    inf = np.inf
    od, ou = br.objective_ends("cost", 10.0, [1.0, inf, inf], [2.0, inf, 3.0], [3.0, 0.0, -1.0])
    assert od.tolist() == [7.0, 10.0, inf] and ou.tolist() == [16.0, 10.0, 7.0]
    od, ou = br.objective_ends("bound", 10.0, [1.0, inf, 2.0], [2.0, inf, 1.0], [3.0, 0.0, 5.0], moves=[True, True, False])
    assert od.tolist() == [13.0, 10.0, 10.0] and ou.tolist() == [4.0, 10.0, 10.0]


@pytest.mark.parametrize("kind,m,n,seed", rr.CASES)
def test_gpu_cases_pass_the_case_builder(kind, m, n, seed):
    """No entry of T near the tolerance and no non-basic column under the
    runner-up exemption at the numpy loop's optimum (the GPU tests check the
    device's optimum again); every case has blockers with side 1, own-bound
    winners or both and non-basic columns at upper, and a zero range only
    where a fixed column meets its own bound."""
    A, _, bix, upb, Binv, _, _, rng, fr, ref = _optimum(kind, m, n, seed)
    assert br.refuse_case(ref) == []
    assert len(br.exempt_columns(ref)) == 0
    nb = ref.nb[ref.kind[ref.nb] != 2]
    keys = np.concatenate([ref.leave_down[nb], ref.leave_up[nb]])
    side1 = int(np.sum((keys >= 0) & (keys % 2 == 1)))
    nown = int(np.sum(keys == br.OWN))
    nup = int(np.sum(ref.kind == 1))
    print(f"{kind} {m}x{n}: {side1} blockers with side 1, {nown} own-bound winners, {nup} non-basic columns at upper")
    assert nup > 0 and side1 + nown > 0 and (m == 7 or side1 > 0)
    zero = (ref.up[nb] == 0.0) | (ref.down[nb] == 0.0)  # only a fixed column's own bound (general_lu has some)
    assert np.all(rng[nb[zero]] == 0.0)
    # the refusals do refuse: an entry of T moved to the tolerance
    T2 = ref.T.copy()
    T2[0, 0] = 1e-9
    ref.T, keep = T2, ref.T
    assert any("T within" in w for w in br.refuse_case(ref))
    ref.T = keep
