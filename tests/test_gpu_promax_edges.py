"""The Promax passes and the loop hand-overs of the fused rotation routes (csrc/rotate.h rot_accum_kernel MODE 2 / 3,
rot_reduce_partials_kernel; csrc/solver.h Rotator::run) at the shapes where they can go wrong: fewer points than a tile and
tile tails, every position of the n_left split, up to 16 (j,k) entries per thread, grids long enough for 2048 partials, the
per-iteration route from iteration 0 and the hand-over of the resident-tile and two-stage persistent loops.  Every call goes
through the C ABI (xmca_rotate_loadings); the reference is oracle/ref_numpy.py, the inputs are oracle/promax_edges.py.

Tolerances:
  TOL = 1e-7 relative (max-norm over the max of the reference) for the full path, as in test_gpu_rotation.py - the device
        follows the same trajectory and stops at the same iteration, the last iterate moves by ~sqrt(tol).
  tail bound (sections 2 and 3): the Promax tail recomputed from the device's own Varimax result leaves only the rounding of
        the tail itself.  The reference's own noise - the tail in float64 against the tail with its N-sized sums and column
        maxima in np.longdouble - is at most 1.23e-14 over the cases (131200 x 6; 4e-16 .. 5e-15 elsewhere, cond(X^H X) 1.0 .. 3.2,
        profiles/promax_tail_accuracy.json, scripts/promax_tail_accuracy.py); the device may deviate by 100 x that
        (1.23e-12: another summation order, up to 2048 partials in two levels), never by less than 1e-13 nor more than 1e-10.
        Largest device deviation measured on an MI355X (`scripts/promax_tail_accuracy.py --device`, same file): 1.27e-14
        (131200 x 6), 3e-16 .. 5e-15 for the other cases - about 1 % of the bound.

That the tests bite was checked with three edits on scratch copies of csrc/rotate.h (each caught by this file alone):
  * `sc` of MODE 2 / 3 without its `n < N` guard: NaN in X^H X wherever N is no multiple of 64 - every test that runs Promax at
    such an N fails ("X^H X is singular"): 10 cases of section 1, 10 of section 2, all of section 3, the wide hand-over.
  * SEL 3 with `n > Nleft` for `n >= Nleft`: norm_right loses the row n_left - sections 1 and 2 fail for every case with a
    right block (norm_right is 0 where that block is one point: relative error 1.0), split additivity fails by 1e-6 at
    N = 70000, and the row permutation fails.
  * rot_reduce_partials_kernel without the last stride when nwg > 256: the three long-grid cases fail sections 1 and 2 (wrong
    iteration count or no convergence, since A0 and the moments take the same sum; B off by 4e-3 in the tail comparison of
    66000 x 14), and every section-3 test of 70000 x 4 fails; all shorter grids pass.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import promax_edges as E

pytestmark = pytest.mark.gpu
TOL = 1e-7
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = E.CASES
IDS = [E.case_id(c) for c in CASES]
MOMENT = CASES[9]           # 70000 x 4 real: fourth-moment route, long grid, last tile of 48 points
NARROW = CASES[4]           # 65 x 17 real: persistent loop on the narrow grid, one point in the second tile
WIDE = CASES[5]             # 200 x 24 complex: persistent loop on the wide grid, last tile of 8 points
PROPERTY_CASES = [MOMENT, NARROW, WIDE]
PROPERTY_IDS = [E.case_id(c) for c in PROPERTY_CASES]
LONG_CASES = [CASES[9], CASES[10], CASES[11]]

_oracle, _device, _varimax = {}, {}, {}


def oracle_of(case, gen=E.edge_loadings):
    """float64 oracle of a case, computed once (never modified by a test)"""
    if case not in _oracle:
        _oracle[case] = E.oracle_case(case, gen)
    return _oracle[case]


def device_of(hip, case, gen=E.edge_loadings):
    """the full device call of a case (Varimax + Promax, B fetched), run once"""
    if case not in _device:
        n, p, cplx, power, n_left, _ = case
        _device[case] = hip.rotate_loadings(oracle_of(case, gen)["A"], n_left, power, tol=E.TOL_STOP, want_B=True)
    return _device[case]


def varimax_of(hip, case):
    if case not in _varimax:
        _varimax[case] = hip.rotate_loadings(oracle_of(case)["A"], case[4], varimax_only=True, want_B=True)
    return _varimax[case]


@pytest.fixture(scope="module")
def tail_bound():
    """100 x the reference's own noise over all cases, from the oracle's Varimax result (no device involved)"""
    worst = 0.0
    for case in CASES:
        ref = oracle_of(case)
        noise, cond = E.tail_noise(ref["Bv"], ref["Rv"], case[3], case[4])
        worst = max(worst, noise)
    bound = E.tail_bound(worst)
    print("reference noise of the Promax tail %.3e -> device bound %s" % (worst, bound))
    assert bound is not None, "a case is too ill-conditioned for the tail comparison: noise %.3e" % worst
    return bound


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("R", "Phi", "B", "norm_left", "norm_right")) and a["n_iter"] == b["n_iter"]


# ----------------------------------------------------------------------------------------------
# 1. full path against the float64 oracle
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_promax_edge_shapes_match_the_oracle(hip, case):
    """Same iteration count, R / Phi / B and both block norms at TOL; an empty block has norm exactly 0.  The oracle's stop
    must not be decided in the last digits: ratio <= 0.7 tol at the stop, >= 1.3 tol one iteration earlier."""
    n, p, cplx, power, n_left, _ = case
    ref = oracle_of(case)
    at, before = E.stop_margin(ref["ratios"])
    print("oracle: %d iterations, stopping ratio %.3f tol at the stop, %.3f tol before" % (ref["n_iter"], at, before))
    assert at <= E.STOP_BELOW and before >= E.STOP_ABOVE
    out = device_of(hip, case)
    errs = {k: E.rel(out[k], ref[k]) for k in ("R", "Phi", "B", "norm_left", "norm_right")}
    print("device: %d iterations, %s" % (out["n_iter"], errs))
    assert out["n_iter"] == ref["n_iter"]
    for k, e in errs.items():
        assert e < TOL, (k, e)
    if n_left == 0:
        assert np.all(out["norm_left"] == 0.0)
    if n_left == n:
        assert np.all(out["norm_right"] == 0.0)


# ----------------------------------------------------------------------------------------------
# 2. the Promax tail alone
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_promax_tail_from_the_device_varimax_result(hip, tail_bound, case):
    """The tail of ref_numpy.promax (behind its Varimax call) recomputed in float64 from the device's own Varimax loadings
    and rotation: R (= R_v L), Phi, B and the block norms of the full device call agree to the tail bound of the module
    docstring - the 1e-7 of the trajectory is gone, a padding point that enters one sum is not."""
    n, p, cplx, power, n_left, _ = case
    full = device_of(hip, case)
    v = varimax_of(hip, case)
    assert v["n_iter"] == full["n_iter"]
    assert np.array_equal(v["Phi"], np.eye(p))
    B, R, Phi, nl, nr, cond = E.promax_tail(v["B"], v["R"], power, n_left)
    ref = {"B": B, "R": R, "Phi": Phi, "norm_left": nl, "norm_right": nr}
    errs = {k: E.rel(full[k], ref[k]) for k in E.TAIL_NAMES}
    print("tail: cond(X^H X) %.2f, bound %.3e, %s" % (cond, tail_bound, errs))
    for k, e in errs.items():
        assert e < tail_bound, (k, e)
    assert np.all(np.isfinite(full["B"])) and np.all(np.isfinite(full["Phi"]))


# ----------------------------------------------------------------------------------------------
# 3. properties that need no oracle
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PROPERTY_CASES, ids=PROPERTY_IDS)
def test_split_additivity_and_independence_of_the_split(hip, case):
    """norm_left^2 + norm_right^2 = column norms^2 of B for every position of the split (empty blocks, one point, around a
    tile boundary, inside the last tile); the split enters nothing else: R, Phi, B keep their bits."""
    n, p, cplx, power, _, _ = case
    A = oracle_of(case)["A"]
    first = None
    for n_left in sorted({0, 1, 63, 64, 65, n - 1, n}):
        out = hip.rotate_loadings(A, n_left, power, tol=E.TOL_STOP, want_B=True)
        total = np.sum(np.abs(out["B"]) ** 2, axis=0)
        e = E.rel(out["norm_left"] ** 2 + out["norm_right"] ** 2, total)
        print("n_left %d: additivity %.3e" % (n_left, e))
        assert e < 1e-12, (n_left, e)
        if n_left == 0:
            assert np.all(out["norm_left"] == 0.0)
        if n_left == n:
            assert np.all(out["norm_right"] == 0.0)
        if first is None:
            first = out
        for k in ("R", "Phi", "B"):
            assert np.array_equal(out[k], first[k]), (n_left, k)
        assert out["n_iter"] == first["n_iter"]


@pytest.mark.parametrize("case", PROPERTY_CASES, ids=PROPERTY_IDS)
def test_row_permutation_inside_the_blocks(hip, tail_bound, case):
    """Rows permuted within the left and within the right block: Phi and both block norms are sums over the rows of a block
    and do not move (tail bound) - a tile or padding slot dropped or counted twice would show, at any N."""
    n, p, cplx, power, n_left, seed = case
    A = oracle_of(case)["A"]
    rng = np.random.default_rng(seed + 1000)
    perm = np.concatenate([rng.permutation(n_left), n_left + rng.permutation(n - n_left)])
    base = device_of(hip, case)
    out = hip.rotate_loadings(np.ascontiguousarray(A[perm]), n_left, power, tol=E.TOL_STOP, want_B=True)
    assert out["n_iter"] == base["n_iter"]
    errs = {k: E.rel(out[k], base[k]) for k in ("Phi", "norm_left", "norm_right")}
    print("permuted rows: bound %.3e, %s" % (tail_bound, errs))
    for k, e in errs.items():
        assert e < tail_bound, (k, e)


@pytest.mark.parametrize("case", PROPERTY_CASES + LONG_CASES[1:], ids=PROPERTY_IDS + [E.case_id(c) for c in LONG_CASES[1:]])
def test_promax_gives_the_same_bits_twice(hip, case):
    """The partials are summed in a fixed order and the maximum does not depend on the order of the atomics: same bits in
    every output, long grids (more than 256 partials, strided first level of the sum) included."""
    n, p, cplx, power, n_left, _ = case
    first = device_of(hip, case)
    again = hip.rotate_loadings(oracle_of(case)["A"], n_left, power, tol=E.TOL_STOP, want_B=True)
    assert _same_bits(first, again)


@pytest.mark.parametrize("case", PROPERTY_CASES, ids=PROPERTY_IDS)
def test_power_one_is_varimax(hip, tail_bound, case):
    """power = 1: the target equals X, so L is diagonal and is scaled to the identity - Phi = I, R stays unitary."""
    n, p, cplx, _, n_left, _ = case
    out = hip.rotate_loadings(oracle_of(case)["A"], n_left, 1, tol=E.TOL_STOP, want_B=True)
    e_phi = E.rel(out["Phi"], np.eye(p))
    e_r = E.rel(out["R"].conj().T @ out["R"], np.eye(p))
    v = varimax_of(hip, case)
    e_v = E.rel(out["R"], v["R"])
    print("power 1: Phi - I %.3e, R^H R - I %.3e, R - R_varimax %.3e (bound %.3e)" % (e_phi, e_r, e_v, tail_bound))
    assert e_phi < tail_bound and e_r < tail_bound and e_v < tail_bound
    assert out["n_iter"] == v["n_iter"]


# ----------------------------------------------------------------------------------------------
# 4. the loops that nothing enters from the start
# ----------------------------------------------------------------------------------------------
PER_ITERATION_CASES = [(WIDE, E.edge_loadings), (CASES[6], E.edge_loadings), (E.SLOW_CASE, E.wide_loadings)]

CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oracle import promax_edges as E
from xmca_amd import _hip
h = _hip.default_handle(0)
g0 = _hip.load_library().xmca_persistent_giveups()
out = {}
for i, (case, gen) in enumerate([(E.CASES[5], E.edge_loadings), (E.CASES[6], E.edge_loadings), (E.SLOW_CASE, E.wide_loadings)]):
    n, p, cplx, power, n_left, seed = case
    r = h.rotate_loadings(gen(n, p, cplx, seed), n_left, power, tol=E.TOL_STOP, want_B=True)
    for k in ("R", "Phi", "B", "norm_left", "norm_right"):
        out["%d_%s" % (i, k)] = r[k]
    out["%d_n_iter" % i] = np.int64(r["n_iter"])
out["giveups"] = np.int64(_hip.load_library().xmca_persistent_giveups() - g0)
np.savez(sys.argv[2], **out)
"""


def test_per_iteration_route_from_iteration_zero(hip, tmp_path):
    """XMCA_VARIMAX_PERSIST=0 (read once per process, hence one fresh child): the route of a partitioned or CU-masked device.
    One launch per iteration from iteration 0 in batches of 32, the arrival ticket carried from batch to batch; the third input
    needs 42 iterations, so the loop crosses a batch boundary and stops inside the next batch (the child's XMCA_TRACE=rot lines,
    which only per_iteration_loop prints, show both batches).  Oracle's iteration count, TOL against the oracle, 1e-9 against the
    persistent loop of this process."""
    assert PER_ITERATION_CASES[0][0] == E.CASES[5] and PER_ITERATION_CASES[1][0] == E.CASES[6]
    refs = [oracle_of(case, gen) for case, gen in PER_ITERATION_CASES]
    assert 32 < refs[2]["n_iter"] < 64
    for ref in refs:
        assert E.stop_is_clear(ref["ratios"]), E.stop_margin(ref["ratios"])
    t0 = time.perf_counter()
    mine = [hip.rotate_loadings(ref["A"], case[4], case[3], tol=E.TOL_STOP, want_B=True) for (case, _), ref in zip(PER_ITERATION_CASES, refs)]
    in_process = time.perf_counter() - t0
    # interpreter, numpy, library load and device initialisation (tens of seconds at worst on a busy machine) + the three calls
    limit = min(90.0 + 10.0 * in_process, 119.0)
    dst = str(tmp_path / "per_iteration.npz")
    env = dict(os.environ, XMCA_VARIMAX_PERSIST="0", XMCA_TRACE="rot")
    env.pop("XMCA_VARIMAX_TEST_GIVEUP", None)
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, dst], env=env, capture_output=True, text=True, timeout=limit)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(dst)
    assert int(got["giveups"]) == 0                       # the persistent loop was never entered
    # only per_iteration_loop prints these lines (XMCA_TRACE=rot), one per batch of 32 launches: the first two inputs stop inside
    # the first batch, the third is not converged after it (32 iterations done) and stops inside the second
    trace = [ln for ln in r.stderr.splitlines() if ln.startswith("[xmca varimax] ")]
    want = []
    for (case, _), ref in zip(PER_ITERATION_CASES, refs):
        head = "[xmca varimax] p=%d N=%d cplx=%d " % (case[1], case[0], int(case[2]))
        if ref["n_iter"] > 32:
            want.append(head + "launched=32 iter=32 conv=0 ")
            want.append(head + "launched=64 iter=%d conv=1 " % ref["n_iter"])
        else:
            want.append(head + "launched=32 iter=%d conv=1 " % ref["n_iter"])
    assert len(trace) == len(want), r.stderr[-2000:]
    for line, start in zip(trace, want):
        assert line.startswith(start), (line, start)
    for i, (ref, own) in enumerate(zip(refs, mine)):
        assert int(got["%d_n_iter" % i]) == ref["n_iter"] == own["n_iter"]
        for k in ("R", "Phi", "B", "norm_left", "norm_right"):
            e_ref, e_own = E.rel(got["%d_%s" % (i, k)], ref[k]), E.rel(got["%d_%s" % (i, k)], own[k])
            print("input %d %s: %.3e against the oracle, %.3e against the persistent loop" % (i, k, e_ref, e_own))
            assert e_ref < TOL and e_own < 1e-9, (i, k, e_ref, e_own)


def _giveups():
    from xmca_amd import _hip
    return int(_hip.load_library().xmca_persistent_giveups())


def test_hand_over_from_the_wide_persistent_loop(hip, monkeypatch):
    """200 x 24 complex (wide grid, resident tiles): the persistent launch stopped after 7 of its 11 iterations, the
    per-iteration launches finish - same stop iteration, R / Phi / B within 1e-9, one give-up counted."""
    n, p, cplx, power, n_left, _ = WIDE
    A = oracle_of(WIDE)["A"]
    whole = device_of(hip, WIDE)
    assert whole["n_iter"] > 7
    g0 = _giveups()
    monkeypatch.setenv("XMCA_VARIMAX_TEST_GIVEUP", "7")
    cut = hip.rotate_loadings(A, n_left, power, tol=E.TOL_STOP, want_B=True)
    assert _giveups() == g0 + 1
    monkeypatch.delenv("XMCA_VARIMAX_TEST_GIVEUP")
    assert cut["n_iter"] == whole["n_iter"]
    for k in ("R", "Phi", "B", "norm_left", "norm_right"):
        assert E.rel(cut[k], whole[k]) < 1e-9, k
    hip.rotate_loadings(A, n_left, power, tol=E.TOL_STOP)
    assert _giveups() == g0 + 1                          # ... and none without the interruption


def test_hand_over_from_the_two_stage_persistent_loop(hip, monkeypatch):
    """12000 x 32 complex, Varimax only (the two-stage input of test_varimax_wide_grid_and_two_stage_sum): the same hand-over
    where the partial G matrices are summed in two stages."""
    A = E.wide_loadings(12000, 32, True, 73)
    whole = hip.rotate_loadings(A, 6000, varimax_only=True, want_B=True)
    assert whole["n_iter"] > 7
    g0 = _giveups()
    monkeypatch.setenv("XMCA_VARIMAX_TEST_GIVEUP", "7")
    cut = hip.rotate_loadings(A, 6000, varimax_only=True, want_B=True)
    assert _giveups() == g0 + 1
    assert cut["n_iter"] == whole["n_iter"]
    assert E.rel(cut["R"], whole["R"]) < 1e-9 and E.rel(cut["B"], whole["B"]) < 1e-9
