"""GPU: `xmca_amd.gaps.fill_gaps(embedding=, tau=)` (M-SSA gap filling) - the DINEOF loop on the lag-embedded
plane with `gap_lag_fill_kernel` of csrc/gap_fill.h.  The numpy restatement and the cases: tests/lagged_fill_gaps_cases.py.

  * the lagged fill kernel alone (`Handle.gap_lag_fill_step`) against numpy's diag(1 / c) A~ P to the bound of a sum of M k
    products, on planes on both sides of the tile edges, mode counts around the chunk a lane holds, lag spans above a row tile and
    tau = T'; untouched entries to the bit, the sum of squared changes to its bound, repeated bits, all-zero and all-one masks;
  * the whole loop state for state against the restatement after 25 iterations (tol = 0), float64 and float32, and after 5
    iterations on 800 x 900 (T' = 798: the tridiagonal route) and 780 x 64 (T' = 764 < 768 <= T: the sweeps and the polish);
  * embedding = 1 to the bit of the call without it, the invariants of the returned field, dead time steps bridged on the
    device, cross-validation, candidates, convergence, the entry's refusals and a neighbour on the handle.

Tolerances.  float64: 50 delta, delta the larger of the difference between the restatement's two float64 routes on the case and
2^-52 max|X| (the margin of tests/test_gpu_fill_gaps.py for the same loop).  float32: 8 eps32, eps32 the distance of the
restatement in float32 arithmetic from the float64 restatement on the case's float32 field - a figure of the restatement alone -,
never above 1e-3 max|X|.  The figures go to the file named by XMCA_LAGGED_FILL_GAPS_ACCURACY when that is set."""
import json
import math
import os

import numpy as np
import pytest

import fill_gaps_cases as D
import lagged_fill_gaps_cases as C
from xmca_amd import _hip, gaps
from xmca_amd.array import MCA

pytestmark = pytest.mark.gpu

F64_MARGIN = 50.0
F32_FACTOR = 8.0
F32_CAP = 1e-3                      # x max|X|: a wrong result must not pass as rounding
WORST = {}
U = 2.0 ** -53


def _note(group, name, value, bound):
    print("%s %s: %.3e (bound %.3e)" % (group, name, value, bound))
    WORST.setdefault(group, {})[name] = {"measured": float(value), "bound": float(bound)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _run(hip, case, dtype=np.float64, **kw):
    T, N, k, M, tau, frac, dead = case
    X = C.case_field(case, dtype)[0]
    kw.setdefault("max_iter", C.iterations_of(case))
    kw.setdefault("tol", 0.0)
    return X, gaps.fill_gaps(X, k, handle=hip, embedding=M, tau=tau, **kw)


def test_the_cases_know_the_tile_of_the_library():
    assert _hip.gap_fill_tile() == (C.TILE_ROWS, C.TILE_COLS)


# ---- the lagged fill kernel ---------------------------------------------------------------------------------------------------------
def _fill_inputs(T, N, k, M, tau, dtype):
    rng = np.random.default_rng([7, T, N, k, M, tau])
    A = rng.standard_normal((T, N)).astype(dtype)
    mask = rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=(T, N), p=[0.7, 0.25, 0.05])
    Z = rng.standard_normal((k, T - (M - 1) * tau))
    P = rng.standard_normal((M * k, N))
    return A, mask, Z, P


KERNEL_CASES = [(T, N, k, M, tau) for T, N in C.KERNEL_PLANES for k in C.KERNEL_MODES for M, tau in C.kernel_embeddings(T)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", KERNEL_CASES, ids=lambda s: "%dx%d_k%d_M%d_tau%d" % s)
def test_lag_fill_step_against_the_averaged_product(hip, shape, dtype):
    T, N, k, M, tau = shape
    A, mask, Z, P = _fill_inputs(T, N, k, M, tau, dtype)
    out, total = hip.gap_lag_fill_step(A, mask, Z, P, M, tau)
    assert out.dtype == A.dtype and out.shape == A.shape
    keep = mask == 0
    assert np.array_equal(_bits(out)[keep], _bits(A)[keep])
    R = C.averaged(Z, P, T, M, tau)
    # a sum of at most M k products in float64, in any order (numpy's own is in the x 4), over c_t; the division by c_t and the
    # rounding of numpy's own quotient
    bound = 4 * M * k * U * C.averaged(np.abs(Z), np.abs(P), T, M, tau) + 2 * U * np.abs(R)
    if dtype == np.float32:
        bound = bound + 2.0 ** -24 * np.abs(R)          # the store rounds to float32
    err = np.abs(out.astype(np.float64) - R)[~keep]
    _note("lag_fill_step_" + np.dtype(dtype).name, "%dx%d_k%d_M%d_tau%d" % shape, np.max(err / bound[~keep]), 1.0)
    assert np.all(err <= bound[~keep])
    d = (out.astype(np.float64) - A.astype(np.float64))[~keep]          # (exact in float64 for float32 planes)
    ref_total = math.fsum(d * d)
    tol_total = (d.size + 4) * 2 * U * ref_total                         # (the bound of test_fill_step_against_the_product)
    _note("lag_fill_sum_" + np.dtype(dtype).name, "%dx%d_k%d_M%d_tau%d" % shape, abs(total - ref_total), tol_total)
    assert abs(total - ref_total) <= tol_total
    out2, total2 = hip.gap_lag_fill_step(A, mask, Z, P, M, tau)
    assert np.array_equal(_bits(out2), _bits(out)) and total2 == total
    if M == 1:          # one window: the chain of gap_fill_kernel and a product by 1
        plain, plain_total = hip.gap_fill_step(A, mask, Z, P)
        assert np.array_equal(_bits(plain), _bits(out)) and plain_total == total


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(65, 257, 17, 5, 3), (150, 30, 16, 24, 3), (64, 256, 1, 2, 32)], ids=lambda s: "%dx%d_k%d_M%d_tau%d" % s)
def test_lag_fill_step_with_nothing_and_with_everything_masked(hip, shape, dtype):
    T, N, k, M, tau = shape
    A, mask, Z, P = _fill_inputs(T, N, k, M, tau, dtype)
    out, total = hip.gap_lag_fill_step(A, np.zeros_like(mask), Z, P, M, tau)
    assert np.array_equal(_bits(out), _bits(A)) and total == 0.0
    out, total = hip.gap_lag_fill_step(A, np.ones_like(mask), Z, P, M, tau)
    assert not np.any(_bits(out) == _bits(A)) and total > 0.0
    R = C.averaged(Z, P, T, M, tau)
    assert np.max(np.abs(out.astype(np.float64) - R)) <= 1e-5 * np.max(np.abs(R))          # (every row of every window took part)


def test_lag_fill_step_refusals_leave_the_handle_usable(hip):
    T, N, k, M, tau = 30, 20, 2, 2, 20          # T' = 10 < tau
    A, mask, Z, P = _fill_inputs(T, N, k, M, tau, np.float64)
    with pytest.raises(ValueError, match="tau"):
        hip.gap_lag_fill_step(A, mask, Z, P, M, tau)
    with pytest.raises(ValueError, match="embedding"):
        hip.gap_lag_fill_step(A, mask, Z, P, 0, 1)
    with pytest.raises(ValueError, match="Z of k x T'"):
        hip.gap_lag_fill_step(A, mask, Z[:, :-1], P, M, tau)
    A, mask, Z, P = _fill_inputs(30, 20, 2, 2, 3, np.float64)
    assert hip.gap_lag_fill_step(A, mask, Z, P, 2, 3)[1] > 0.0


# ---- the whole loop, state for state ------------------------------------------------------------------------------------------------
def _held_to_the_restatement(case, X, out):
    ref, delta, name = C.reference(case), C.route_delta(case), C.case_name(case)
    T, N, k, M, tau, frac, dead = case
    its = C.iterations_of(case)
    assert out["iterations"] == its and not out["converged"] and out["n_modes"] == k and out["cv_rms"] is None
    assert out["embedding"] == M and out["tau"] == tau
    err = float(np.max(np.abs(out["field"] - ref["field"])))
    _note("state_float64", name, err, F64_MARGIN * delta)
    assert err <= F64_MARGIN * delta
    hist = float(np.max(np.abs(out["history"] - ref["history"])))
    _note("history_float64", name, hist, F64_MARGIN * delta)
    assert out["history"].shape == (its,) and hist <= F64_MARGIN * delta
    Tp = T - (M - 1) * tau
    lam = float(np.max(np.abs(out["singular_values"] * (Tp - 1) / ref["lam"] - 1)))
    _note("lam_float64", name, lam, 1e-10)
    assert lam <= 1e-10


@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
def test_state_after_25_iterations_float64(hip, case):
    X, out = _run(hip, case)
    _held_to_the_restatement(case, X, out)


def test_state_on_the_partial_eigensolver_route_float64(hip):
    """T' = 798: the k leading vectors come from the partial stage of the tridiagonal route (a k x T' plane, no polish)"""
    hip.reset_timings()
    X, out = _run(hip, C.LARGE_CASE)
    assert hip.timings().get("trd_reduce_calls") == C.BIG_ITERATIONS          # (the reduction ran once per iteration)
    _held_to_the_restatement(C.LARGE_CASE, X, out)


def test_the_eigensolver_route_is_chosen_at_the_windows_not_at_the_time_steps(hip):
    """T = 780 >= 768 > T' = 764: the block Jacobi sweeps and the polish, on a T' x T' plane of vectors"""
    hip.reset_timings()
    X, out = _run(hip, C.EDGE_CASE)
    tm = hip.timings()
    assert not tm.get("trd_reduce_calls") and "gap_lag_gram" in tm and "gap_eigh" in tm          # the reduction did not run
    _held_to_the_restatement(C.EDGE_CASE, X, out)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
def test_state_after_25_iterations_float32(hip, case):
    X, out = _run(hip, case, np.float32)
    ref = C.reference(case, np.float32)          # in float64 on the float32 input
    eps32 = C.eps32(case)
    assert out["field"].dtype == np.float32 and out["iterations"] == C.STATE_ITERATIONS
    err = float(np.max(np.abs(out["field"].astype(np.float64) - ref["field"])))
    bound = min(F32_FACTOR * eps32, F32_CAP * float(np.nanmax(np.abs(X))))
    _note("state_float32", C.case_name(case), err, bound)
    WORST["state_float32"][C.case_name(case)]["eps32"] = eps32
    assert err <= bound


# ---- bits and invariants --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_one_window_returns_the_bits_of_the_call_without_an_embedding(hip, dtype):
    T, N, k, M, tau, frac, dead = C.CASES[3]
    X = C.case_field(C.CASES[3], dtype)[0]
    idx = D.cv_indices(X, C.CV_SHARE, C.CV_SEED)
    plain = gaps.fill_gaps(X, k, max_iter=10, tol=0.0, cv_idx=idx, handle=hip)
    one = gaps.fill_gaps(X, k, max_iter=10, tol=0.0, cv_idx=idx, handle=hip, embedding=1, tau=7)
    assert np.array_equal(_bits(one["field"]), _bits(plain["field"])) and np.array_equal(one["history"], plain["history"])
    assert np.array_equal(one["singular_values"], plain["singular_values"]) and one["cv_rms"] == plain["cv_rms"]
    assert set(one) == set(plain)
    # ... and so does the lagged entry itself with one window
    field, history, cv_rms, lam = hip.fill_gaps_lagged(X, k, 1, 7, 10, 0.0, cv_idx=idx)
    assert np.array_equal(_bits(field), _bits(plain["field"])) and np.array_equal(history, plain["history"]) and cv_rms == plain["cv_rms"]
    assert np.array_equal(lam / (T - 1), plain["singular_values"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_present_and_withheld_entries_keep_their_bits_and_only_dead_columns_are_nan(hip, dtype):
    case = C.CASES[3]
    T, N, k, M, tau, frac, dead = case
    X = C.case_field(case, dtype)[0]
    gone = [0, 17, N - 1]
    X[:, gone] = np.nan
    flat_present = np.flatnonzero(np.isfinite(X).reshape(-1))
    idx = np.sort(np.random.default_rng(2).choice(flat_present, size=flat_present.size // 20, replace=False))
    out = gaps.fill_gaps(X, k, max_iter=10, tol=0.0, cv_idx=idx, handle=hip, embedding=M, tau=tau)
    F = out["field"]
    assert F.dtype == X.dtype and F.shape == X.shape and out["cv_rms"] > 0.0
    present = np.isfinite(X)
    assert np.array_equal(_bits(F)[present], _bits(X)[present])          # (the withheld entries are among them)
    nan_cols = np.isnan(F).all(axis=0)
    assert list(np.flatnonzero(nan_cols)) == gone and np.isfinite(F[:, ~nan_cols]).all()
    again = gaps.fill_gaps(X, k, max_iter=10, tol=0.0, cv_idx=idx, handle=hip, embedding=M, tau=tau)
    assert np.array_equal(_bits(again["field"]), _bits(F)) and np.array_equal(again["history"], out["history"])
    assert np.array_equal(again["singular_values"], out["singular_values"]) and again["cv_rms"] == out["cv_rms"]


def test_a_field_with_two_spatial_dimensions_comes_back_in_its_shape(hip):
    case = C.CASES[0]
    T, N, k, M, tau, frac, dead = case
    X = C.case_field(case)[0]
    X[:, 7] = np.nan
    cube = X.reshape(T, 5, 8)
    out = gaps.fill_gaps(cube, k, max_iter=10, tol=0.0, handle=hip, embedding=M, tau=tau)
    flat = gaps.fill_gaps(X, k, max_iter=10, tol=0.0, handle=hip, embedding=M, tau=tau)
    assert out["field"].shape == (T, 5, 8) and np.array_equal(_bits(out["field"].reshape(T, N)), _bits(flat["field"]))
    assert np.isnan(out["field"][:, 0, 7]).all() and np.isnan(out["field"]).sum() == T


# ---- dead time steps, cross-validation, convergence ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.DEVICE_DEAD_CASES, ids=C.case_name)
def test_dead_time_steps_are_bridged_on_the_device_and_not_by_one_window(hip, case):
    T, N, k, M, tau, frac, dead = case
    X, truth, rows = C.case_field(case)
    lagged = gaps.fill_gaps(X, k, max_iter=C.STATE_ITERATIONS, tol=0.0, handle=hip, embedding=M, tau=tau)
    plain = gaps.fill_gaps(X, k, max_iter=C.STATE_ITERATIONS, tol=0.0, handle=hip)
    a = C.dead_step_ratio(lagged["field"], X, truth, rows)
    b = C.dead_step_ratio(plain["field"], X, truth, rows)
    _note("dead_steps_lagged", C.case_name(case), a, C.DEAD_RATIO)
    _note("dead_steps_one_window", C.case_name(case), b, C.DINEOF_DEAD_RATIO)
    assert a <= C.DEAD_RATIO and b >= C.DINEOF_DEAD_RATIO


def test_candidates_give_the_restatements_curve_and_choose_four_modes(hip):
    case = C.CV_CASE
    T, N, k, M, tau, frac, dead = case
    X = C.case_field(case)[0]
    idx = D.cv_indices(X, C.CV_SHARE, C.CV_SEED)
    out = gaps.fill_gaps(X, C.CV_CANDIDATES, max_iter=C.STATE_ITERATIONS, tol=0.0, cv_idx=idx, handle=hip, embedding=M, tau=tau)
    assert list(out["cv_curve"]) == list(C.CV_CANDIDATES)
    for kk in C.CV_CANDIDATES:
        ref = C.reference(case, cv=True, k=kk)["cv_rms"]
        tol = F64_MARGIN * C.route_delta(case, cv=True, k=kk)
        _note("cv_curve_float64", "k%d" % kk, abs(out["cv_curve"][kk] - ref), tol)
        assert abs(out["cv_curve"][kk] - ref) <= tol
    assert out["n_modes"] == 4 and out["cv_rms"] == out["cv_curve"][4]
    assert np.array_equal(_bits(out["field"]).reshape(-1)[idx], _bits(X).reshape(-1)[idx])
    final = gaps.fill_gaps(X, 4, max_iter=C.STATE_ITERATIONS, tol=0.0, handle=hip, embedding=M, tau=tau)          # nothing withheld
    assert np.array_equal(_bits(final["field"]), _bits(out["field"])) and np.isfinite(out["field"]).all()
    by_fraction = gaps.fill_gaps(X, 4, max_iter=C.STATE_ITERATIONS, tol=0.0, cv_fraction=C.CV_SHARE, seed=C.CV_SEED, handle=hip,
                                 embedding=M, tau=tau)
    assert by_fraction["cv_rms"] == out["cv_rms"]          # (the same draw: every column of the case is kept)


def test_the_loop_stops_at_the_restatements_iteration(hip):
    case = C.CONVERGENCE_CASE
    T, N, k, M, tau, frac, dead = case
    X = C.case_field(case)[0]
    ref = C.mssa_fill(X, k, M, tau, 300, C.CONVERGENCE_TOL)
    out = gaps.fill_gaps(X, k, tol=C.CONVERGENCE_TOL, handle=hip, embedding=M, tau=tau)
    print("iterations", out["iterations"], "restatement", ref["iterations"], "last d", out["history"][-1])
    assert out["converged"] and out["iterations"] == ref["iterations"]
    assert out["history"].shape == (out["iterations"],) and out["history"][-1] < C.CONVERGENCE_TOL
    assert np.all(out["history"][:-1] >= C.CONVERGENCE_TOL)
    short = gaps.fill_gaps(X, k, max_iter=5, tol=C.CONVERGENCE_TOL, handle=hip, embedding=M, tau=tau)
    assert not short["converged"] and short["iterations"] == 5 and np.array_equal(short["history"], out["history"][:5])


# ---- the C entry's own refusals, a neighbour on the handle, the facade ---------------------------------------------------------------
def test_refusals_of_the_entry_point_leave_the_handle_usable(hip):
    case = C.CASES[0]
    T, N, k, M, tau, frac, dead = case
    X = C.case_field(case)[0]
    good = hip.fill_gaps_lagged(X, k, M, tau, 3, 0.0)
    for bad_M, bad_tau, what in ((0, 1, "embedding"), (M, 0, "tau"), (T, 1, "at least 2"), (3, 60, "at least 2"), (2, 61, "every window")):
        with pytest.raises(ValueError, match=what):
            hip.fill_gaps_lagged(X, k, bad_M, bad_tau, 3, 0.0)
    for bad_k, MM in ((0, M), (T - (M - 1) * tau, M), (11, 110)):          # T' = 109 binds; T' = 11 binds
        with pytest.raises(ValueError, match="n_modes"):
            hip.fill_gaps_lagged(X, bad_k, MM, tau, 3, 0.0)
    with pytest.raises(ValueError, match="max_iter"):
        hip.fill_gaps_lagged(X, k, M, tau, 0, 0.0)
    for bad_tol in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tol"):
            hip.fill_gaps_lagged(X, k, M, tau, 3, bad_tol)
    gone = X.copy()
    gone[:, 2] = np.nan
    with pytest.raises(ValueError, match="no finite value"):
        hip.fill_gaps_lagged(gone, k, M, tau, 3, 0.0)
    inf = X.copy()
    inf[0, 0] = -np.inf
    with pytest.raises(ValueError, match="Inf"):
        hip.fill_gaps_lagged(inf, k, M, tau, 3, 0.0)
    missing = np.flatnonzero(np.isnan(X).reshape(-1))
    with pytest.raises(ValueError, match="missing value"):
        hip.fill_gaps_lagged(X, k, M, tau, 3, 0.0, cv_idx=np.array([missing[0]]))
    flat = np.where(np.isfinite(X), np.arange(N, dtype=np.float64), np.nan)          # every column constant where present
    with pytest.raises(np.linalg.LinAlgError, match="variance"):
        hip.fill_gaps_lagged(flat, k, M, tau, 3, 0.0)
    again = hip.fill_gaps_lagged(X, k, M, tau, 3, 0.0)
    assert np.array_equal(_bits(again[0]), _bits(good[0])) and np.array_equal(again[1], good[1])


def test_a_solved_and_rotated_neighbour_keeps_its_result_to_the_bit(hip):
    case = C.CASES[4]
    T, N, k, M, tau, frac, dead = case
    X, truth, rows = C.case_field(case)
    m = MCA(truth, handle=hip)
    m.solve()
    m.rotate(3)
    before = (m.singular_values().copy(), m.eofs(3)['left'].copy(), m.pcs(3)['left'].copy())
    hip.reset_timings()
    out = gaps.fill_gaps(X, k, max_iter=10, tol=0.0, handle=hip, embedding=M, tau=tau)
    assert {"gap_center", "gram", "gap_lag_gram", "gap_eigh", "gap_project", "gap_fill", "gap_finish"} <= set(hip.timings())
    for a, b in zip(before, (m.singular_values(), m.eofs(3)['left'], m.pcs(3)['left'])):
        assert np.array_equal(a, b)
    assert np.isfinite(out["field"]).all()


def test_zz_write_accuracy_record():
    """(last in the file) the figures of this run, for profiles/lagged_fill_gaps_accuracy.json"""
    path = os.environ.get("XMCA_LAGGED_FILL_GAPS_ACCURACY")
    if path and WORST:
        with open(path, "w") as f:
            json.dump({"what": "tests/test_gpu_lagged_fill_gaps.py with XMCA_LAGGED_FILL_GAPS_ACCURACY set: per group and case the "
                               "measured figure and its bound (state_*: max |device - numpy restatement| of the field after the "
                               "iterations; state_float32 also eps32, the restatement's own float32 error, of which the bound is 8)",
                       "tolerances": {"float64": "%g x delta per case" % F64_MARGIN, "float32": "%g x eps32 per case" % F32_FACTOR,
                                      "float32_cap": "1e-3 max|X|"},
                       "worst": {g: max(v["measured"] for v in cases.values()) for g, cases in WORST.items()},
                       "figures": WORST}, f, indent=1, sort_keys=True)
