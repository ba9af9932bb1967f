"""GPU: `xmca_amd.gaps.fill_gaps` - DINEOF gap filling with the masked kernels of csrc/gap_fill.h.  The numpy
restatement and the cases: tests/fill_gaps_cases.py.

  * the centring and mask kernels alone (`Handle.gap_center`) against exactly summed column means, on shapes on both sides of
    the fill kernel's tile edges, with a column that holds one value and a row that holds none;
  * the fill kernel alone (`Handle.gap_fill_step`) against Z^T P to the bound of a sum of k products, untouched entries to the bit,
    the sum of squared changes to its bound, an all-zero mask, one mode, and mode counts above the chunk a lane holds;
  * the whole loop state for state against the restatement after 25 iterations (tol = 0) on both eigensolver routes - T up to
    97, where the block Jacobi's vectors are polished, and 800 x 900 (5 iterations), where the partial stage of the tridiagonal
    route gives the k leading vectors alone -, cross-validation, candidates,
    convergence, recovery of the removed values, the invariants of the returned field, a neighbour on the handle, the facade.

Tolerances.  float64: 50 delta, delta the larger of the difference between the restatement's two float64 routes on the case and
2^-52 max|X| - the device's split-K Gram product and its eigensolver round differently from LAPACK and 25 iterations carry that
along.  float32: 8 x the worst difference measured on an MI355X over the cases (profiles/fill_gaps_accuracy.json), never above
1e-3 max|X|.  The worst differences go to the file named by XMCA_FILL_GAPS_ACCURACY when that is set."""
import json
import math
import os
import sys

import numpy as np
import pytest

import fill_gaps_cases as C
from xmca_amd import _hip, gaps
from xmca_amd.array import MCA

pytestmark = pytest.mark.gpu

F64_MARGIN = 50.0
F32_MEASURED = 2.360e-06            # worst |device - restatement| over STATE_CASES on float32 fields (MI355X, 97x333; max|X| ~ 12)
F32_TOL = 8 * F32_MEASURED
F32_CAP = 1e-3                      # x max|X|: a wrong result must not pass as rounding
WORST = {}
U = 2.0 ** -53


def _note(group, name, value, bound):
    print("%s %s: %.3e (bound %.3e)" % (group, name, value, bound))
    WORST.setdefault(group, {})[name] = {"measured": float(value), "bound": float(bound)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _case(case, dtype=np.float64):
    T, N, r, k, frac = case
    return C.case_field(T, N, r, frac, dtype) + (k,)


def test_the_cases_know_the_tile_of_the_library():
    assert _hip.gap_fill_tile() == (C.TILE_ROWS, C.TILE_COLS)


# ---- the centring and mask kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", C.EDGE_CASES + [C.MAIN_CASES[0]], ids=C.case_name)
def test_centring_against_exact_column_means(hip, case, dtype):
    X = _case(case, dtype)[0]
    T, N = X.shape
    X[:, 3] = np.nan
    X[T // 2, 3] = 7.25                         # a column with one present value
    X[T - 2, :] = np.nan                         # a time step with nothing present
    present = np.isfinite(X)
    mean, mask, A, scale = hip.gap_center(X)
    assert mask.dtype == np.uint8 and np.array_equal(mask, (~present).astype(np.uint8))
    X64 = X.astype(np.float64)
    exact = np.array([math.fsum(X64[present[:, n], n]) / present[:, n].sum() for n in range(N)])
    bound = present.sum(axis=0) * U * np.nanmax(np.abs(X64), axis=0)          # of a float64 sum in any order, then one division
    err = np.abs(mean - exact)
    _note("center_mean_" + np.dtype(dtype).name, C.case_name(case), np.max(err / bound), 1.0)
    assert np.all(err <= bound)
    assert mean[3] == 7.25 and A[T // 2, 3] == 0.0
    eps = float(np.finfo(dtype).eps)
    ref = np.where(present, X64 - exact, 0.0)
    assert np.all(A[~present] == 0.0)
    assert np.all(np.abs(A - ref) <= bound + eps * np.abs(ref))               # (the plane is stored in the field's dtype)
    assert A.astype(dtype).astype(np.float64).tobytes() == A.tobytes()
    ref_scale = math.sqrt(math.fsum(ref[present] ** 2) / present.sum())
    tol = ref_scale * (present.sum() * U + 2 * eps) + 2 * bound.max()
    _note("center_scale_" + np.dtype(dtype).name, C.case_name(case), abs(scale - ref_scale), tol)
    assert abs(scale - ref_scale) <= tol
    again = hip.gap_center(X)
    assert np.array_equal(again[0], mean) and np.array_equal(again[2], A) and again[3] == scale


def test_centring_refuses_a_dead_column_and_an_inf(hip):
    X = _case(C.MAIN_CASES[0])[0]
    bad = X.copy()
    bad[:, 4] = np.nan
    with pytest.raises(ValueError, match="no finite value"):
        hip.gap_center(bad)
    bad = X.copy()
    bad[1, 1] = np.inf
    with pytest.raises(ValueError, match="Inf"):
        hip.gap_center(bad)
    assert hip.gap_center(X)[1].sum() == np.isnan(X).sum()


# ---- the fill kernel --------------------------------------------------------------------------------------------------------------
def _fill_inputs(T, N, k, dtype, seed=0):
    rng = np.random.default_rng([seed, T, N, k])
    A = rng.standard_normal((T, N)).astype(dtype)
    mask = rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=(T, N), p=[0.7, 0.25, 0.05])
    Z = rng.standard_normal((k, T))
    P = rng.standard_normal((k, N))
    return A, mask, Z, P


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", C.KERNEL_SHAPES, ids=lambda s: "%dx%d_k%d" % s)
def test_fill_step_against_the_product(hip, shape, dtype):
    T, N, k = shape
    A, mask, Z, P = _fill_inputs(T, N, k, dtype)
    out, total = hip.gap_fill_step(A, mask, Z, P)
    assert out.dtype == A.dtype and out.shape == A.shape
    keep = mask == 0
    assert np.array_equal(_bits(out)[keep], _bits(A)[keep])
    R = Z.T @ P
    # a sum of k products in float64: k u sum|z||p| in any order; x 4 for the order of the sum (numpy's own is in it too)
    bound = 4 * k * U * (np.abs(Z).T @ np.abs(P))
    if dtype == np.float32:
        bound = bound + 2.0 ** -24 * np.abs(R)          # the store rounds to float32
    err = np.abs(out.astype(np.float64) - R)[~keep]
    _note("fill_step_" + np.dtype(dtype).name, "%dx%d_k%d" % shape, np.max(err / bound[~keep]), 1.0)
    assert np.all(err <= bound[~keep])
    d = (out.astype(np.float64) - A.astype(np.float64))[~keep]          # (exact in float64 for float32 planes)
    ref_total = math.fsum(d * d)
    # every term d^2 within 2 u of the exact one (the difference and the square), then a sum of n terms in a fixed tree
    tol_total = (d.size + 4) * 2 * U * ref_total
    _note("fill_sum_" + np.dtype(dtype).name, "%dx%d_k%d" % shape, abs(total - ref_total), tol_total)
    assert abs(total - ref_total) <= tol_total
    out2, total2 = hip.gap_fill_step(A, mask, Z, P)
    assert np.array_equal(_bits(out2), _bits(out)) and total2 == total


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fill_step_with_nothing_masked_changes_nothing(hip, dtype):
    T, N, k = C.KERNEL_SHAPES[1]
    A, mask, Z, P = _fill_inputs(T, N, k, dtype)
    out, total = hip.gap_fill_step(A, np.zeros_like(mask), Z, P)
    assert np.array_equal(_bits(out), _bits(A)) and total == 0.0
    out, total = hip.gap_fill_step(A, np.ones_like(mask), Z, P)          # ... and with everything masked every entry moves
    assert not np.any(_bits(out) == _bits(A)) and total > 0.0


# ---- the whole loop, state for state ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.STATE_CASES, ids=C.case_name)
def test_state_after_25_iterations_float64(hip, case):
    X, truth, k = _case(case)
    ref = C.reference(case)
    delta = C.route_delta(case)
    out = gaps.fill_gaps(X, k, max_iter=C.STATE_ITERATIONS, tol=0.0, handle=hip)
    assert out["iterations"] == C.STATE_ITERATIONS and not out["converged"] and out["n_modes"] == k and out["cv_rms"] is None
    err = float(np.max(np.abs(out["field"] - ref["field"])))
    _note("state_float64", C.case_name(case), err, F64_MARGIN * delta)
    assert err <= F64_MARGIN * delta
    hist = float(np.max(np.abs(out["history"] - ref["history"])))
    _note("history_float64", C.case_name(case), hist, F64_MARGIN * delta)
    assert out["history"].shape == (C.STATE_ITERATIONS,) and hist <= F64_MARGIN * delta
    lam = float(np.max(np.abs(out["singular_values"] * (X.shape[0] - 1) / ref["lam"] - 1)))
    _note("lam_float64", C.case_name(case), lam, 1e-10)
    assert lam <= 1e-10


@pytest.mark.parametrize("case", C.STATE_CASES, ids=C.case_name)
def test_state_after_25_iterations_float32(hip, case):
    X, truth, k = _case(case, np.float32)
    ref = C.reference(case, np.float32)          # in float64 on the float32 input
    out = gaps.fill_gaps(X, k, max_iter=C.STATE_ITERATIONS, tol=0.0, handle=hip)
    assert out["field"].dtype == np.float32 and out["iterations"] == C.STATE_ITERATIONS
    err = float(np.max(np.abs(out["field"].astype(np.float64) - ref["field"])))
    cap = F32_CAP * float(np.nanmax(np.abs(X)))
    _note("state_float32", C.case_name(case), err, min(F32_TOL, cap))
    assert F32_TOL <= cap
    assert err <= F32_TOL


def test_state_on_the_partial_eigensolver_route_float64(hip):
    """T = 800: the k leading vectors come from the partial stage of the tridiagonal route (a k x T plane, no polish)"""
    case, its = C.LARGE_CASE, C.LARGE_ITERATIONS
    X, truth, k = _case(case)
    ref = C.reference(case, iterations=its)
    delta = C.route_delta(case, iterations=its)
    hip.reset_timings()
    out = gaps.fill_gaps(X, k, max_iter=its, tol=0.0, handle=hip)
    assert hip.timings().get("trd_reduce_calls") == its          # (the reduction ran once per iteration: this is that route)
    err = float(np.max(np.abs(out["field"] - ref["field"])))
    _note("state_float64", C.case_name(case), err, F64_MARGIN * delta)
    assert out["iterations"] == its and err <= F64_MARGIN * delta
    hist = float(np.max(np.abs(out["history"] - ref["history"])))
    _note("history_float64", C.case_name(case), hist, F64_MARGIN * delta)
    assert hist <= F64_MARGIN * delta
    lam = float(np.max(np.abs(out["singular_values"] * (X.shape[0] - 1) / ref["lam"] - 1)))
    _note("lam_float64", C.case_name(case), lam, 1e-10)
    assert lam <= 1e-10
    present = np.isfinite(X)
    assert np.array_equal(_bits(out["field"])[present], _bits(X)[present]) and np.isfinite(out["field"]).all()
    again = gaps.fill_gaps(X, k, max_iter=its, tol=0.0, handle=hip)
    assert np.array_equal(_bits(again["field"]), _bits(out["field"]))


def test_state_on_the_partial_eigensolver_route_float32(hip):
    case, its = C.LARGE_CASE, C.LARGE_ITERATIONS
    X, truth, k = _case(case, np.float32)
    ref = C.reference(case, np.float32, iterations=its)
    out = gaps.fill_gaps(X, k, max_iter=its, tol=0.0, handle=hip)
    assert out["field"].dtype == np.float32 and out["iterations"] == its
    err = float(np.max(np.abs(out["field"].astype(np.float64) - ref["field"])))
    cap = F32_CAP * float(np.nanmax(np.abs(X)))
    _note("state_float32", C.case_name(case), err, min(F32_TOL, cap))
    assert F32_TOL <= cap and err <= F32_TOL


# ---- invariants of the returned field ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_present_entries_keep_their_bits_and_only_dead_columns_are_nan(hip, dtype):
    T, N, r, k, frac = C.MAIN_CASES[1]
    X = C.case_field(T, N, r, frac, dtype)[0]
    dead = [0, 17, N - 1]
    X[:, dead] = np.nan
    out = gaps.fill_gaps(X, k, max_iter=10, tol=0.0, handle=hip)
    F = out["field"]
    assert F.dtype == X.dtype and F.shape == X.shape
    present = np.isfinite(X)
    assert np.array_equal(_bits(F)[present], _bits(X)[present])
    nan_cols = np.isnan(F).all(axis=0)
    assert list(np.flatnonzero(nan_cols)) == dead and np.isfinite(F[:, ~nan_cols]).all()
    again = gaps.fill_gaps(X, k, max_iter=10, tol=0.0, handle=hip)
    assert np.array_equal(_bits(again["field"]), _bits(F)) and np.array_equal(again["history"], out["history"])
    assert np.array_equal(again["singular_values"], out["singular_values"])


def test_a_field_with_two_spatial_dimensions_comes_back_in_its_shape(hip):
    T, N, r, k, frac = C.MAIN_CASES[0]
    X = C.case_field(T, N, r, frac)[0]
    X[:, 7] = np.nan
    cube = X.reshape(T, 5, 6)
    out = gaps.fill_gaps(cube, k, max_iter=10, tol=0.0, handle=hip)
    flat = gaps.fill_gaps(X, k, max_iter=10, tol=0.0, handle=hip)
    assert out["field"].shape == (T, 5, 6) and np.array_equal(_bits(out["field"].reshape(T, N)), _bits(flat["field"]))
    assert np.isnan(out["field"][:, 1, 1]).all() and np.isnan(out["field"]).sum() == T


# ---- convergence, cross-validation, recovery -----------------------------------------------------------------------------------------
def test_convergence_at_the_restatements_step(hip):
    X, truth, k = _case(C.CONVERGENCE_CASE)
    out = gaps.fill_gaps(X, k, tol=C.CONVERGENCE_TOL, handle=hip)
    print("iterations", out["iterations"], "last d", out["history"][-1])
    assert out["converged"] and abs(out["iterations"] - C.CONVERGENCE_ITERATIONS) <= 1
    assert out["history"].shape == (out["iterations"],) and out["history"][-1] < C.CONVERGENCE_TOL
    assert np.all(out["history"][:-1] >= C.CONVERGENCE_TOL)
    short = gaps.fill_gaps(X, k, max_iter=5, tol=C.CONVERGENCE_TOL, handle=hip)
    assert not short["converged"] and short["iterations"] == 5 and short["history"].shape == (5,)
    assert np.array_equal(short["history"], out["history"][:5])


def test_cross_validation_error_and_the_withheld_bits(hip):
    case = C.CV_CASE
    X, truth, k = _case(case)
    idx = C.cv_indices(X, C.CV_SHARE, C.CV_SEED)
    ref = C.reference(case, cv=True)
    delta = C.route_delta(case, cv=True)
    out = gaps.fill_gaps(X, k, max_iter=C.STATE_ITERATIONS, tol=0.0, cv_idx=idx, handle=hip)
    # the state tolerance scaled to the value: 50 delta belongs to values of the size max|X|, cv_rms is that much smaller
    tol = F64_MARGIN * delta * ref["cv_rms"] / float(np.nanmax(np.abs(X)))
    err = abs(out["cv_rms"] - ref["cv_rms"])
    _note("cv_rms_float64", C.case_name(case), err, tol)
    assert err <= tol
    assert float(np.max(np.abs(out["field"] - ref["field"]))) <= F64_MARGIN * delta
    assert np.array_equal(_bits(out["field"]).reshape(-1)[idx], _bits(X).reshape(-1)[idx])
    by_fraction = gaps.fill_gaps(X, k, max_iter=C.STATE_ITERATIONS, tol=0.0, cv_fraction=C.CV_SHARE, seed=C.CV_SEED, handle=hip)
    assert by_fraction["cv_rms"] == out["cv_rms"]          # (the same draw: every column of the case is kept)


def test_candidates_choose_the_restatements_number_of_modes(hip):
    X, truth, k = _case(C.CV_CASE)
    idx = C.cv_indices(X, C.CV_SHARE, C.CV_SEED)
    curve = {kk: C.dineof(X, kk, 60, 1e-5, cv_idx=idx)["cv_rms"] for kk in C.CV_CANDIDATES}
    out = gaps.fill_gaps(X, C.CV_CANDIDATES, max_iter=60, tol=1e-5, cv_idx=idx, handle=hip)
    print("cv curve", out["cv_curve"], "restatement", curve)
    assert list(out["cv_curve"]) == list(C.CV_CANDIDATES)
    assert sorted(out["cv_curve"], key=out["cv_curve"].get) == sorted(curve, key=curve.get)
    assert out["n_modes"] == min(curve, key=curve.get) and out["cv_rms"] == out["cv_curve"][out["n_modes"]]
    final = gaps.fill_gaps(X, out["n_modes"], max_iter=60, tol=1e-5, handle=hip)          # nothing withheld in the last run
    assert np.array_equal(_bits(final["field"]), _bits(out["field"])) and np.isfinite(out["field"]).all()


@pytest.mark.parametrize("case", C.MAIN_CASES, ids=C.case_name)
def test_recovery_of_the_removed_values(hip, case):
    X, truth, k = _case(case)
    out = gaps.fill_gaps(X, k, max_iter=60, tol=1e-5, handle=hip)
    ratio = C.recovery_ratio(out["field"], X, truth)
    _note("recovery_ratio", C.case_name(case), ratio, C.RECOVERY_RATIO)
    assert ratio <= C.RECOVERY_RATIO


# ---- the C entry's own refusals, a neighbour on the handle, the facade ---------------------------------------------------------------
def test_refusals_of_the_entry_point_leave_the_handle_usable(hip):
    X, truth, k = _case(C.MAIN_CASES[0])
    T, N = X.shape
    good = hip.fill_gaps(X, k, 3, 0.0)
    for bad_k in (0, min(T, N)):
        with pytest.raises(ValueError, match="n_modes"):
            hip.fill_gaps(X, bad_k, 3, 0.0)
    with pytest.raises(ValueError, match="max_iter"):
        hip.fill_gaps(X, k, 0, 0.0)
    for bad_tol in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tol"):
            hip.fill_gaps(X, k, 3, bad_tol)
    dead = X.copy()
    dead[:, 2] = np.nan
    with pytest.raises(ValueError, match="no finite value"):
        hip.fill_gaps(dead, k, 3, 0.0)
    inf = X.copy()
    inf[0, 0] = -np.inf
    with pytest.raises(ValueError, match="Inf"):
        hip.fill_gaps(inf, k, 3, 0.0)
    present = np.flatnonzero(np.isfinite(X).reshape(-1))
    missing = np.flatnonzero(np.isnan(X).reshape(-1))
    for bad_idx, what in (([present[0], X.size], "out of range"), ([present[0], present[0]], "repeated"), ([missing[0]], "missing value")):
        with pytest.raises(ValueError, match=what):
            hip.fill_gaps(X, k, 3, 0.0, cv_idx=np.array(bad_idx))
    flat = np.where(np.isfinite(X), np.arange(N, dtype=np.float64), np.nan)          # every column constant where present
    with pytest.raises(np.linalg.LinAlgError, match="variance"):
        hip.fill_gaps(flat, k, 3, 0.0)
    again = hip.fill_gaps(X, k, 3, 0.0)
    assert np.array_equal(_bits(again[0]), _bits(good[0])) and np.array_equal(again[1], good[1])


def test_a_solved_and_rotated_neighbour_keeps_its_result_to_the_bit(hip):
    T, N, r, k, frac = C.MAIN_CASES[1]
    X, truth = C.case_field(T, N, r, frac)
    m = MCA(truth, handle=hip)
    m.solve()
    m.rotate(3)
    before = (m.singular_values().copy(), m.eofs(3)['left'].copy(), m.pcs(3)['left'].copy())
    hip.reset_timings()
    out = gaps.fill_gaps(X, k, max_iter=10, tol=0.0, handle=hip)
    assert {"gap_center", "gram", "gap_eigh", "gap_project", "gap_fill", "gap_finish"} <= set(hip.timings())
    for a, b in zip(before, (m.singular_values(), m.eofs(3)['left'], m.pcs(3)['left'])):
        assert np.array_equal(a, b)
    filled = MCA(out["field"], handle=hip)
    filled.solve()
    assert filled._fields['left'].shape == (T, N) and filled.eofs(2)['left'].shape == (N, 2)          # every column kept
    assert np.isnan(X).any(axis=0).all()          # (the field with its gaps would have kept none)


def test_facade_returns_a_dataarray_over_the_fields_coordinates(hip):
    try:
        import xarray as xr
    except Exception:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
        import xarray as xr
    from xmca_amd import xarray as facade
    T, N, r, k, frac = C.MAIN_CASES[0]
    X = C.case_field(T, N, r, frac)[0]
    X[:, 11] = np.nan
    time, lat, lon = np.arange(T) * 10, np.linspace(-20, 20, 5), np.linspace(0, 50, 6)
    da = xr.DataArray(X.reshape(T, 5, 6), dims=['time', 'lat', 'lon'], coords={'time': time, 'lat': lat, 'lon': lon}, name='sst',
                      attrs={'units': 'K'})
    out = facade.fill_gaps(da, k, max_iter=10, tol=0.0, handle=hip)
    plain = gaps.fill_gaps(X.reshape(T, 5, 6), k, max_iter=10, tol=0.0, handle=hip)
    F = out['field']
    assert isinstance(F, xr.DataArray) and list(F.dims) == ['time', 'lat', 'lon'] and F.name == 'sst' and dict(F.attrs) == {'units': 'K'}
    for name, values in (('time', time), ('lat', lat), ('lon', lon)):
        assert np.array_equal(np.asarray(F.coords[name]), values)
    assert np.array_equal(_bits(np.asarray(F.values)), _bits(plain['field'])) and out['iterations'] == 10
    assert set(out) == set(plain) == {'field', 'n_modes', 'iterations', 'converged', 'history', 'cv_rms', 'singular_values'}


def test_zz_write_accuracy_record():
    """(last in the file) the worst differences of this run, for profiles/fill_gaps_accuracy.json"""
    path = os.environ.get("XMCA_FILL_GAPS_ACCURACY")
    if path and WORST:
        with open(path, "w") as f:
            json.dump({"what": "tests/test_gpu_fill_gaps.py with XMCA_FILL_GAPS_ACCURACY set: per group and case the measured figure "
                               "and its bound (state_*: max |device - numpy restatement| of the field after the iterations)",
                       "tolerances": {"float64": "%g x delta per case" % F64_MARGIN, "float32": F32_TOL, "float32_cap": "1e-3 max|X|"},
                       "worst": {g: max(v["measured"] for v in cases.values()) for g, cases in WORST.items()},
                       "figures": WORST}, f, indent=1, sort_keys=True)
