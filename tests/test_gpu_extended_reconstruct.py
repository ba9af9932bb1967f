"""GPU: `MCA.extended_reconstruct` - reconstructed components of extended EOFs as one product diag(1 / c) A~ P
(csrc/lag_reconstruct.h).  Truth and cases: tests/extended_reconstruct_cases.py.

  * the placement kernel alone through `Handle.lag_expand`: bit equality with numpy's placement, 1 / c_t included, at window counts
    around the 32 lanes of half a wavefront and at shifts up to the window count; the same bits on a second call;
  * the window means through `Handle.lag_window_means`: bit equality with numpy on integer-valued fields (every sum is exact), at
    column counts around the 64 lanes of a wavefront and past one workgroup, for float64 and float32 fields; on real-valued fields
    within the bound of a sum of T' terms;
  * end to end against the diagonal averaging of the truncated SVD at the project's model tolerances (tests/test_gpu_configs.py):
    1e-5 max|X| for float64 fields, 1e-3 max|X| for float32 ones; additivity over mode groups; the same bits on a second call;
  * completeness: all modes with original_scale=True give the field back;
  * `extended_reconstruct(1)` against `solve()` + `reconstructed_fields`, a solved and rotated model left bit-identical, a lost
    handle, output='torch', the xarray facade with coslat weights.

The worst measured errors of the end-to-end and completeness cases go to the file named by XMCA_EXTENDED_RECONSTRUCT_ACCURACY when
that is set (profiles/extended_reconstruct_accuracy.json holds the MI355X figures)."""
import json
import os
import sys

import numpy as np
import pytest

try:
    import torch                                            # (before the first device call of the session, as the other torch tests do)
except Exception:
    torch = None

import extended_eofs_cases as E
import extended_reconstruct_cases as C
from xmca_amd.array import MCA

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-5, np.float32: 1e-3}          # x max|X|
WORST = {}
WINDOWS = (2, 31, 32, 33)
LAGS = (1, 2, 5)


def _shifts(Tp):
    return (1, 3, Tp)


def _record(name, dtype, err, scale):
    key = name + "_" + np.dtype(dtype).name
    WORST[key] = max(WORST.get(key, 0.0), float(err / scale))
    print(key, "error / max|X| = %.3g" % (err / scale))


# ---- lag_expand ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tp", WINDOWS)
def test_lag_expand_is_numpy_placement_to_the_bit(hip, Tp):
    rng = np.random.default_rng(Tp)
    for M in LAGS:
        for tau in _shifts(Tp):
            for q in (1, 3):
                Z = rng.standard_normal((q, Tp))
                for ind in (False, True):
                    if M > 1 and tau > Tp:           # (T' = 2, tau = 3) time steps in no window: refused
                        with pytest.raises(ValueError):
                            hip.lag_expand(Z, M, tau, ind)
                        continue
                    A, inv = hip.lag_expand(Z, M, tau, ind)
                    T = Tp + (M - 1) * tau
                    assert A.shape == (T, M * (q + int(ind))) and inv.shape == (T,)
                    assert np.array_equal(A, C.expand(Z, M, tau, ind)), (Tp, M, tau, q, ind)
                    assert np.array_equal(inv, 1.0 / C.counts(T, M, tau)), (Tp, M, tau, q, ind)
                    A2, inv2 = hip.lag_expand(Z, M, tau, ind)
                    assert np.array_equal(A, A2) and np.array_equal(inv, inv2)


def test_lag_expand_refuses_bad_arguments(hip):
    Z = np.ones((2, 5))
    for M, tau in ((0, 1), (2, 0), (2, 6)):
        with pytest.raises(ValueError):
            hip.lag_expand(Z, M, tau, True)
    with pytest.raises(ValueError):
        hip.lag_expand(np.ones(5), 2, 1, True)
    A, inv = hip.lag_expand(Z, 2, 5, True)          # tau = T': the windows abut
    assert np.array_equal(inv, np.ones(10)) and np.array_equal(A, C.expand(Z, 2, 5, True))


# ---- lag_window_means ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_window_means_of_integer_fields_are_numpy_to_the_bit(hip, N, dtype):
    """|x| < 2^20 and at most 37 rows: every partial sum is an integer below 2^26, exact in any order and in float32 storage; the
    quotient by T' is one rounding of the same two numbers"""
    for Tp in WINDOWS:
        for M in LAGS:
            for tau in _shifts(Tp):
                T = Tp + (M - 1) * tau
                X = np.random.default_rng([Tp, M, tau, N]).integers(-2 ** 20 + 1, 2 ** 20, (T, N)).astype(dtype)
                hip.set_field(0, X)
                got = hip.lag_window_means(T, N, M, tau)
                assert got.shape == (M, N) and got.dtype == np.float64
                assert np.array_equal(got, C.window_means(X, M, tau)), (Tp, M, tau)
                assert np.array_equal(got, hip.lag_window_means(T, N, M, tau))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("N", [1, 65, 257])
def test_window_means_of_real_fields_are_within_the_bound_of_their_sums(hip, N, dtype):
    """two float64 sums of the same T' numbers in different orders differ by at most T' 2^-52 sum|x|"""
    for Tp in WINDOWS + (130,):
        for M in LAGS:
            for tau in _shifts(Tp):
                T = Tp + (M - 1) * tau
                X = (np.random.default_rng([Tp, M, tau, N]).standard_normal((T, N)) + 0.5).astype(dtype)
                hip.set_field(0, X)
                got = hip.lag_window_means(T, N, M, tau)
                bound = Tp * 2.0 ** -52 * C.window_means(np.abs(X), M, tau).max() * Tp
                err = np.abs(got - C.window_means(X, M, tau)).max()
                assert err <= bound, (Tp, M, tau, err, bound)


def test_window_means_refuse_bad_arguments(hip):
    hip.set_field(0, np.ones((10, 3)))
    for M, tau in ((0, 1), (2, 0), (4, 4)):
        with pytest.raises(ValueError):
            hip.lag_window_means(10, 3, M, tau)
    assert np.array_equal(hip.lag_window_means(10, 3, 4, 3), np.ones((4, 3)))


# ---- end to end: mode groups --------------------------------------------------------------------------------------------
def _check_groups(hip, name, field, X, keep, M, tau, dtype):
    """`field`: what the model is given; X: its kept columns (float64); the model centres them"""
    tol = TOL[dtype]
    mean = X.mean(axis=0)
    Xc = X - mean
    scale = np.abs(Xc).max()
    most = C.n_modes(Xc, M, tau)
    m = MCA(field.copy(), handle=hip)                                   # no solve() before it
    got = {}
    for i, group in enumerate(C.MODE_GROUPS):
        out = m.extended_reconstruct(M, tau=tau, mode=group, original_scale=False)['left']
        assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == field.shape
        flat = out.reshape(out.shape[0], -1)
        assert np.isnan(flat[:, ~keep]).all() and not np.isnan(flat[:, keep]).any()
        got[i] = flat[:, keep]
        err = np.abs(got[i] - C.truth(Xc, M, tau, C.mode_indices(group, most))).max()
        _record(name + "_group%d" % i, dtype, err, scale)
        assert err <= tol * scale, (group, err, tol * scale)
    # RC(1..3) = RC(1) + RC(2..3)
    err = np.abs(got[3] - (got[0] + got[4])).max()
    _record(name + "_additivity", dtype, err, scale)
    assert err <= tol * scale
    # the original scale: window means and the field's mean come back
    out = m.extended_reconstruct(M, tau=tau, mode=3)['left'].reshape(field.shape[0], -1)
    ref = C.truth(Xc, M, tau, np.arange(3), means=True) + mean
    err = np.abs(out[:, keep] - ref).max()
    _record(name + "_original_scale", dtype, err, np.abs(X).max())
    assert np.isnan(out[:, ~keep]).all() and err <= tol * np.abs(X).max()
    # a second call gives the same bits
    again = m.extended_reconstruct(M, tau=tau, mode=3)['left'].reshape(field.shape[0], -1)
    assert np.array_equal(out, again, equal_nan=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", C.GROUP_CASES, ids=lambda c: c[0])
def test_mode_groups_match_the_diagonal_average_of_the_truncated_svd(hip, case, dtype):
    name, T, N, M, tau, seed = case
    X = (E.case_field(T, N, seed) + np.linspace(-2.0, 2.0, N)).astype(dtype)
    _check_groups(hip, name, X, X.astype(np.float64), np.ones(N, dtype=bool), M, tau, dtype)


def test_mode_groups_past_the_tridiagonal_threshold(hip):
    name, T, N, M, tau, seed = C.LARGE_CASE
    X = E.case_field(T, N, seed)
    _check_groups(hip, name, X, X, np.ones(N, dtype=bool), M, tau, np.float64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_mode_groups_of_a_masked_three_dimensional_field(hip, dtype):
    name, T, shape, masked, M, tau, k, seed = C.MASKED_CASE
    full, X, keep = E.masked_field(T, shape, masked, seed)
    full = (full + 1.5).astype(dtype)
    _check_groups(hip, name, full, full.reshape(T, -1)[:, keep].astype(np.float64), keep, M, tau, dtype)


# ---- completeness -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("preprocess", ["device", "host"])
@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalized"])
@pytest.mark.parametrize("case", C.COMPLETE_CASES, ids=lambda c: "%dx%d_M%d_t%d" % c)
def test_all_modes_give_the_field_back(hip, case, normalize, preprocess, dtype):
    T, N, M, tau = case
    X = (C.full_field(T, N, 0) * np.linspace(0.5, 3.0, N) + np.linspace(-4.0, 4.0, N)).astype(dtype)
    m = MCA(X.copy(), handle=hip, preprocess=preprocess)
    if normalize:
        m.normalize()
    out = m.extended_reconstruct(M, tau, None, True)['left']
    assert out.dtype == np.float64 and out.shape == X.shape
    scale = np.abs(X).max()
    err = np.abs(out - X.astype(np.float64)).max()
    _record("complete_%dx%d_M%d_t%d_%s_%s" % (case + ("normalized" if normalize else "raw", preprocess)), dtype, err, scale)
    assert err <= TOL[dtype] * scale, (err, TOL[dtype] * scale)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_all_modes_give_a_masked_three_dimensional_field_back(hip, dtype):
    name, T, shape, masked, M, tau, k, seed = C.MASKED_CASE
    full, X, keep = C.masked_full_field(T, shape, masked, seed)
    full = (full + 2.5).astype(dtype)
    out = MCA(full.copy(), handle=hip).extended_reconstruct(M, tau, None, True)['left']
    assert out.shape == full.shape and np.array_equal(np.isnan(out), np.isnan(full))
    scale = np.nanmax(np.abs(full))
    err = np.nanmax(np.abs(out - full.astype(np.float64)))
    _record("complete_" + name, dtype, err, scale)
    assert err <= TOL[dtype] * scale


# ---- M = 1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("original_scale", [False, True], ids=["solve_units", "original_scale"])
@pytest.mark.parametrize("mode", [3, slice(2, 3)], ids=["k3", "k2to3"])
@pytest.mark.parametrize("shape", [(40, 23), (30, 130)], ids=["40x23", "30x130"])
def test_an_embedding_of_one_is_reconstructed_fields(hip, shape, mode, original_scale, dtype):
    X = (E.case_field(shape[0], shape[1], 0) + np.linspace(-1.0, 1.0, shape[1])).astype(dtype)
    m = MCA(X.copy(), handle=hip)
    m.solve()
    ref = np.asarray(m.reconstructed_fields(mode=mode, original_scale=original_scale)['left'], dtype=np.float64)
    out = m.extended_reconstruct(1, mode=mode, original_scale=original_scale)['left']
    assert out.shape == ref.shape
    assert np.abs(out - ref).max() <= TOL[dtype] * np.abs(X).max()


# ---- state --------------------------------------------------------------------------------------------------------------
def test_a_solved_and_rotated_model_keeps_its_result_to_the_bit(hip):
    name, T, N, M, tau, seed = C.GROUP_CASES[2]
    m = MCA(E.case_field(T, N, seed), handle=hip)
    m.solve()
    m.rotate(3)
    before = (m.singular_values().copy(), m.eofs(3)['left'].copy(), m.pcs(3)['left'].copy())
    eeof = m.extended_eofs(M, tau=tau, n_modes=3)
    hip.reset_timings()
    first = m.extended_reconstruct(M, tau=tau, mode=slice(1, 2))['left']
    assert {"eeof_expand", "eeof_window_means", "eeof_reconstruct"} <= set(hip.timings())
    for a, b in zip(before, (m.singular_values(), m.eofs(3)['left'], m.pcs(3)['left'])):
        assert np.array_equal(a, b)
    # a refused call leaves the handle usable
    with pytest.raises(ValueError):
        m.extended_reconstruct(M, tau=tau, mode=T)
    with pytest.raises(ValueError):
        hip.extended_reconstruct(T, N, M, tau, [1, 0], True)
    with pytest.raises(ValueError):
        hip.extended_reconstruct(T, N, 2, T - 3, [0], True)
    assert np.array_equal(first, m.extended_reconstruct(M, tau=tau, mode=slice(1, 2))['left'])
    for a, b in zip(before, (m.singular_values(), m.eofs(3)['left'], m.pcs(3)['left'])):
        assert np.array_equal(a, b)
    # extended_eofs returns the bits it returned before the reconstruction
    after = m.extended_eofs(M, tau=tau, n_modes=3)
    for key in ('singular_values', 'explained_variance', 'pcs'):
        assert np.array_equal(eeof[key], after[key])
    assert np.array_equal(eeof['eofs']['left'], after['eofs']['left'])


def test_a_model_that_lost_the_handle_uploads_its_field_again(hip):
    name, T, N, M, tau, seed = C.GROUP_CASES[0]
    X = E.case_field(T, N, seed)
    a = MCA(X.copy(), handle=hip)
    first = a.extended_reconstruct(M, tau=tau, mode=3)['left']
    b = MCA(E.case_field(T + 3, N + 2, seed + 1), handle=hip)          # takes over the resident field
    b.solve()
    second = a.extended_reconstruct(M, tau=tau, mode=3)['left']
    # (the field is centred again on the host before it goes up: the same field to rounding, not to the bit)
    assert np.abs(first - second).max() <= 1e-10 * np.abs(X).max()


def test_torch_output_is_written_on_the_device_with_the_bits_of_the_numpy_result(hip):
    assert torch is not None, "torch is part of the GPU test environment"
    name, T, shape, masked, M, tau, k, seed = C.MASKED_CASE
    full = E.masked_field(T, shape, masked, seed)[0] + 1.5
    ref = MCA(full.copy(), handle=hip).extended_reconstruct(M, tau=tau, mode=slice(2, 3))['left']
    out = MCA(torch.from_numpy(full).to("cuda:%d" % hip.device), handle=hip).extended_reconstruct(M, tau=tau, mode=slice(2, 3))['left']
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float64 and out.device == torch.device("cuda", hip.device)
    assert tuple(out.shape) == full.shape
    assert np.array_equal(out.cpu().numpy(), ref, equal_nan=True)
    # numpy in, tensors out
    out = MCA(full.copy(), handle=hip, output="torch").extended_reconstruct(M, tau=tau, mode=slice(2, 3))['left']
    assert isinstance(out, torch.Tensor) and np.array_equal(out.cpu().numpy(), ref, equal_nan=True)


def test_facade_on_a_lat_lon_field_with_coslat_weights(hip):
    try:
        import xarray as xr
    except Exception:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
        import xarray as xr
    from xmca_amd.xarray import xMCA
    name, T, shape, masked, M, tau, k, seed = C.MASKED_CASE
    full, X, keep = E.masked_field(T, shape, masked, seed)
    full = full + 3.0
    time, lat, lon = np.arange(T) * 10, np.linspace(-20, 20, shape[0]), np.linspace(0, 50, shape[1])
    da = xr.DataArray(full, dims=['time', 'lat', 'lon'], coords={'time': time, 'lat': lat, 'lon': lon})
    xm = xMCA(da)
    xm._handle_override = hip
    xm.apply_coslat()
    out = xm.extended_reconstruct(M, tau=tau, mode=slice(1, 2))['left']
    assert list(out.dims) == ['time', 'lat', 'lon'] and out.values.shape == full.shape
    assert np.array_equal(np.asarray(out.coords['time']), time)
    assert np.array_equal(np.asarray(out.coords['lat']), lat) and np.array_equal(np.asarray(out.coords['lon']), lon)
    assert np.array_equal(np.isnan(out.values), np.isnan(full))
    # the field solve() sees carries sqrt(cos(lat) + 1e-6); the inverse divides by sqrt(cos(lat)), as reconstructed_fields does
    cos = np.cos(np.deg2rad(np.repeat(lat, shape[1])))[keep]
    Xk = full.reshape(T, -1)[:, keep]
    mean = Xk.mean(axis=0)
    Xw = (Xk - mean) * np.sqrt(cos + 1e-6)
    ref = C.truth(Xw, M, tau, np.arange(2), means=True) / np.sqrt(cos) + mean
    err = np.abs(out.values.reshape(T, -1)[:, keep] - ref).max()
    assert err <= 1e-5 * np.abs(Xk).max(), err
    raw = xm.extended_reconstruct(M, tau=tau, mode=slice(1, 2), original_scale=False)['left']
    err = np.abs(raw.values.reshape(T, -1)[:, keep] - C.truth(Xw, M, tau, np.arange(2))).max()
    assert err <= 1e-5 * np.abs(Xw).max(), err


def test_zz_write_accuracy_record():
    """(last in the file) the worst errors of the end-to-end and completeness cases, for profiles/extended_reconstruct_accuracy.json"""
    path = os.environ.get("XMCA_EXTENDED_RECONSTRUCT_ACCURACY")
    if path and WORST:
        with open(path, "w") as f:
            json.dump({"tolerances_times_max_abs_field": {"float64": TOL[np.float64], "float32": TOL[np.float32]},
                       "worst_errors_over_max_abs_field": WORST}, f, indent=1, sort_keys=True)
