"""solve(complexify=True, extend='theta', period=m) on the device against the numpy restatement of the extension
(tests/theta_cases.py).

Kernel level: `xmca_theta_fit` (alpha, b0, level, seasonal means of every column, forecast and backcast) and the imaginary planes
X_im = G0 X + B C of `xmca_complexify_theta`.  The bounds come from the restatement alone (`theta_cases.tolerances`): alpha within
2 * 16^-6 (four candidates of the last round); everything else within 4 x the change of the restatement's own value when its
alpha moves by that step, plus a rounding floor of 64 eps T max |X|.  The columns meet the condition that no first-round choice
hinges on rounding (`theta_cases.checked_fits` asserts it).

Through the class: singular values, phase-aligned vectors, rotate(4) and fields() against the project's numpy oracle solve
(oracle/ref_numpy.py) of the restated analytic signal, at the tolerance tests/test_gpu_extend_exp.py applies to the 'exp' route
(its TOL and its `_rel`); n_modes, predict, bootstrapping and the xarray facade once each.  Without the feature every test here
fails: the entry points are missing, and `solve` raises ImportError("extend='theta' needs statsmodels").
"""
import os
import sys

import numpy as np
import pytest

import theta_cases as tc
from conftest import align_modes
from oracle import ref_numpy
from test_gpu_extend_exp import TOL, _rel
from xmca_amd import _hip
from xmca_amd.array import MCA
from xmca_amd.tools.array import block_bootstrap

pytestmark = pytest.mark.gpu


def _assert_fit_and_planes(dev_fit, dev_im, X, m, what):
    """dev_fit (2, 3 + m, N) and dev_im (T, N) of the device against the restatement of the float64 field X."""
    pair = tc.checked_fits(X, m)
    tol = tc.tolerances(X, m, pair)
    ref_fit = tc.packed(pair)
    ref_im = tc.analytic_signal(X, m, pair).imag
    assert np.isfinite(dev_fit).all() and np.isfinite(dev_im).all(), what
    err_fit = np.abs(dev_fit - ref_fit)
    err_im = float(np.abs(dev_im - ref_im).max())
    print("theta", what, "alpha %.3g (bound %.3g)" % (err_fit[:, 0].max(), tc.ALPHA_STEP),
          "fit/bound %.3g" % (err_fit[:, 1:] / tol["fit"][:, 1:]).max(), "planes %.3g (bound %.3g)" % (err_im, tol["planes"]))
    assert np.all(err_fit[:, 0] <= tc.ALPHA_STEP), what
    assert np.all(err_fit <= tol["fit"]), what
    assert err_im <= tol["planes"], what
    return pair


def _device_fit_and_planes(hip, X, m):
    T, N = X.shape
    hip.set_field(0, np.ascontiguousarray(X))
    fit = hip.theta_fit(0, N, m)                       # (a float32 field: fitted through a float64 copy)
    hip.complexify_theta(T, m)
    im = hip.get_field_imag(0, (T, N))
    assert hip.field_dtype == np.float64
    again = hip.theta_fit(0, N, m)                     # (the promoted field; the same bits on every call)
    assert np.array_equal(fit, again)
    return fit, im


@pytest.mark.parametrize("N", tc.N_VALUES)
@pytest.mark.parametrize("tkind", [0, 1, 2])
@pytest.mark.parametrize("m", tc.M_VALUES)
def test_fit_and_planes_match_the_restatement(hip, m, tkind, N):
    T = tc.lengths(m)[tkind]
    X = tc.columns(T, 130, m, seed=100 * m + T)[:, :N]
    for dtype in (np.float64, np.float32):
        Xd = X.astype(dtype)
        fit, im = _device_fit_and_planes(hip, Xd, m)
        _assert_fit_and_planes(fit, im, Xd.astype(np.float64), m, (m, T, N, np.dtype(dtype).name))


def test_alpha_at_both_bounds_in_the_interior_and_the_zero_column(hip):
    m, T = 4, 25
    X = tc.columns(T, 130, m, seed=100 * m + T)
    fit, im = _device_fit_and_planes(hip, X, m)
    alpha = fit[0, 0]
    assert np.sum(alpha == tc.ALPHA_LO) >= 20 and np.sum(alpha > 0.999) >= 10 and np.sum((alpha > 0.01) & (alpha < 0.99)) >= 20
    zero = np.arange(4, 130, 6)                        # the constant grid points: alpha = 1e-4, everything else exactly 0
    assert np.all(fit[:, 0][:, zero] == tc.ALPHA_LO)
    assert np.all(fit[:, 1:][:, :, zero] == 0.0) and np.all(im[:, zero] == 0.0)


def test_a_columns_fit_does_not_depend_on_its_neighbours(hip):
    """No exchange between columns, a fixed order over the candidates: column c of a wide field has the bits it has alone."""
    m, T = 3, 11
    X = tc.columns(T, 130, m, seed=100 * m + T)
    wide, im_wide = _device_fit_and_planes(hip, X, m)
    for c in (0, 63, 64, 129):
        one, im_one = _device_fit_and_planes(hip, X[:, c:c + 1], m)
        assert np.array_equal(one[:, :, 0], wide[:, :, c])
        assert np.abs(im_one[:, 0] - im_wide[:, c]).max() <= 64 * np.finfo(np.float64).eps * T * np.abs(X).max()   # (the GEMM tiles differ)


def test_entry_points_refuse_a_bad_period(hip):
    hip.set_field(0, tc.columns(9, 5, 4, seed=1))
    for period in (0, -1, 5):
        with pytest.raises(ValueError):
            hip.theta_fit(0, 5, period)
    col3, hbar, B = _hip.theta_imag_parts(9, 4)
    for period in (0, 5):
        assert hip._lib.xmca_complexify_theta(hip._h, _hip._ptr(col3), _hip._ptr(hbar), _hip._ptr(B), period) == _hip.ERR_INVALID


# ---- through the class ------------------------------------------------------------------------------------------------------------
T_CLS, M_CLS = 25, 4


def _class_fields(two=True, nan=False, dtype=np.float64):
    """130 and 65 grid points; the constant ones are left out (rotate() and normalize() divide by a grid point's norm - the
    all-zero column is fitted in the tests above)."""
    left = tc.columns(T_CLS, 156, M_CLS, seed=31)[:, np.arange(156) % 6 != 4] + 3.0
    right = tc.columns(T_CLS, 78, M_CLS, seed=32)[:, np.arange(78) % 6 != 4] * 2.0 - 1.0
    if nan:
        left = left.copy()
        left[3, 7] = np.nan
        left[:, 100] = np.nan
    out = (left, right) if two else (left,)
    return tuple(f.astype(dtype) for f in out)


def _restated(fields, m, normalize=False):
    """Centred kept columns (as the constructor leaves them) and their restated analytic signals."""
    real, signals = [], []
    for f in fields:
        x, _valid, _mean, std = ref_numpy.flatten_and_center(f)
        if normalize:
            x = x / std
        x = np.asarray(x, dtype=np.float64)
        real.append(x)
        signals.append(tc.analytic_signal(x, m))
    return real, signals


def _assert_solution(model, signals, n=4):
    ref = ref_numpy.solve(signals, complexify=False)
    s = model.singular_values(n)
    assert s.dtype == np.float64
    assert _rel(s, ref["singular_values"][:n]) < TOL
    phases = {}
    for side, k in enumerate(model._keys):
        V = model._V[k][:, :n]
        assert V.dtype == np.complex128
        Va, phases[k] = align_modes(V, ref["V"][side][:, :n])
        assert _rel(Va, ref["V"][side][:, :n]) < TOL, k
    return ref, phases


@pytest.mark.parametrize("preprocess", ["host", "device"])
@pytest.mark.parametrize("case", ["two_fields", "one_field_f32", "masked", "normalized"])
def test_solve_theta_matches_the_oracle(case, preprocess):
    fields = _class_fields(two=case != "one_field_f32", nan=case == "masked", dtype=np.float32 if case == "one_field_f32" else np.float64)
    model = MCA(*fields, preprocess=preprocess)
    if case == "normalized":
        model.normalize()
    model.solve(complexify=True, extend='theta', period=M_CLS)
    real, signals = _restated(fields, M_CLS, normalize=case == "normalized")
    ref, _ = _assert_solution(model, signals)
    # the fits and planes behind it: the device's own, against the restatement of the field the constructor made
    dev = model._device()
    for side, k in enumerate(model._keys):
        x = np.asarray(dev.get_field(side, real[side].shape, np.float64), dtype=np.float64)    # (centred / scaled as the device holds it)
        assert _rel(x, real[side]) < 1e-6
        _assert_fit_and_planes(dev.theta_fit(side, x.shape[1], M_CLS), dev.get_field_imag(side, x.shape), x, M_CLS, (case, preprocess, k))
    # fields(): the analytic signal the device solved
    got = model.fields()
    for side, k in enumerate(model._keys):
        full = got[k].reshape(T_CLS, -1)
        kept = ~np.isnan(full).any(axis=0)
        assert full.dtype == np.complex128 and kept.sum() == signals[side].shape[1]
        assert _rel(full[:, kept], signals[side]) < TOL, k
    model.rotate(4, 1)
    rot = ref_numpy.rotate(ref["V"], ref["singular_values"], 4, 1)
    assert _rel(model._variance, rot["variance"]) < TOL
    assert _rel(np.abs(model._rotation_matrix), np.abs(rot["R"])) < TOL          # R = D^H R_ref D: moduli are gauge-free


def test_no_host_extension_and_no_statsmodels(monkeypatch):
    import scipy.signal

    def boom(*a, **k):
        raise AssertionError("host extension / Hilbert transform called")
    monkeypatch.setattr(MCA, "_complexify", boom)
    monkeypatch.setattr(MCA, "_extend", boom)
    monkeypatch.setattr(MCA, "_theta_forecast", boom)
    monkeypatch.setattr(scipy.signal, "hilbert", boom)
    fields = _class_fields()
    model = MCA(*fields)
    model.solve(complexify=True, extend='theta', period=M_CLS)
    model.rotate(4, 1)
    assert model.pcs(4)['left'].shape == (T_CLS, 4) and model.eofs(4)['right'].shape == (65, 4)
    assert model.fields()['left'].dtype == np.complex128


def test_n_modes(hip):
    fields = _class_fields()
    _, signals = _restated(fields, M_CLS)
    model = MCA(*fields, handle=hip)
    model.solve(complexify=True, extend='theta', period=M_CLS, n_modes=3)
    assert len(model.singular_values()) == 3 and model._V['left'].shape[1] == 3
    _assert_solution(model, signals, n=3)


def test_predict(hip):
    fields = _class_fields(two=False)
    _, signals = _restated(fields, M_CLS)
    model = MCA(*fields, handle=hip)
    model.solve(complexify=True, extend='theta', period=M_CLS)
    ref, phases = _assert_solution(model, signals, n=4)
    model.rotate(4, 1)                                 # (predict mixes the n_rot rotated modes: the reference's formula, array.py:1299-1428)
    new = np.random.default_rng(8).standard_normal((7, 130)) + 3.0
    got = model.predict(new, n=3)['left']
    R = model.rotation_matrix(inverse_transpose=True)
    V = ref["V"][0][:, :4] * phases['left']            # the oracle's vectors in the model's gauge
    want = ((new - fields[0].mean(axis=0)) @ V / np.sqrt(ref["singular_values"][:4])) @ R
    assert _rel(got, want[:, model._var_idx][:, :3]) < TOL


def test_fields_after_another_model_used_the_handle(hip):
    fields = _class_fields(two=False)
    _, signals = _restated(fields, M_CLS)
    model = MCA(*fields, handle=hip)
    model.solve(complexify=True, extend='theta', period=M_CLS)
    other = MCA(*_class_fields(), handle=hip)
    other.solve(complexify=True)
    assert _rel(model.fields()['left'], signals[0]) < TOL              # extended again on the device, not on the host
    _assert_solution(model, signals)


def test_bootstrapping_runs_every_replicate_on_the_device(hip):
    fields = _class_fields(two=False)
    model = MCA(*fields, handle=hip)
    model.solve(complexify=True, extend='theta', period=M_CLS)
    np.random.seed(5)
    got = model.bootstrapping(3, n_modes=4, on_left=True, block_size=5)
    # the reference's loop on the same draws, every replicate by the restatement and the oracle
    x = ref_numpy.flatten_and_center(fields[0])[0]
    np.random.seed(5)
    want = np.zeros((4, 3))
    for run in range(3):
        x = block_bootstrap(x, axis=0, block_size=5, replace=True)
        signal = tc.analytic_signal(x - x.mean(axis=0), M_CLS)
        want[:, run] = ref_numpy.solve([signal])["singular_values"][:4]
    assert _rel(got, want) < TOL


def test_through_the_xarray_facade():
    try:
        import xarray as xr
    except Exception:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
        import xarray as xr
    from xmca_amd.xarray import xMCA
    nlat, nlon = 10, 13                                  # (130 grid points)
    values = _class_fields(two=False)[0]
    field = xr.DataArray(values.reshape(T_CLS, nlat, nlon), dims=["time", "lat", "lon"],
                         coords={"time": np.arange(T_CLS), "lat": np.linspace(-45.0, 45.0, nlat), "lon": np.linspace(0.0, 120.0, nlon)})
    model = xMCA(field)
    model.solve(complexify=True, extend='theta', period=M_CLS)
    _, signals = _restated((values,), M_CLS)
    ref = ref_numpy.solve(signals)
    assert _rel(np.asarray(model.singular_values(4).values), ref["singular_values"][:4]) < TOL
    assert model.pcs(3)['left'].shape == (T_CLS, 3) and model.eofs(3)['left'].shape == (nlat, nlon, 3)
