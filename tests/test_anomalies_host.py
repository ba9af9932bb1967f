"""CPU: `xmca_amd.prepare` without a device - every argument rule on a handle stub that fails on any device call,
the columns of `time_basis` and their continuation, the self-checks of the numpy restatement the GPU tests compare with
(tests/anomalies_cases.py), the five ABI entries, and the xarray wrapper."""
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

import anomalies_cases as C
from abi_cases import check_entry, header_abi_version, header_text
from xmca_amd import _hip, prepare
from xmca_amd.prepare import anomalies, remove, time_basis

try:
    import xarray as xr                      # the real package, where it exists
except Exception:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
    import xarray as xr

from xmca_amd import xarray as facade

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"xmca_column_regress": 14, "xmca_column_residual": 13, "xmca_reg_mask": 8, "xmca_reg_solve": 8, "xmca_reg_residual_tile": 2}


class _NoDevice:
    """a handle that fails the test when anything reaches it"""

    def __getattr__(self, name):
        raise AssertionError("device touched: " + name)


def _field(T=24, N=5, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, N)) + 10.0
    X[rng.random((T, N)) < 0.2] = np.nan
    return X


def _anom(X, **kw):
    return anomalies(X, handle=_NoDevice(), **kw)


# ---- time_basis ---------------------------------------------------------------------------------------------------------------
def test_the_constant_the_phase_means_and_the_harmonics():
    assert np.array_equal(time_basis(5), np.ones((5, 1)))
    B = time_basis(7, period=3)
    assert B.shape == (7, 3) and B.dtype == np.float64
    assert np.array_equal(B, np.eye(3)[np.arange(7) % 3])
    B = time_basis(30, period=12, harmonics=2)
    t = np.arange(30)
    want = np.stack([np.ones(30), np.cos(2 * np.pi * t / 12), np.sin(2 * np.pi * t / 12), np.cos(4 * np.pi * t / 12),
                     np.sin(4 * np.pi * t / 12)], axis=1)
    assert B.shape == (30, 5) and np.max(np.abs(B - want)) < 1e-14
    assert np.array_equal(B[:12], B[12:24])                       # (the angle is taken of t mod period: exactly periodic)


def test_the_trend_column_is_centred_and_scaled_by_the_span():
    B = time_basis(10, trend=True)
    assert B.shape == (10, 2) and np.array_equal(B[:, 1], (np.arange(10) - 4.5) / 10)
    B = time_basis(4, period=2, trend=True, start=3, span=8)
    assert np.array_equal(B[:, :2], np.eye(2)[np.arange(3, 7) % 2]) and np.array_equal(B[:, 2], (np.arange(3, 7) - 3.5) / 8)


@pytest.mark.parametrize("kw", [dict(), dict(period=12), dict(period=12, harmonics=3), dict(period=5, trend=True)], ids=str)
def test_start_continues_a_basis_when_span_is_the_same(kw):
    T = 17
    both = dict(kw, span=2 * T) if kw.get("trend") else kw
    whole = time_basis(2 * T, **kw)
    assert np.array_equal(np.vstack([time_basis(T, **both), time_basis(T, start=T, **both)]), whole)


def test_the_cap_is_sixteen_columns():
    assert time_basis(20, period=12, trend=True).shape[1] == 13
    assert time_basis(40, period=365, harmonics=7, trend=True).shape[1] == 16
    assert time_basis(20, period=16).shape[1] == 16
    for kw in (dict(period=17), dict(period=16, trend=True), dict(period=365, harmonics=8)):
        with pytest.raises(ValueError, match="at most 16"):
            time_basis(20, **kw)


@pytest.mark.parametrize("kw, match", [
    (dict(n_steps=0), "n_steps"), (dict(n_steps=2.0), "n_steps"), (dict(n_steps=True), "n_steps"), (dict(period=0), "period"),
    (dict(period=12.0), "period"), (dict(period="12"), "period"), (dict(harmonics=2), "harmonics need a period"),
    (dict(period=12, harmonics=0), "harmonics"), (dict(period=12, harmonics=6), "harmonics"), (dict(period=4, harmonics=2), "harmonics"),
    (dict(period=12, harmonics=1.0), "harmonics"), (dict(trend=1), "trend"), (dict(trend=None), "trend"), (dict(start=-1), "start"),
    (dict(start=1.5), "start"), (dict(trend=True, span=0), "span"), (dict(trend=True, span=2.5), "span"), (dict(span=10), "span")], ids=str)
def test_bad_basis_arguments_raise(kw, match):
    kw = dict(dict(n_steps=10), **kw)
    with pytest.raises(ValueError, match=match):
        time_basis(**kw)


# ---- anomalies / remove: argument rules ---------------------------------------------------------------------------------------
def test_bad_fields_raise_before_any_device_work():
    with pytest.raises(ValueError, match="float"):
        _anom(np.arange(24).reshape(6, 4))
    with pytest.raises(ValueError, match="float"):
        _anom(_field().astype(np.complex128))
    with pytest.raises(ValueError, match="float"):
        _anom(_field().astype(np.float16))
    with pytest.raises(ValueError, match="spatial"):
        _anom(np.arange(6.0))
    with pytest.raises(ValueError, match="time first"):
        _anom(np.float64(3.0))
    with pytest.raises(ValueError, match="empty"):
        _anom(np.zeros((6, 0)))
    for inf in (np.inf, -np.inf):
        X = _field()
        X[3, 2] = inf
        with pytest.raises(ValueError, match="Inf"):
            _anom(X)
        with pytest.raises(ValueError, match="Inf"):
            remove(X, time_basis(24), np.zeros((1, 5)), handle=_NoDevice())


def test_bad_basis_choices_raise_before_any_device_work():
    X = _field()
    with pytest.raises(ValueError, match="at most 16"):
        _anom(X, period=17)                                       # k = 17 is refused
    with pytest.raises(ValueError, match="harmonics"):
        _anom(X, period=12, harmonics=6)
    with pytest.raises(ValueError, match="not both"):
        _anom(X, period=12, basis=np.ones((24, 1)))
    with pytest.raises(ValueError, match="not both"):
        _anom(X, trend=True, basis=np.ones((24, 1)))
    with pytest.raises(ValueError, match="rows"):
        _anom(X, basis=np.ones((23, 2)))
    with pytest.raises(ValueError, match="columns"):
        _anom(X, basis=np.ones((24, 17)))
    with pytest.raises(ValueError, match="columns"):
        _anom(X, basis=np.ones((24, 0)))
    with pytest.raises(ValueError, match=r"\(T, k\)"):
        _anom(X, basis=np.ones(24))
    with pytest.raises(ValueError, match="real"):
        _anom(X, basis=np.ones((24, 2), dtype=complex))
    for bad in (np.nan, np.inf):
        B = np.ones((24, 2))
        B[3, 1] = bad
        with pytest.raises(ValueError, match="NaN or an Inf"):
            _anom(X, basis=B)


def test_bad_models_raise_before_any_device_work():
    X, B = _field(), time_basis(24, period=12)
    with pytest.raises(ValueError, match="shape"):
        remove(X, B, np.zeros((11, 5)), handle=_NoDevice())
    with pytest.raises(ValueError, match="shape"):
        remove(X.reshape(24, 5, 1), B, np.zeros((12, 5)), handle=_NoDevice())
    with pytest.raises(ValueError, match="rows"):
        remove(X, B[:20], np.zeros((12, 5)), handle=_NoDevice())
    with pytest.raises(ValueError, match="real"):
        remove(X, B, np.zeros((12, 5), dtype=complex), handle=_NoDevice())
    C_ = np.zeros((12, 5))
    C_[0, 0] = np.inf
    with pytest.raises(ValueError, match="Inf"):
        remove(X, B, C_, handle=_NoDevice())


def test_a_host_tensor_is_refused_with_advice(monkeypatch):
    try:
        import torch
        tensor = torch.zeros(6, 4, dtype=torch.float64)
    except Exception:          # no torch here: a tensor is whatever the imported `torch` module calls Tensor
        import types
        torch = types.ModuleType("torch")

        class Tensor:
            shape = (6, 4)
            device = types.SimpleNamespace(type="cpu", index=None)

            def dim(self):
                return 2
        torch.Tensor = Tensor
        monkeypatch.setitem(sys.modules, "torch", torch)
        tensor = torch.Tensor()
    with pytest.raises(ValueError, match="handle's GPU"):
        _anom(tensor)


def test_valid_arguments_reach_the_handle_and_nothing_else_does():
    with pytest.raises(AssertionError, match="device touched: column_regress"):
        _anom(_field(), period=12, trend=True)
    with pytest.raises(AssertionError, match="device touched: column_regress"):
        _anom(_field().astype(np.float32).reshape(24, 5, 1), basis=np.ones((24, 1)))
    coef = np.zeros((12, 5))
    coef[:, 2] = np.nan                          # (a grid point that was not fitted)
    with pytest.raises(AssertionError, match="device touched: column_residual"):
        remove(_field(), time_basis(24, period=12), coef, handle=_NoDevice())


def test_the_docstring_states_the_definiteness_criterion():
    doc = " ".join(anomalies.__doc__.split())
    assert "every pivot" in doc and "1e-8" in doc and "order of the basis columns" in doc
    assert prepare.PIVOT_MIN == C.PIVOT_MIN == 1e-8 and prepare.MAX_COLUMNS == 16
    src = open(os.path.join(REPO, "xmca_amd", "csrc", "regress.h")).read()
    assert re.search(r"REG_PIVOT_MIN\s*=\s*1e-8\b", src) and re.search(r"REG_K\s*=\s*16\b", src)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_shapes_the_kernels_take_another_path_at():
    rows, cols = _hip.reg_residual_tile()
    Ts, Ns, ks = ({c[i] for c in C.CASES} for i in range(3))
    assert Ts == {17, 33, 49, 130} and Ns == {1, 63, 64, 65, 257} and ks == {1, 2, 6, 13, 16} == set(C.BASES)
    assert max(Ts) > 2 * rows and min(Ts) < rows and max(Ns) > cols and {63, 64, 65} <= Ns
    for k, kw in C.BASES.items():
        assert time_basis(40, **kw).shape[1] == k


@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
def test_the_expected_mask_follows_from_counts_and_the_restatement_agrees(case):
    B = C.basis_of(case)
    for pattern in C.patterns_of(case):
        X, expected = C.case_field(case, pattern)
        assert np.array_equal(expected, C.expected_fitted(case, X)), pattern
        field, coef, fitted = C.reference(case, pattern)
        assert np.array_equal(fitted, expected), pattern
        assert np.array_equal(np.isnan(field[:, fitted]), np.isnan(X[:, fitted])) and np.isnan(field[:, ~fitted]).all()
        assert np.isfinite(coef[:, fitted]).all() and np.isnan(coef[:, ~fitted]).all()
        for n in np.flatnonzero(expected):          # far from the threshold: rounding cannot move a column across it
            p = np.isfinite(X[:, n])
            assert C.pivot_shares(B[p].T @ B[p]).min() >= C.PIVOT_FLOOR, (pattern, n)
        for n in np.flatnonzero(~expected):         # ... and a refused column fails by a count or by an exact zero
            p = np.isfinite(X[:, n])
            assert p.sum() < case[2] or C.pivot_shares(B[p].T @ B[p])[5] == 0.0, (pattern, n)


def test_the_normal_equations_agree_with_lstsq_in_numpy():
    """the route the device takes, in numpy float64, against the restatement's lstsq: 5.2e-15 of max|X| at these shapes"""
    worst = 0.0
    for case in [c for c in C.CASES if c[2] >= 6]:
        X, _ = C.case_field(case, "random")
        B = C.basis_of(case)
        field, coef, fitted = C.reference(case, "random")
        for n in np.flatnonzero(fitted):
            p = np.isfinite(X[:, n])
            c = np.linalg.solve(B[p].T @ B[p], B[p].T @ X[p, n])
            worst = max(worst, np.max(np.abs(X[p, n] - B[p] @ c - field[p, n])) / np.nanmax(np.abs(X)))
    assert worst < 1e-13, worst


def test_float32_inputs_are_widened_fitted_in_float64_and_rounded_once():
    case = (33, 64, 13)
    X32, _ = C.case_field(case, "random", "float32")
    f32, c32, _ = C.reference(case, "random", "float32")
    f64, c64, _ = C.restate(X32.astype(np.float64), C.basis_of(case))
    assert f32.dtype == np.float32 and np.array_equal(c32, c64) and np.array_equal(f32, f64.astype(np.float32), equal_nan=True)


def test_the_bounds_of_the_gpu_tests_are_those_of_the_profile():
    import test_gpu_anomalies as G
    prof = json.load(open(os.path.join(REPO, "profiles", "anomalies_accuracy.json")))
    assert G.BOUND64 == pytest.approx(8 * prof["worst"]["field_float64"], rel=1e-3) and G.BOUND64 < 1e-11
    assert G.BOUND64 == pytest.approx(prof["bounds"]["float64_of_max_abs_X"], rel=1e-3)
    assert G.BOUND32_ULPS == prof["bounds"]["float32_ulps_of_max_abs_X"] >= prof["worst"]["field_float32"]


# ---- ABI and facade -------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entries_and_the_binding_has_them():
    for name, n_args in NEW.items():
        check_entry(name, n_args)
    assert header_abi_version() == _hip.ABI_VERSION == 16
    text = header_text(comments=True)                 # (the stage names stand in a comment)
    for stage in ("reg_mask", "reg_moments", "reg_solve", "reg_residual"):
        assert '"%s"' % stage in text, stage
    for method in ("column_regress", "column_residual", "reg_mask", "reg_solve"):
        assert callable(getattr(_hip.Handle, method))
    assert _hip.reg_residual_tile() == (64, 256)


def test_the_package_does_not_export_the_module():
    import xmca_amd
    assert "anomalies" not in xmca_amd.__all__ and "prepare" not in xmca_amd.__all__


def test_the_xarray_wrapper_has_the_parameters_of_anomalies():
    a = inspect.signature(anomalies).parameters
    b = inspect.signature(facade.anomalies).parameters
    assert list(a)[1:] == list(b)[1:] and list(b)[0] == "da"
    for name in list(a)[1:]:
        assert a[name].default == b[name].default and a[name].kind == b[name].kind, name


class _Recorder:
    """a handle that answers column_regress with zeros of the right shapes"""
    device = 0

    def column_regress(self, X, B, alloc=None):
        return np.zeros_like(X), np.zeros((B.shape[1], X.shape[1])), np.ones(X.shape[1], dtype=bool)


def test_the_xarray_wrapper_checks_before_the_device_and_wraps_the_dict():
    da = xr.DataArray(_field(T=24, N=6).reshape(24, 2, 3), dims=["time", "lat", "lon"],
                      coords={"time": np.arange(24), "lat": [0.0, 1.0], "lon": [0.0, 1.0, 2.0]}, name="sst", attrs={"units": "K"})
    with pytest.raises(ValueError, match="at most 16"):
        facade.anomalies(da, period=17, handle=_NoDevice())
    with pytest.raises(AssertionError, match="device touched: column_regress"):
        facade.anomalies(da, period=12, handle=_NoDevice())
    with pytest.raises(TypeError, match="DataArray"):
        facade.anomalies(da.values, period=12, handle=_NoDevice())
    out = facade.anomalies(da, period=12, trend=True, handle=_Recorder())
    assert tuple(out["field"].dims) == ("time", "lat", "lon") and out["field"].shape == (24, 2, 3) and out["field"].name == "sst"
    assert dict(out["field"].attrs) == {"units": "K"}
    assert tuple(out["coefficients"].dims) == ("basis", "lat", "lon") and out["coefficients"].shape == (13, 2, 3)
    assert tuple(out["fitted"].dims) == ("lat", "lon") and out["fitted"].values.dtype == bool
    assert tuple(out["basis"].dims) == ("time", "basis") and np.array_equal(out["basis"].values, time_basis(24, period=12, trend=True))
    assert np.array_equal(np.asarray(out["coefficients"].coords["lon"].values), [0.0, 1.0, 2.0])
    assert "time" not in out["coefficients"].coords and "lat" not in out["basis"].coords
