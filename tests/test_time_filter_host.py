"""CPU: `xmca_amd.prepare.lanczos_weights` / `time_filter` without a device - the weights of Duchon (1979), every
argument rule on a handle stub that fails on any device call, the self-checks of the numpy restatement the GPU tests compare with
(tests/time_filter_cases.py), the two ABI entries, and the xarray wrapper."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

import time_filter_cases as C
from abi_cases import check_entry, header_abi_version, header_text
from xmca_amd import _hip, prepare
from xmca_amd.prepare import lanczos_weights, time_filter

try:
    import xarray as xr                      # the real package, where it exists
except Exception:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
    import xarray as xr

from xmca_amd import xarray as facade

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"xmca_time_filter": 16, "xmca_time_filter_tile": 3}


class _NoDevice:
    """a handle that fails the test when anything reaches it"""

    def __getattr__(self, name):
        raise AssertionError("device touched: " + name)


def _field(T=40, N=5, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, N)) + 10.0
    X[rng.random((T, N)) < 0.2] = np.nan
    return X


def _filt(X, w=None, **kw):
    return time_filter(X, lanczos_weights(5, 0.2) if w is None else w, handle=_NoDevice(), **kw)


# ---- lanczos_weights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 3, 25, 61, 121, 1025])
@pytest.mark.parametrize("cutoff", [0.02, 0.1, 1.0 / 3.0, (0.05, 0.2), (0.1, 0.4)], ids=str)
def test_the_weights_sum_to_one_or_zero_and_are_symmetric(L, cutoff):
    w = lanczos_weights(L, cutoff)
    assert w.shape == (L,) and w.dtype == np.float64 and np.isfinite(w).all()
    want = 0.0 if isinstance(cutoff, tuple) else 1.0
    assert abs(float(np.sum(w.astype(np.longdouble)) - want)) <= 1e-15 * np.sum(np.abs(w))
    assert np.array_equal(w, w[::-1])


def test_one_weight_is_the_identity_and_the_formula_is_duchons():
    assert np.array_equal(lanczos_weights(1, 0.3), [1.0])
    L, fc = 9, 0.15
    h = 4
    j = np.arange(-h, h + 1).astype(float)
    raw = np.where(j == 0, 2 * fc, np.sin(2 * np.pi * fc * np.where(j == 0, 1, j)) / (np.pi * np.where(j == 0, 1, j))
                   * np.sin(np.pi * np.where(j == 0, 1, j) / (h + 1)) / (np.pi * np.where(j == 0, 1, j) / (h + 1)))
    assert np.max(np.abs(lanczos_weights(L, fc) - raw / raw.sum())) < 1e-16
    band = lanczos_weights(L, (0.1, 0.3))
    assert np.max(np.abs(band - (lanczos_weights(L, 0.3) - lanczos_weights(L, 0.1)))) < 1e-16


@pytest.mark.parametrize("L", [61, 121, 1025])
@pytest.mark.parametrize("fc", [0.05, 0.1, 0.25])
def test_the_response_is_a_half_at_the_cutoff_one_in_the_pass_band_and_zero_in_the_stop_band(L, fc):
    w = lanczos_weights(L, fc)
    assert abs(C.response(w, fc) - 0.5) <= 0.05
    assert abs(C.response(w, 0.0) - 1.0) < 1e-12 and abs(C.response(w, fc / 4) - 1.0) < 0.02
    for f in (min(2.0 * fc, 0.45), 0.5):
        assert abs(C.response(w, f)) < 0.02, f
    lo, hi = fc / 2, fc + 0.15
    band = lanczos_weights(L, (lo, hi))
    assert abs(C.response(band, 0.0)) < 1e-12 and abs(C.response(band, (lo + hi) / 2) - 1.0) < 0.02 and abs(C.response(band, 0.5)) < 0.02
    assert abs(C.response(band, lo) - 0.5) <= 0.05 and abs(C.response(band, hi) - 0.5) <= 0.05


@pytest.mark.parametrize("args", [
    (0, 0.1), (2, 0.1), (1027, 0.1), (5.0, 0.1), (True, 0.1), ("5", 0.1), (5, 0.0), (5, 0.5), (5, -0.1), (5, 0.7), (5, np.nan), (5, "0.1"),
    (5, None), (5, True), (5, (0.1,)), (5, (0.1, 0.2, 0.3)), (5, (0.2, 0.1)), (5, (0.1, 0.1)), (5, (0.0, 0.2)), (5, (0.1, 0.5)),
    (5, ((0.1, 0.2), (0.1, 0.2)))], ids=str)
def test_bad_weight_arguments_raise(args):
    with pytest.raises(ValueError, match="lanczos_weights"):
        lanczos_weights(*args)


# ---- time_filter: argument rules ------------------------------------------------------------------------------------------------
def test_bad_fields_raise_before_any_device_work():
    with pytest.raises(ValueError, match="float"):
        _filt(np.arange(24).reshape(6, 4))
    with pytest.raises(ValueError, match="float"):
        _filt(_field().astype(np.complex128))
    with pytest.raises(ValueError, match="float"):
        _filt(_field().astype(np.float16))
    with pytest.raises(ValueError, match="spatial"):
        _filt(np.arange(6.0))
    with pytest.raises(ValueError, match="time first"):
        _filt(np.float64(3.0))
    with pytest.raises(ValueError, match="empty"):
        _filt(np.zeros((6, 0)))
    for inf in (np.inf, -np.inf):
        X = _field()
        X[3, 2] = inf
        with pytest.raises(ValueError, match="Inf"):
            _filt(X)


def test_bad_weights_raise_before_any_device_work():
    X = _field()
    for bad, match in ((np.ones(4), "odd"), (np.ones(0), "odd"), (np.ones(1027), "at most 1025"), (np.ones((3, 3)), "vector"),
                       (np.ones(3, dtype=complex), "real"), (np.array(["a", "b", "c"]), "real"), (1.0, "vector"),
                       (np.array([1.0, np.nan, 1.0]), "NaN or an Inf"), (np.array([1.0, np.inf, 1.0]), "NaN or an Inf")):
        with pytest.raises(ValueError, match=match):
            _filt(X, bad)


def test_bad_options_raise_before_any_device_work():
    X = _field()
    for kw, match in ((dict(complement=1), "complement"), (dict(complement=None), "complement"), (dict(missing="skip"), "missing"),
                      (dict(missing=None), "missing"), (dict(missing="renormalize"), "missing"), (dict(edges="reflect"), "edges"),
                      (dict(edges=None), "edges"), (dict(missing="renormalise", edges="trim"), "edges='nan'"),
                      (dict(missing="renormalise", min_weight=0.0), "min_weight"), (dict(missing="renormalise", min_weight=1.5), "min_weight"),
                      (dict(missing="renormalise", min_weight=-0.5), "min_weight"), (dict(missing="renormalise", min_weight=None), "min_weight"),
                      (dict(missing="renormalise", min_weight=np.nan), "min_weight"), (dict(missing="renormalise", min_weight=True), "min_weight")):
        with pytest.raises(ValueError, match=match):
            _filt(X, **kw)
    with pytest.raises(ValueError, match="sum"):                   # band-pass weights cannot be renormalised
        _filt(X, lanczos_weights(5, (0.1, 0.3)), missing="renormalise")
    with pytest.raises(ValueError, match="sum"):
        _filt(X, -lanczos_weights(5, 0.2), missing="renormalise")
    with pytest.raises(ValueError, match="as many time steps"):    # a record shorter than the filter cannot be trimmed
        _filt(X[:4], edges="trim")


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
        _filt(tensor)


def test_valid_arguments_reach_the_handle_and_nothing_else_does():
    for kw in (dict(), dict(complement=True), dict(edges="trim"), dict(missing="renormalise"), dict(missing="renormalise", min_weight=1),
               dict(missing="renormalise", min_weight=1e-3, complement=True)):
        with pytest.raises(AssertionError, match="device touched: time_filter"):
            _filt(_field(), **kw)
    with pytest.raises(AssertionError, match="device touched: time_filter"):
        _filt(_field().astype(np.float32).reshape(40, 5, 1), [0.25, 0.5, 0.25])
    with pytest.raises(AssertionError, match="device touched: time_filter"):
        _filt(_field(T=5), edges="trim")                            # T == L is enough
    with pytest.raises(AssertionError, match="device touched: time_filter"):
        _filt(_field(T=3))                                          # shorter than the filter: all NaN, not an error
    with pytest.raises(AssertionError, match="device touched: time_filter"):
        _filt(_field(), np.arange(1025.0))


class _Recorder:
    """a handle that records what `time_filter` hands over and answers with zeros of the right shape"""
    device = 0

    def time_filter(self, X, w, **kw):
        self.got = dict(kw, w=w)
        T = X.shape[0] - (len(w) - 1 if kw["trim"] else 0)
        return np.zeros((T, X.shape[1]), dtype=X.dtype)


def test_the_threshold_is_formed_once_on_the_host():
    rec = _Recorder()
    w = C.case_weights(C.CASES[2])
    out = time_filter(_field(), w, missing="renormalise", min_weight=0.3, handle=rec)
    assert out.shape == (40, 5) and rec.got["renormalise"] and not rec.got["trim"] and rec.got["alloc"] is None
    assert rec.got["den_min"] == float(np.float64(0.3) * np.float64(C.weight_sum(w))) and rec.got["w"].dtype == np.float64
    out = time_filter(_field().reshape(40, 5, 1).astype(np.float32), [1, 2, 3, 4, 5], edges="trim", complement=True, handle=rec)
    assert out.shape == (36, 5, 1) and out.dtype == np.float32 and rec.got["trim"] and rec.got["complement"] and rec.got["den_min"] == 0.0


def test_the_constants_are_those_of_the_kernel():
    assert prepare.MAX_WEIGHTS == 1025
    src = open(os.path.join(REPO, "xmca_amd", "csrc", "time_filter.h")).read()
    assert re.search(r"TF_MAX_WEIGHTS\s*=\s*1025\b", src) and re.search(r"TF_COLS\s*=\s*256\b", src)
    assert "atomic" not in re.sub(r"//.*", "", src)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_shapes_the_kernel_takes_another_path_at():
    rows, cols, most = _hip.time_filter_tile()
    assert (rows, cols, most) == (C.R, C.C, 1025)
    Ts, Ns, Ls = ({c[i] for c in C.CASES} for i in (1, 2, 3))
    assert {rows - 1, rows, rows + 1, 2 * rows + 1} <= Ts and Ns >= {1, cols - 1, cols, cols + 1, 4 * cols + 1}
    assert Ls == {1, 3, 2 * rows + 1, most}
    assert any(c[3] == most and c[1] > most for c in C.CASES) and any(c[3] == most and c[1] < most for c in C.CASES)
    assert any(c[1] < c[3] for c in C.CASES if c[3] < most)                              # a record shorter than its filter
    assert {c[5] for c in C.CASES} == set(C.PATTERNS) and {c[4] for c in C.CASES} == {"sym", "asym", "band"}
    assert {m for c in C.CASES for m in c[7]} == set(C.MODES)
    for c in C.CASES:
        assert "n" not in c[7] or c[1] >= c[3], c[0]
        w = C.case_weights(c)
        assert w.size == c[3] and (c[4] == "band" or abs(w.sum() - 1.0) < 1e-12)
        assert np.array_equal(w, w[::-1]) == (c[4] != "asym" or c[3] == 1), c[0]
    run = next(c for c in C.CASES if c[5] == "run")
    gaps = np.isnan(C.case_field(run))
    assert max(np.diff(np.flatnonzero(np.r_[True, ~gaps[:, 0], True])).max() - 1, 0) > run[3]      # the run is longer than L


def test_the_restatement_is_a_correlation_not_a_convolution():
    """gap-free columns, asymmetric weights: rows h : T - h are np.convolve(x, w[::-1], 'valid') - a reversed tap order would show"""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((50, 4))
    for L in (1, 3, 9, 33):
        w = rng.uniform(0.1, 1.0, L) * np.where(np.arange(L) % 4 == 1, -0.2, 1.0)          # asymmetric, mixed signs, positive sum
        got = C.restate(X, w)
        h = L // 2
        assert np.isnan(got[:h]).all() and np.isnan(got[50 - h:]).all()
        for n in range(4):
            want = np.convolve(X[:, n], w[::-1], "valid")
            assert np.max(np.abs(got[h:50 - h, n] - want)) < 1e-14
            if L > 1:
                assert np.max(np.abs(got[h:50 - h, n] - np.convolve(X[:, n], w, "valid"))) > 1e-3
        assert np.array_equal(C.restate(X, w, edges="trim"), got[h:50 - h])
        assert np.array_equal(C.restate(X, w, complement=True, edges="trim"), X[h:50 - h] - got[h:50 - h])
        # with nothing missing away from the edges the renormalised smoother is the strict one over the sum of the weights
        full = C.restate(X, w / w.sum(), missing="renormalise")
        assert np.max(np.abs(full[h:50 - h] - got[h:50 - h] / w.sum())) < 1e-13 and np.isfinite(full[h:50 - h]).all()


@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
def test_the_nan_rules_of_the_restatement(case):
    name, T, N, L, kind, pattern, min_weight, modes = case
    X, w, h = C.case_field(case), C.case_weights(case), L // 2
    gaps = np.isnan(X)
    strict = C.restate(X, w)
    for t in range(T):                       # any of the L entries missing or outside the record
        want = gaps[max(t - h, 0):t + h + 1].any(axis=0) | (t - h < 0) | (t + h > T - 1)
        assert np.array_equal(np.isnan(strict[t]), want), t
    if "n" in modes:
        assert np.array_equal(C.restate(X, w, edges="trim"), strict[h:T - h], equal_nan=True)
    if "r" in modes:
        ren = C.restate(X, w, missing="renormalise", min_weight=min_weight)
        assert np.isnan(ren[gaps]).all()                              # a missing entry stays missing
        assert np.isfinite(ren[~gaps]).mean() > 0.5                   # ... and most of the rest is filled in
        assert np.array_equal(np.isnan(ren), C.expected_nan(name, "float64", True))


@pytest.mark.parametrize("case", [c for c in C.CASES if "r" in c[7]], ids=C.case_name)
def test_no_nan_decision_of_a_renormalise_case_sits_on_the_threshold(case):
    """min |den - den_min| >= 1e-9 sum |w| over all entries, in longdouble: the float64 chain of the denominators (errors of
    L 2^-53 sum |w| at the most) decides every entry as the exact one does, so the GPU tests compare NaN masks exactly"""
    for dtype in C.DTYPES:
        assert C.threshold_margin(case, dtype) >= 1e-9, dtype


def test_the_bound_covers_the_float64_restatement():
    """the restatement rounds twice per tap where the bound allows for one rounding: still inside it, and not by orders of magnitude"""
    for case in C.CASES[:11]:
        X, w = C.case_field(case), C.case_weights(case)
        for m in case[7]:
            for comp in (False, True):
                isnan, y, bound = C.reference(case, m, comp, "float64")
                got = C.restate(X, w, complement=comp, min_weight=case[6], **C.MODES[m])
                assert np.array_equal(np.isnan(got), isnan), (case[0], m, comp)
                assert C.worst_ratio(got, isnan, y, bound) <= 1.0, (case[0], m, comp)


# ---- ABI and facade -------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entries_and_the_binding_has_them():
    for name, n_args in NEW.items():
        check_entry(name, n_args)
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version()
    text = header_text(comments=True)                 # (the stage names stand in a comment)
    for stage in ("time_filter", "ingest_strided"):
        assert '"%s"' % stage in text, stage
    assert callable(_hip.Handle.time_filter)
    lib = _hip.load_library()
    import ctypes
    a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert lib.xmca_time_filter_tile(ctypes.byref(a), ctypes.byref(b), None) == _hip.ERR_INVALID
    assert lib.xmca_time_filter_tile(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0 and (a.value, b.value, c.value) == (16, 256, 1025)


def test_the_package_does_not_export_the_module():
    import xmca_amd
    assert "time_filter" not in xmca_amd.__all__ and "lanczos_weights" not in xmca_amd.__all__


def test_the_xarray_wrapper_has_the_parameters_of_time_filter():
    a = inspect.signature(time_filter).parameters
    b = inspect.signature(facade.time_filter).parameters
    assert list(a)[1:] == list(b)[1:] and list(b)[0] == "da"
    for name in list(a)[1:]:
        assert a[name].default == b[name].default and a[name].kind == b[name].kind, name


def test_the_xarray_wrapper_checks_before_the_device_and_wraps_the_field():
    da = xr.DataArray(_field(T=24, N=6).reshape(24, 2, 3), dims=["time", "lat", "lon"],
                      coords={"time": np.arange(100, 124), "lat": [0.0, 1.0], "lon": [0.0, 1.0, 2.0]}, name="sst", attrs={"units": "K"})
    w = lanczos_weights(7, 0.2)
    with pytest.raises(ValueError, match="odd"):
        facade.time_filter(da, np.ones(4), handle=_NoDevice())
    with pytest.raises(AssertionError, match="device touched: time_filter"):
        facade.time_filter(da, w, handle=_NoDevice())
    with pytest.raises(TypeError, match="DataArray"):
        facade.time_filter(da.values, w, handle=_NoDevice())
    out = facade.time_filter(da, w, handle=_Recorder())
    assert tuple(out.dims) == ("time", "lat", "lon") and out.shape == (24, 2, 3) and out.name == "sst" and dict(out.attrs) == {"units": "K"}
    assert np.array_equal(np.asarray(out.coords["time"].values), np.arange(100, 124))
    out = facade.time_filter(da, w, edges="trim", handle=_Recorder())
    assert tuple(out.dims) == ("time", "lat", "lon") and out.shape == (18, 2, 3) and out.name == "sst"
    assert np.array_equal(np.asarray(out.coords["time"].values), np.arange(103, 121))
    assert np.array_equal(np.asarray(out.coords["lon"].values), [0.0, 1.0, 2.0])
    assert np.array_equal(np.asarray(da.coords["time"].values), np.arange(100, 124))          # the input keeps its coordinates
