"""GPU: `xmca_amd.prepare.time_filter` - the one kernel of csrc/time_filter.h.  The numpy restatement, the longdouble
truth and the cases: tests/time_filter_cases.py (T around the R = 16 rows of a tile and on both sides of L, N in {1, C - 1, C, C + 1,
4 C + 1} around its C = 256 columns, L in {1, 3, 2 R + 1, 1025}; symmetric, asymmetric and band-pass weights; seven gap patterns).

Bounds.  NaN positions equal the restatement's exactly, every entry: no decision of a committed case sits on the threshold
(tests/test_time_filter_host.py).  Values stay within the bound `time_filter_cases.reference` computes per entry in longdouble,
nothing of it measured: 2 [(L + 4) 2^-53 (sum |w_k x| + |S| sum_present |w_k|) / |den| + 2^-53 (|x_t| + |y|)] - in strict mode den = 1
and the |S| sum |w| term absent - plus half a float32 spacing at |y| for a float32 field.  Worst error / bound measured on an MI355X
(profiles/time_filter_accuracy.json, written by scripts/time_filter_accuracy.py)."""
import numpy as np
import pytest

import time_filter_cases as C
from xmca_amd import _hip
from xmca_amd.array import MCA
from xmca_amd.prepare import lanczos_weights, time_filter

pytestmark = pytest.mark.gpu

RUNS = C.runs()


def _run_name(run):
    return "%s-%s-%s" % (run[0][0], run[1], "complement" if run[2] else "smooth")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _call(hip, case, mode, complement, dtype):
    return time_filter(C.case_field(case, dtype), C.case_weights(case), complement=complement, min_weight=case[6], handle=hip, **C.MODES[mode])


def test_the_cases_know_the_tile_of_the_library():
    rows, cols, most = _hip.time_filter_tile()
    Ts, Ns, Ls = ({c[i] for c in C.CASES} for i in (1, 2, 3))
    assert {rows - 1, rows, rows + 1, 2 * rows + 1} <= Ts and max(Ts) > most > min(Ts)
    assert {1, cols - 1, cols, cols + 1, 4 * cols + 1} <= Ns and Ls == {1, 3, 2 * rows + 1, most}


# ---- against the restatement and the longdouble truth ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("run", RUNS, ids=_run_name)
def test_against_the_restatement(hip, run, dtype):
    case, mode, complement = run
    name, T, N, L = case[:4]
    got = _call(hip, case, mode, complement, dtype)
    isnan, y, bound = C.reference(case, mode, complement, dtype)
    assert isinstance(got, np.ndarray) and got.dtype == np.dtype(dtype) and got.shape == ((T - (L - 1) if mode == "n" else T), N)
    assert np.array_equal(np.isnan(got), isnan)                      # every entry, exactly
    assert not np.isinf(got).any()
    ratio = C.worst_ratio(got, isnan, y, bound)
    print(_run_name(run), dtype, "live %d of %d" % ((~isnan).sum(), isnan.size), "error / bound %.3g" % ratio)
    assert ratio <= 1.0


# ---- checks that need no reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("L", [1, 3, 33, 121])
def test_a_constant_field_comes_back_under_normalised_low_pass_weights(hip, L, dtype):
    T, N = 150, 257
    X = np.full((T, N), 7.25, dtype=dtype)
    gaps = np.random.default_rng(L).random((T, N)) < 0.02
    X[gaps] = np.nan
    w = lanczos_weights(L, 0.1)
    tol = (L + 4) * 2.0 ** -52 * 7.25 * np.sum(np.abs(w)) * 2 + (np.spacing(np.float32(7.25)) if dtype == "float32" else 0.0)
    for kw in (dict(), dict(edges="trim"), dict(missing="renormalise", min_weight=0.3)):
        out = time_filter(X, w, handle=hip, **kw)
        live = ~np.isnan(out)
        assert live.any() and np.max(np.abs(out[live].astype(np.float64) - 7.25)) <= tol / (0.3 if "min_weight" in kw else 1.0), kw
        high = time_filter(X, w, complement=True, handle=hip, **kw)
        assert np.array_equal(np.isnan(high), ~live) and np.max(np.abs(high[live].astype(np.float64))) <= tol / (0.3 if "min_weight" in kw else 1.0)


@pytest.mark.parametrize("L, fc, f", [(33, 0.1, 0.04), (33, 0.1, 0.3), (121, 0.05, 0.05), (1025, 0.01, 0.004)])
def test_a_cosine_comes_back_scaled_by_the_response(hip, L, fc, f):
    T, N, h = 1100, 7, L // 2
    phase = np.linspace(0.0, 1.0, N)
    X = np.cos(2 * np.pi * (f * np.arange(T)[:, None] + phase[None, :]))
    w = lanczos_weights(L, fc)
    out = time_filter(X, w, handle=hip)
    assert np.isnan(out[:h]).all() and np.isnan(out[T - h:]).all()
    resp = C.response(w, f)
    tol_x = 4 * 2.0 ** -53 * 2 * np.pi * (f * T + 1) * np.sum(np.abs(w))          # the samples' own rounding: that of their arguments
    assert np.max(np.abs(out[h:T - h] - resp * X[h:T - h])) <= (L + 4) * 2.0 ** -52 * np.sum(np.abs(w)) + tol_x
    high = time_filter(X, w, complement=True, edges="trim", handle=hip)
    assert np.max(np.abs(high - (1.0 - resp) * X[h:T - h])) <= (L + 4) * 2.0 ** -52 * np.sum(np.abs(w)) + tol_x


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("case", [c for c in C.CASES if "n" in c[7]], ids=C.case_name)
def test_trim_is_the_interior_of_nan_to_the_bit_and_a_repeated_call_repeats_its_bits(hip, case, dtype):
    T, h = case[1], case[3] // 2
    for complement in (False, True):
        full = _call(hip, case, "s", complement, dtype)
        assert np.array_equal(_bits(_call(hip, case, "n", complement, dtype)), _bits(full[h:T - h]))
        assert np.array_equal(_bits(_call(hip, case, "s", complement, dtype)), _bits(full))
        if "r" in case[7]:
            assert np.array_equal(_bits(_call(hip, case, "r", complement, dtype)), _bits(_call(hip, case, "r", complement, dtype)))


def test_the_entry_point_refuses_bad_arguments_before_any_launch(hip):
    """XMCA_ERR_INVALID from the C entry itself (the Python layer checks the same things earlier); the handle stays usable"""
    X, w, out = np.ones((20, 3)), np.array([0.25, 0.5, 0.25] + [0.0] * 1030), np.empty((20, 3))
    p = _hip._ptr

    def call(T=20, N=3, stride_t=3, stride_n=1, dtype=_hip.XMCA_F64, L=3, renorm=0, den_min=0.0, trim=0, weights=w, where=_hip.HOST):
        return hip._lib.xmca_time_filter(hip._h, p(X), where, T, N, stride_t, stride_n, dtype, p(weights), L, 0, renorm, den_min, trim, p(out), _hip.HOST)
    assert call() == 0 and abs(out[5, 1] - 1.0) < 1e-15 and np.isnan(out[0]).all()
    bad_w, neg_w = w.copy(), -w
    bad_w[1] = np.nan
    for bad in (dict(L=0), dict(L=2), dict(L=1027), dict(L=-1), dict(T=0), dict(N=0), dict(dtype=7), dict(stride_t=-1), dict(stride_n=-1),
                dict(where=5), dict(weights=bad_w), dict(T=2, trim=1), dict(renorm=1, den_min=0.5, trim=1), dict(renorm=1, den_min=0.0),
                dict(renorm=1, den_min=1.5), dict(renorm=1, den_min=-0.5), dict(renorm=1, den_min=np.nan),
                dict(renorm=1, den_min=0.5, weights=neg_w)):
        assert call(**bad) == _hip.ERR_INVALID, bad
    with pytest.raises(ValueError, match="odd"):
        hip.time_filter(X, np.ones(4))
    assert call(renorm=1, den_min=0.5) == 0 and np.max(np.abs(out - 1.0)) < 1e-15


# ---- tensors -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("layout", ["contiguous", "transposed", "column slice", "three dimensions"])
def test_a_gpu_tensor_gives_a_gpu_tensor_with_the_bits_of_the_numpy_route(hip, layout, dtype):
    import torch
    case = next(c for c in C.CASES if c[0] == "halo-sparse")
    T, N = case[1], case[2]
    X, w = C.case_field(case, dtype), C.case_weights(case)
    dev = torch.device("cuda", hip.device)
    if layout == "contiguous":
        t = torch.from_numpy(X.copy()).to(dev)
    elif layout == "transposed":
        t = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev).T
        assert t.stride() == (1, T)
    elif layout == "column slice":
        wide = torch.full((T, N + 30), 7.0, dtype=getattr(torch, dtype), device=dev)
        wide[:, 10:10 + N] = torch.from_numpy(X.copy()).to(dev)
        t = wide[:, 10:10 + N]
        assert t.stride() == (N + 30, 1)
    else:
        X = X[:, :256]
        t = torch.from_numpy(X.copy()).to(dev).reshape(T, 16, 16)
    before = t.clone()
    for kw in (dict(), dict(edges="trim", complement=True), dict(missing="renormalise", min_weight=case[6])):
        want = time_filter(X, w, handle=hip, **kw)
        out = time_filter(t, w, handle=hip, **kw)
        assert isinstance(out, torch.Tensor) and out.device == dev and out.dtype == t.dtype and out.is_contiguous()
        assert tuple(out.shape) == (want.shape[0],) + tuple(t.shape[1:])
        assert np.array_equal(_bits(out.cpu().numpy().reshape(want.shape)), _bits(want))
    assert torch.equal(torch.nan_to_num(t, nan=-1.0), torch.nan_to_num(before, nan=-1.0))          # the input is unchanged


def test_a_tensor_with_an_inf_is_refused(hip):
    import torch
    t = torch.ones(20, 4, dtype=torch.float64, device=torch.device("cuda", hip.device))
    t[3, 1] = float("inf")
    with pytest.raises(ValueError, match="Inf"):
        time_filter(t, [0.25, 0.5, 0.25], handle=hip)


# ---- state and pipeline --------------------------------------------------------------------------------------------------------------
def test_a_solved_rotated_model_on_the_handle_keeps_its_result_to_the_bit(hip):
    rng = np.random.default_rng(11)
    F = rng.standard_normal((40, 6)) @ rng.standard_normal((6, 90)) + 0.1 * rng.standard_normal((40, 90))
    m = MCA(F, handle=hip)
    m.solve()
    m.rotate(3)
    before = (m.singular_values().copy(), m.eofs(3)['left'].copy(), m.pcs(3)['left'].copy())
    case = next(c for c in C.CASES if c[0] == "halo-sparse")
    hip.reset_timings()
    _call(hip, case, "s", False, "float64")
    _call(hip, case, "r", True, "float32")
    assert "time_filter" in set(hip.timings())
    for a, b in zip(before, (m.singular_values(), m.eofs(3)['left'], m.pcs(3)['left'])):
        assert np.array_equal(_bits(a), _bits(b))


def test_the_pipeline_time_filter_then_mca(hip):
    rng = np.random.default_rng(2)
    T, N, L = 120, 70, 25
    t = np.arange(T)[:, None]
    X = np.cos(2 * np.pi * 0.02 * t) * rng.standard_normal((1, N)) + np.cos(2 * np.pi * 0.3 * t) * rng.standard_normal((1, N)) \
        + 0.01 * rng.standard_normal((T, N))
    low = time_filter(X, lanczos_weights(L, 0.1), edges="trim", handle=hip)
    assert low.shape == (T - L + 1, N) and np.isfinite(low).all()
    m = MCA(low, handle=hip)
    m.solve()
    ev = m.explained_variance()
    assert ev[0] > 95.0                                # the slow wave alone is left: one mode carries the filtered field


# ---- xarray ----------------------------------------------------------------------------------------------------------------------------
def test_the_xarray_wrapper_returns_the_field_over_the_dims_of_the_input(hip):
    import os
    import sys
    try:
        import xarray as xr
    except Exception:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
        import xarray as xr
    from xmca_amd import xarray as facade
    case = next(c for c in C.CASES if c[0] == "halo-run")
    T, N, L = case[1], case[2], case[3]
    X, w = C.case_field(case), C.case_weights(case)
    da = xr.DataArray(X.reshape(T, 5, 13), dims=["time", "lat", "lon"],
                      coords={"time": np.arange(T), "lat": np.arange(5.0), "lon": np.arange(13.0)}, name="sst", attrs={"units": "K"})
    for kw in (dict(), dict(edges="trim"), dict(missing="renormalise", min_weight=case[6], complement=True)):
        out = facade.time_filter(da, w, handle=hip, **kw)
        want = time_filter(X, w, handle=hip, **kw)
        assert tuple(out.dims) == ("time", "lat", "lon") and out.name == "sst" and dict(out.attrs) == {"units": "K"}
        assert np.array_equal(_bits(np.asarray(out.values).reshape(want.shape)), _bits(want))
        first = L // 2 if kw.get("edges") == "trim" else 0
        assert np.array_equal(np.asarray(out.coords["time"].values), np.arange(first, T - first))
