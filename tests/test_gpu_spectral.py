"""GPU: `xmca_amd.spectral.spectral_maps` - the kernels of csrc/spectral.h.  The numpy restatement, the longdouble
truth and the cases: tests/spectral_cases.py (T in {L, L + step - 1, L + step, 3 L + 1}, L in {8, 9, 16, 64, 100} and once 4096, step in
{L, L // 2, ceil(L / 4)} and a non-divisor, N in {1, 255, 256, 257, 1025} around the C = 256 columns of a workgroup, q in {0, 1, 2, 4},
bin lists of {1, B - 1, B, B + 1, 2 B + 1} entries around the group B(q), three windows, both detrend modes, nine gap patterns, both
dtypes).

Bounds.  `segments` and every NaN position equal the restatement's exactly: no live rule of a committed case sits on its threshold
(tests/test_spectral_host.py).  power, index_power, cospectrum, quadrature, coherence and gain stay within the allowance
`spectral_cases.bounds` computes per entry in longdouble from the truth's own sums, nothing of it measured: with u = 2^-53 each part of
a segment's Z errs by at most (L + 4) u (sum |w x'| + |W_k| sum |x'| / L), the sums over K_n segments add (K_n + 3) u of themselves,
the ratios follow to first order; the allowance is twice that, plus half a float32 spacing at the value for a float32 field.  phase
is compared, on the circle, where |C| exceeds 2^10 times its own bound - every live entry of the committed cases.  p is compared with
(1 - coherence)^(Ke - 1) in longdouble at the device's own coherence within 16 u (1 + |ln p|) p.  Worst error / bound measured on an
MI355X: profiles/spectral_accuracy.json, written by scripts/spectral_accuracy.py."""
import numpy as np
import pytest

try:
    import torch                                            # (before the first device call of the session, as the other torch tests do)
except Exception:
    torch = None

import spectral_cases as C
from xmca_amd import _hip
from xmca_amd.array import MCA
from xmca_amd.lagged import center_index
from xmca_amd.spectral import spectral_maps, welch_window

pytestmark = pytest.mark.gpu

DEVICE_KEYS = ("power", "segments") + C.CROSS


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _keys(out):
    return [k for k in DEVICE_KEYS if k in out]


def _same_bits(a, b):
    return _keys(a) == _keys(b) and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in _keys(a))


def _call(hip, case, dtype, **over):
    X, index, kw = C.case_call(case, dtype)
    kw.update(over)
    return spectral_maps(X, index, nperseg=case[4], handle=hip, **kw)


def check_against(got, rest, truth, allow, phase_ok, q, dtype):
    """The assertions of a run against its references; returns the worst error / bound per map."""
    assert np.array_equal(got["segments"], rest["segments"]) and got["segments"].dtype == np.int32          # every column, exactly
    report = {}
    for key in C.MAPS[:1 if q == 0 else None]:
        live = C.live_of(rest, key)
        assert got[key].dtype == np.dtype(dtype) and got[key].shape == rest[key].shape, key
        assert np.array_equal(np.isnan(got[key]), ~live), key                                             # every NaN position, exactly
        assert not np.isinf(got[key]).any(), key
        sel = phase_ok if key == "phase" else live
        report[key] = C.worst_ratio(got[key], truth[key], allow[key], sel, circular=key == "phase")
    if q:
        live = rest["live"]
        assert got["p"].dtype == np.float64 and np.array_equal(np.isnan(got["p"]), ~live)
        assert np.all((got["coherence"][live] >= 0) & (got["coherence"][live] <= 1)) and np.all((got["p"][live] >= 0) & (got["p"][live] <= 1))
        assert np.all(np.abs(got["phase"][live]) <= np.float32(np.pi) if dtype == "float32" else np.abs(got["phase"][live]) <= np.pi)
        report["p"] = C.p_ratio(got["p"], got["coherence"], rest["ke"], live)
    return report


def test_the_cases_know_the_tile_of_the_library():
    cols, rows, groups = _hip.spectral_tile()
    assert (cols, rows, groups) == (C.C, C.R, C.GROUPS)
    assert {1, cols - 1, cols, cols + 1, 4 * cols + 1} <= {c[2] for c in C.CASES}
    for q in (0, 1, 2, 4):
        B = groups[q]
        lengths = {len(c[8]) for c in C.CASES if c[3] == q}
        assert any(n % B for n in lengths) and any(n >= B for n in lengths), (q, lengths)    # a partial group and a whole one


# ---- against the restatement and the longdouble truth ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
def test_against_the_restatement(hip, case, dtype):
    name, T, N, q, L, step, window, detrend, bins, pattern, ms = case
    got = _call(hip, case, dtype)
    rest, truth, allow, phase_ok = C.reference(name, dtype)
    assert set(got) == {"power", "segments", "freqs", "bins"} | (set(C.CROSS) if q else set())
    assert all(isinstance(got[k], np.ndarray) for k in got)
    assert got["power"].shape == (len(bins), N) and got["segments"].shape == (N,) and tuple(got["bins"]) == tuple(bins)
    assert np.array_equal(got["freqs"], np.array(bins) / L)
    report = check_against(got, rest, truth, allow, phase_ok, q, dtype)
    print(name, dtype, "error / bound:", {k: "%.3g" % v for k, v in report.items()})
    assert all(v <= 1.0 for v in report.values()), report


# ---- checks that need no reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
def test_a_column_used_as_its_own_index_is_coherent_with_gain_one(hip, dtype):
    rng = np.random.default_rng(4)
    T, N, L = 200, 257, 32
    X = (10.0 + rng.standard_normal((T, N))).astype(dtype)
    y = X[:, [5, 200]].astype(np.float64)
    out = spectral_maps(X, y, nperseg=L, handle=hip)
    truth = C.restate(X, y, L, real=np.longdouble)
    allow, _ = C.bounds(truth, L, 1.0, dtype)
    for j, n in enumerate((5, 200)):
        for key, want in (("coherence", 1), ("gain", 1)):
            assert np.all(np.abs(out[key][:, n, j].astype(np.longdouble) - want) <= allow[key][:, n, j]), key
        assert np.all(out["p"][:, n, j] <= 1e-12)
        assert np.all(np.abs(out["power"][:, n].astype(np.longdouble) - out["index_power"][:, n, j]) <= allow["power"][:, n] + allow["index_power"][:, n, j])
    assert np.all(out["coherence"][1:, 6, 0] < 0.95) and (out["segments"] == C.segments_of(T, L, L // 2)).all()


@pytest.mark.parametrize("d", [5, -5])
def test_a_planted_lag_comes_back_with_the_sign_of_its_phase(hip, d):
    """x[t] = y[t - d]: the index leads by d steps, and the phase at frequency f is near -2 pi f d (d = -5: the index lags)"""
    rng = np.random.default_rng(8)
    T, L = 2000, 64
    y = rng.standard_normal(T)
    X = 10.0 + 0.05 * rng.standard_normal((T, 3))
    X[:, 1] += 3.0 * np.roll(y, d)
    bins = [5, 2, 4, 3]
    out = spectral_maps(X, y, nperseg=L, bins=bins, handle=hip)
    f = np.array(bins) / L
    phase = out["phase"][:, 1, 0]
    assert np.all(np.sign(phase) == -np.sign(d)) and np.max(np.abs(-phase / (2 * np.pi * f) - d)) < 1.0
    assert np.all(out["coherence"][:, 1, 0] > 0.5) and np.all(out["p"][:, 1, 0] < 1e-6) and np.all(np.abs(out["gain"][:, 1, 0] - 3.0) < 0.6)
    assert np.all(out["coherence"][:, 0, 0] < 0.5)


def test_welch_of_a_gap_free_field_is_scipys(hip):
    import scipy.signal
    rng = np.random.default_rng(12)
    T, N, L, step, fs = 300, 40, 50, 20, 12.0
    y = rng.standard_normal(T)
    X = 10.0 + rng.standard_normal((T, N)) + 0.7 * np.roll(y, 2)[:, None]
    out = spectral_maps(X, y, nperseg=L, step=step, fs=fs, min_segments=1, handle=hip)
    kw = dict(fs=fs, window="hann", nperseg=L, noverlap=L - step, detrend="constant", axis=0)
    freqs, pxx = scipy.signal.welch(X, **kw)
    _, pxy = scipy.signal.csd((y - y.mean())[:, None], X, **kw)
    _, coh = scipy.signal.coherence((y - y.mean())[:, None], X, **kw)
    assert np.allclose(out["freqs"], freqs, rtol=1e-15)
    for got, want in ((out["power"], pxx), (out["cospectrum"][..., 0], pxy.real), (out["quadrature"][..., 0], pxy.imag), (out["coherence"][..., 0], coh)):
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


# ---- bits --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("name", ["wide", "single", "q4-plus", "nondiv"])
def test_a_call_repeats_its_bits_and_a_bin_does_not_see_the_other_bins(hip, name, dtype):
    case = C.case_by_name(name)
    bins = list(case[8])
    B = C.GROUPS[case[3]]
    whole = _call(hip, case, dtype)
    assert _same_bits(whole, _call(hip, case, dtype))                                  # a repeated call
    cut = B + 1 if len(bins) > B + 1 else 1                                            # the first call ends inside a group of bins
    first, rest = _call(hip, case, dtype, bins=bins[:cut]), _call(hip, case, dtype, bins=bins[cut:])
    keys = [k for k in _keys(whole) if k != "segments"]
    for k in keys:                                                                     # a bin list split in two calls
        assert np.array_equal(_bits(np.concatenate([first[k], rest[k]])), _bits(whole[k])), k
    order = np.random.default_rng(len(bins)).permutation(len(bins))
    mixed = _call(hip, case, dtype, bins=[bins[i] for i in order])                     # a permuted bin list
    assert tuple(mixed["bins"]) == tuple(bins[i] for i in order)
    for k in keys:
        assert np.array_equal(_bits(mixed[k]), _bits(whole[k][order])), k
    full = _call(hip, case, dtype, bins=None)                                          # every bin of the spectrum
    assert full["power"].shape[0] == case[4] // 2 + 1
    for k in keys:
        assert np.array_equal(_bits(full[k][bins]), _bits(whole[k])), k
    for part in (first, rest, mixed, full):
        assert np.array_equal(part["segments"], whole["segments"])


# ---- tensors -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("layout", ["contiguous", "transposed", "column slice", "three dimensions"])
def test_a_gpu_tensor_gives_gpu_tensors_with_the_bits_of_the_numpy_route(hip, layout, dtype):
    case = C.case_by_name("q2-plus")
    name, T, N, q, L, step, window, detrend, bins, pattern, ms = case
    X, y, kw = C.case_call(case, dtype)
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
        t = torch.from_numpy(X.copy()).to(dev).reshape(T, 16, 16)
    before = t.clone()
    S = tuple(t.shape[1:])
    for index in (y, None):
        want = spectral_maps(X, index, nperseg=L, handle=hip, **kw)
        out = spectral_maps(t, index, nperseg=L, handle=hip, **kw)
        assert set(out) == set(want)
        for k in _keys(want):
            kind = torch.int32 if k == "segments" else torch.float64 if k == "p" else t.dtype
            assert isinstance(out[k], torch.Tensor) and out[k].device == dev and out[k].dtype == kind and out[k].is_contiguous(), k
            assert tuple(out[k].shape) == (() if k == "segments" else (len(bins),)) + S + (() if k in ("power", "segments") else (q,)), k
            assert np.array_equal(_bits(out[k].cpu().numpy().reshape(want[k].shape)), _bits(want[k])), k
        assert isinstance(out["bins"], np.ndarray) and isinstance(out["freqs"], np.ndarray) and tuple(out["bins"]) == tuple(bins)
    assert torch.equal(torch.nan_to_num(t, nan=-1.0), torch.nan_to_num(before, nan=-1.0))          # the input is unchanged
    again = spectral_maps(t, torch.from_numpy(y).to(dev), nperseg=L, handle=hip, **kw)               # an index on the GPU is fetched
    want = spectral_maps(X, y, nperseg=L, handle=hip, **kw)
    assert np.array_equal(_bits(again["coherence"].cpu().numpy().reshape(want["coherence"].shape)), _bits(want["coherence"]))


def test_a_tensor_with_an_inf_is_refused(hip):
    t = torch.ones(20, 4, dtype=torch.float64, device=torch.device("cuda", hip.device))
    t[3, 1] = float("inf")
    with pytest.raises(ValueError, match="Inf"):
        spectral_maps(t, np.arange(20.0), nperseg=8, handle=hip)


# ---- state -----------------------------------------------------------------------------------------------------------------------------
def test_a_solved_rotated_model_on_the_handle_keeps_its_result_to_the_bit(hip):
    rng = np.random.default_rng(11)
    F = rng.standard_normal((40, 6)) @ rng.standard_normal((6, 90)) + 0.1 * rng.standard_normal((40, 90))
    m = MCA(F, handle=hip)
    m.solve()
    m.rotate(3)
    before = (m.singular_values().copy(), m.eofs(3)['left'].copy(), m.pcs(3)['left'].copy())
    hip.reset_timings()
    _call(hip, C.case_by_name("q0-minus"), "float64")
    assert {"spectral_center", "spectral_segments", "spectral_finish"} <= set(hip.timings()) and "spectral_index" not in set(hip.timings())
    hip.reset_timings()
    _call(hip, C.case_by_name("nondiv"), "float32")          # detrend=None: no centring pass
    assert {"spectral_index", "spectral_segments", "spectral_finish"} <= set(hip.timings()) and "spectral_center" not in set(hip.timings())
    for a, b in zip(before, (m.singular_values(), m.eofs(3)['left'], m.pcs(3)['left'])):
        assert np.array_equal(_bits(a), _bits(b))
    out = spectral_maps(F, m.pcs(3)['left'], nperseg=16, handle=hip)          # the documented two-line route
    assert out["coherence"].shape == (9, 90, 3) and np.isfinite(out["coherence"][1:]).all() and np.isfinite(out["power"]).all()


# ---- the C entry -----------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_bad_arguments_before_any_launch(hip):
    """XMCA_ERR_INVALID from the C entry itself (the Python layer checks the same things earlier); the handle stays usable"""
    T, N, q, L, F = 40, 3, 2, 16, 3
    rng = np.random.default_rng(0)
    X = rng.standard_normal((T, N)) + 10.0
    Y, _ = center_index(rng.standard_normal((T, q)))
    wide, _ = center_index(rng.standard_normal((T, 5)))
    w = welch_window("hann", L)
    bins = np.array([8, 0, 3], dtype=np.int32)
    power, seg = np.empty((F, N)), np.zeros(N, dtype=np.int32)          # (a refused call writes nothing)
    maps = [np.empty((F, N, q)) for _ in range(7)]
    p = _hip._ptr

    def call(T=T, N=N, stride_t=N, stride_n=1, dtype=_hip.XMCA_F64, Y=Y, q=q, L=L, step=8, w=w, detrend=_hip.DETREND_MEAN, bins=bins, F=F, fs=1.0,
             ms=2, where=_hip.HOST, out_where=_hip.HOST, power=power, first=maps[0]):
        return hip._lib.xmca_spectral_maps(hip._h, p(X), where, T, N, stride_t, stride_n, dtype, p(Y), q, L, step, p(w), detrend, p(bins), F, fs, ms,
                                           p(power), p(first), p(maps[1]), p(maps[2]), p(maps[3]), p(maps[4]), p(maps[5]), p(maps[6]), p(seg), out_where)
    assert call() == 0 and np.all(seg == 4) and np.isfinite(power).all() and np.isfinite(maps[3][0]).all()
    bad_y, bad_w = Y.copy(), w.copy()
    bad_y[4, 1], bad_w[3] = np.nan, np.inf
    for bad in (dict(q=-1), dict(q=5, Y=wide), dict(L=7), dict(L=4097), dict(L=41), dict(step=3), dict(step=17), dict(step=0), dict(detrend=2),
                dict(detrend=-1), dict(F=0), dict(F=10), dict(bins=np.array([0, 9, 1], dtype=np.int32)), dict(bins=np.array([0, -1, 1], dtype=np.int32)),
                dict(bins=np.array([1, 0, 1], dtype=np.int32)), dict(w=bad_w), dict(w=np.zeros(L)), dict(fs=0.0), dict(fs=-2.0), dict(fs=np.inf),
                dict(fs=np.nan), dict(ms=0), dict(Y=bad_y), dict(dtype=7), dict(where=5), dict(out_where=5), dict(stride_t=-1), dict(stride_n=-1),
                dict(T=0), dict(N=0), dict(Y=None), dict(power=None), dict(first=None), dict(w=None), dict(bins=None)):
        assert call(**bad) == _hip.ERR_INVALID, bad
    with pytest.raises(ValueError, match="T x q"):
        hip.spectral_maps(X, Y[:10], L, 8, w, True, bins, 1.0, 2)
    again = [m.copy() for m in maps] + [power.copy()]
    assert call() == 0 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, maps + [power]))
    assert call(q=0, Y=None, first=None) == 0 and np.isfinite(power).all()          # the field alone


# ---- xarray ----------------------------------------------------------------------------------------------------------------------------
def test_the_xarray_wrapper_returns_the_maps_over_the_dims_of_the_input(hip):
    import os
    import sys
    try:
        import xarray as xr
    except Exception:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
        import xarray as xr
    from xmca_amd import xarray as facade
    case = C.case_by_name("q2-plus")
    name, T, N, q, L, step, window, detrend, bins, pattern, ms = case
    X, y, kw = C.case_call(case)
    X = X[:, :65]
    da = xr.DataArray(X.reshape(T, 5, 13), dims=["time", "lat", "lon"],
                      coords={"time": np.arange(T), "lat": np.arange(5.0), "lon": np.arange(13.0)}, name="sst", attrs={"units": "K"})
    index = xr.DataArray(y, dims=["time", "mode"], coords={"time": np.arange(T)})
    out = facade.spectral_maps(da, index, nperseg=L, handle=hip, **kw)
    want = spectral_maps(X, y, nperseg=L, handle=hip, **kw)
    for k in C.CROSS:
        assert tuple(out[k].dims) == ("frequency", "lat", "lon", "index")
        assert np.array_equal(_bits(np.asarray(out[k].values).reshape(want[k].shape)), _bits(want[k]))
        assert np.array_equal(np.asarray(out[k].coords["frequency"].values), want["freqs"])
    assert tuple(out["power"].dims) == ("frequency", "lat", "lon") and tuple(out["segments"].dims) == ("lat", "lon")
