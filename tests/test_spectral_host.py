"""No device: `xmca_amd.spectral.spectral_maps` - the refusals of the Python layer, what reaches the handle, the numpy
restatement of tests/spectral_cases.py against scipy.signal.welch / csd / coherence, against its longdouble truth and the bound, the
conditions on the committed cases that let the GPU test demand exact integers and NaN positions everywhere, the index rules of the
kernels restated in Python against the definition, `effective_segments`, the header and the xarray wrapper."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

import spectral_cases as C
from abi_cases import check_entry, header_abi_version, header_text
from xmca_amd import _hip, lagged, spectral
from xmca_amd.spectral import effective_segments, spectral_maps, welch_window

try:
    import xarray as xr                      # the real package, where it exists
except Exception:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
    import xarray as xr

from xmca_amd import xarray as facade

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"xmca_spectral_maps": 28, "xmca_spectral_tile": 3}
WALKED = ["tiny", "odd", "l8", "two", "three", "q4-plus", "q4-minus", "q1-group", "q0-minus", "q2-plus", "constant"]


class _NoDevice:
    """a handle that fails the test when anything reaches it"""

    def __getattr__(self, name):
        raise AssertionError("device touched: " + name)


class _Restated:
    """a handle that answers `spectral_maps` with the numpy restatement and records what it was handed"""
    device = 0

    def spectral_maps(self, X, Yc, nperseg, step, weights, detrend_mean, bins, fs, min_segments, alloc=None):
        self.got = dict(Yc=Yc, nperseg=nperseg, step=step, weights=weights, detrend_mean=detrend_mean, bins=bins, fs=fs,
                        min_segments=min_segments, alloc=alloc)
        # (the restatement centres the index once more: the mean of a centred series is rounding noise, and nothing here looks at bits)
        rest = C.restate(X, Yc, nperseg, step, np.asarray(weights), "mean" if detrend_mean else None, bins, fs, min_segments)
        keys = ("power",) + (C.CROSS if Yc is not None else ())
        out = {k: rest[k] for k in keys}
        out["segments"] = rest["segments"].astype(np.int32)
        return out


def _field(T=40, N=5, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, N)) + 10.0
    X[rng.random((T, N)) < 0.03] = np.nan
    return X


def _index(T=40, q=2, seed=5):
    return np.random.default_rng(seed).standard_normal((T, q)) + 3.0


def _maps(X=None, index=None, **kw):
    kw.setdefault("nperseg", 16)
    return spectral_maps(_field() if X is None else X, index, handle=_NoDevice(), **kw)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_bad_fields_raise_before_any_device_work():
    for bad, match in ((np.ones(40), "spatial"), (np.ones((40, 5), dtype=np.int32), "float32 or float64"), (np.ones((40, 5)) * 1j, "float32 or float64"),
                       (np.empty((40, 0)), "empty"), (np.float64(3.0), "time first"), (np.ones((15, 3)), "exceeds")):
        with pytest.raises(ValueError, match=match):
            _maps(bad)
    X = _field()
    X[3, 1] = np.inf
    with pytest.raises(ValueError, match="Inf"):
        _maps(X)


def test_bad_indices_raise_before_any_device_work():
    y = _index()
    nan, inf, const = y.copy(), y.copy(), y.copy()
    nan[3, 0], inf[5, 1], const[:, 1] = np.nan, np.inf, 2.5
    for bad, match in ((y[:39], "time steps"), (y[:, :0], "between 1 and 4"), (np.ones((40, 5)) * y[:, :1], "between 1 and 4"),
                       (y.reshape(40, 2, 1), "shape"), (nan, "NaN or an Inf"), (inf, "NaN or an Inf"), (const, "constant"),
                       (y * 1j, "real"), (np.array(["a"] * 40), "real"), (np.full(40, 7.0), "constant")):
        with pytest.raises(ValueError, match=match):
            _maps(index=bad)


def test_bad_segments_windows_and_bins_raise_before_any_device_work():
    for kw, match in ((dict(nperseg=7), "nperseg"), (dict(nperseg=4097), "nperseg"), (dict(nperseg=16.0), "nperseg"), (dict(nperseg=True), "nperseg"),
                      (dict(nperseg=41), "exceeds"), (dict(step=3), "step"), (dict(step=17), "step"), (dict(step=8.0), "step"),
                      (dict(step=True), "step"), (dict(window="hamming"), "window"), (dict(window=np.ones(15)), "window array"),
                      (dict(window=np.zeros(16)), "squared weights"), (dict(window=np.r_[np.ones(15), np.nan]), "NaN or an Inf"),
                      (dict(window=np.ones(16) * 1j), "window array"), (dict(window=np.ones((16, 1))), "window array"),
                      (dict(detrend="linear"), "detrend"), (dict(detrend=False), "detrend"), (dict(detrend="constant"), "detrend"),
                      (dict(bins=()), "empty"), (dict(bins=(0, 1, 0)), "distinct"), (dict(bins=(0, 9)), r"\[0, nperseg // 2\]"),
                      (dict(bins=(-1,)), r"\[0, nperseg // 2\]"), (dict(bins=(0.0,)), "integer"), (dict(bins=(True,)), "integer"),
                      (dict(bins=3), "sequence"), (dict(fs=0.0), "fs"), (dict(fs=-1.0), "fs"), (dict(fs=np.inf), "fs"), (dict(fs="1"), "fs"),
                      (dict(fs=True), "fs"), (dict(min_segments=0), "min_segments"), (dict(min_segments=2.0), "min_segments"),
                      (dict(min_segments=True), "min_segments"), (dict(min_segments=None), "min_segments")):
        with pytest.raises(ValueError, match=match):
            _maps(**kw)


def test_valid_arguments_reach_the_handle_and_nothing_else_does():
    for kw in (dict(), dict(nperseg=8), dict(nperseg=40), dict(step=4), dict(step=16), dict(window="boxcar"), dict(window=np.arange(16.0)),
               dict(window=list(range(1, 17))), dict(detrend=None), dict(bins=[8, 0]), dict(bins=np.array([3], dtype=np.int16)), dict(fs=12),
               dict(min_segments=1), dict(index=_index()), dict(index=_index()[:, 0]), dict(index=np.arange(40)), dict(index=_index(q=4)),
               dict(X=_field().astype(np.float32).reshape(40, 5, 1))):
        with pytest.raises(AssertionError, match="device touched: spectral_maps"):
            _maps(**kw)


def test_the_index_is_centred_on_the_host_and_the_results_keep_the_callers_shapes():
    rec = _Restated()
    X, y = _field().reshape(40, 5, 1), _index(q=3)
    out = spectral_maps(X, y, nperseg=16, step=5, bins=[8, 0, 3], fs=4.0, min_segments=1, handle=rec)
    mean = np.zeros(3)
    for row in y:
        mean = mean + row
    assert np.array_equal(rec.got["Yc"], y - mean / 40.0) and rec.got["Yc"].dtype == np.float64 and rec.got["alloc"] is None
    assert rec.got["nperseg"] == 16 and rec.got["step"] == 5 and rec.got["detrend_mean"] is True and list(rec.got["bins"]) == [8, 0, 3]
    assert rec.got["fs"] == 4.0 and rec.got["min_segments"] == 1 and np.array_equal(rec.got["weights"], welch_window("hann", 16))
    assert set(out) == {"power", "segments", "freqs", "bins"} | set(C.CROSS)
    assert out["power"].shape == (3, 5, 1) and out["segments"].shape == (5, 1) and out["segments"].dtype == np.int32
    assert all(out[k].shape == (3, 5, 1, 3) for k in C.CROSS) and all(out[k].dtype == np.float64 for k in C.CROSS + ("power",))
    assert out["bins"].dtype == np.int64 and list(out["bins"]) == [8, 0, 3] and np.array_equal(out["freqs"], np.array([8, 0, 3]) * 4.0 / 16)
    out = spectral_maps(X.astype(np.float32), None, nperseg=16, handle=rec)
    assert set(out) == {"power", "segments", "freqs", "bins"} and rec.got["Yc"] is None and rec.got["step"] == 8
    assert out["power"].shape == (9, 5, 1) and out["power"].dtype == np.float32 and list(out["bins"]) == list(range(9))
    one = spectral_maps(X, y[:, 0], nperseg=16, detrend=None, handle=rec)
    assert one["coherence"].shape == (9, 5, 1, 1) and rec.got["detrend_mean"] is False and one["p"].dtype == np.float64


def test_the_windows_are_scipys_and_the_twiddle_table_is_exact_at_the_quarter_turns():
    import scipy.signal
    for L in (8, 9, 100, 4096):
        # (scipy evaluates in float64: its angle 2 pi j / L carries 2 u of up to 2 pi, which half the cosine passes on as up to 6.3 u)
        assert np.max(np.abs(welch_window("hann", L) - scipy.signal.get_window("hann", L))) <= 8 * C.U
        assert np.array_equal(welch_window("boxcar", L), np.ones(L)) and welch_window("hann", L).dtype == np.float64
        tw = spectral.twiddle_table(L)
        t = 2 * np.pi * np.arange(L) / L
        assert tw.shape == (L, 2) and np.max(np.abs(tw[:, 0] - np.cos(t))) < 1e-15 * L and np.max(np.abs(tw[:, 1] + np.sin(t))) < 1e-15 * L
        assert tw[0, 0] == 1.0 and tw[0, 1] == 0.0
        if L % 4 == 0:
            assert (tw[L // 4] == [0.0, -1.0]).all() and (tw[L // 2] == [-1.0, 0.0]).all() and (tw[3 * L // 4] == [0.0, 1.0]).all()
        c, ms = spectral._twiddle_extended(L)
        assert np.max(np.abs(c * c + ms * ms - 1)) < 4 * 2.0 ** -63
    a = np.array([0.5, 1.0, 2.0, 0.0, 0.25, 1.5, 3.0, 1.0])
    assert np.array_equal(welch_window(a, 8), a) and np.array_equal(welch_window(list(range(1, 9)), 8), np.arange(1.0, 9.0))


def test_effective_segments():
    """Welch (1967): equal to K where the segments do not overlap, below K where they do, exact small cases by hand"""
    assert np.array_equal(effective_segments(np.arange(8), np.ones(16), 16), np.arange(8.0))
    assert np.array_equal(effective_segments(np.arange(8), welch_window("hann", 64), 64), np.arange(8.0))
    assert effective_segments(0, np.ones(8), 4) == 0.0 and effective_segments(1, np.ones(8), 4) == 1.0
    # boxcar, 50 % overlap: rho_1 = 1 / 2;  K = 2: 2 / (1 + 2 (1 / 2) (1 / 4)) = 1.6;  K = 4: 4 / (1 + 2 (3 / 4) (1 / 4)) = 32 / 11
    assert effective_segments(2, np.ones(8), 4) == pytest.approx(1.6, rel=1e-15)
    assert effective_segments(4, np.ones(8), 4) == pytest.approx(32 / 11, rel=1e-15)
    # Hann, 50 % overlap: rho_1 = 1 / 6 (the periodic window, L even)
    assert effective_segments(23, welch_window("hann", 64), 32) == pytest.approx(23 / (1 + 2 * (22 / 23) / 36), rel=1e-14)
    # 75 % overlap: three shifts count, and only those below K
    w = welch_window("hann", 16)
    rho = [np.sum(w[:16 - 4 * j] * w[4 * j:]) / np.sum(w * w) for j in (1, 2, 3)]
    assert effective_segments(2, w, 4) == pytest.approx(2 / (1 + 2 * 0.5 * rho[0] ** 2), rel=1e-14)
    assert effective_segments(9, w, 4) == pytest.approx(9 / (1 + 2 * sum((1 - j / 9) * rho[j - 1] ** 2 for j in (1, 2, 3))), rel=1e-14)
    ke = effective_segments(np.arange(1, 40), w, 4)
    assert np.all(np.diff(ke) > 0) and np.all(ke <= np.arange(1, 40)) and np.all(ke[1:] > 1.25)
    for bad in (-1, 2.5, np.array([1.0])):
        with pytest.raises(ValueError):
            effective_segments(bad, w, 4)


def test_the_constants_are_those_of_the_kernel():
    src = open(os.path.join(REPO, "xmca_amd", "csrc", "spectral.h")).read()
    assert spectral.MAX_INDICES == 4 and re.search(r"SP_MAX_Q\s*=\s*4\b", src)
    assert (spectral.MIN_NPERSEG, spectral.MAX_NPERSEG) == (8, 4096) and re.search(r"SP_MIN_L\s*=\s*8\s*,\s*SP_MAX_L\s*=\s*4096\b", src)
    assert re.search(r"SP_LIVE\s*=\s*0x1p-40\b", src) and C.LIVE == 2.0 ** -40
    code = re.sub(r"//.*", "", src)
    assert "atomic" not in code and "sincos" not in code and "sin(" not in code.replace("sinl(", "") and "cos(" not in code.replace("cosl(", "")


# ---- the restatement against scipy --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L, step, window, detrend", [(16, 8, "hann", "mean"), (9, 4, "hann", "mean"), (9, 3, "boxcar", None), (64, 16, "custom", "mean"),
                                                      (100, 37, "hann", None), (8, 8, "boxcar", "mean"), (25, 7, "custom", None)])
def test_the_restatement_is_scipys_welch_csd_and_coherence(L, step, window, detrend):
    """Gap-free float64: power = welch(x), cospectrum + i quadrature = csd(index, x), coherence = coherence(index, x), index_power =
    welch(index), to 1e-12 of the largest value of each map; the phase is the angle of csd."""
    import scipy.signal
    rng = np.random.default_rng(L + step)
    T, N, q, fs = 3 * L + 5, 7, 2, 2.5
    y = rng.standard_normal((T, q)) + 4.0
    X = 10.0 + rng.standard_normal((T, N))
    X[3:] += 0.8 * (y[:-3, :1] - 4.0)
    j = np.arange(L)
    w = 0.2 + ((7 * j) % 5) / 5.0 + j / L if window == "custom" else welch_window(window, L)
    rest = C.restate(X, y, L, step, w, detrend, None, fs, 1)
    kw = dict(fs=fs, window=w, nperseg=L, noverlap=L - step, detrend="constant" if detrend else False, axis=0)
    freqs, pxx = scipy.signal.welch(X, **kw)
    yc = lagged.center_index(y)[0]                 # (the index is centred over the record whatever `detrend` says: scipy gets that one)
    _, pyy = scipy.signal.welch(yc, **kw)
    assert np.allclose(freqs, np.arange(L // 2 + 1) * fs / L, rtol=1e-15, atol=0)
    assert (rest["segments"] == C.segments_of(T, L, step)).all()
    worst = {}

    def close(key, got, want):
        worst[key] = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        assert worst[key] <= 1e-12, (key, worst[key])
    close("power", rest["power"], pxx)
    for i in range(q):
        _, pxy = scipy.signal.csd(yc[:, i][:, None], X, **kw)
        _, coh = scipy.signal.coherence(yc[:, i][:, None], X, **kw)
        close("index_power", rest["index_power"][:, :, i], np.repeat(pyy[:, i][:, None], N, axis=1))
        close("cospectrum", rest["cospectrum"][:, :, i], pxy.real)
        close("quadrature", rest["quadrature"][:, :, i], pxy.imag)
        live = rest["live"][:, :, i]
        # (bin 0 of a de-meaned segment is sum_j w_j (x_j - mean): rounding noise under the boxcar alone, and dead there by the rule)
        assert live[1:L // 2].all() and live[0].all() != (detrend == "mean" and window == "boxcar")
        close("coherence", rest["coherence"][:, :, i][live], coh[live])
        close("gain", rest["gain"][:, :, i][live], (np.abs(pxy) / pyy[:, i][:, None])[live])
        inner = live & (np.abs(pxy) > 1e-6 * np.max(np.abs(pxy)))
        assert np.max(C.angle_between(rest["phase"][:, :, i][inner], np.angle(pxy)[inner])) < 1e-9
    print(L, step, window, detrend, "restatement against scipy, relative to the largest value:", {k: "%.2g" % v for k, v in worst.items()})


def test_a_planted_lead_of_the_index_has_a_negative_phase_in_the_restatement():
    rng = np.random.default_rng(8)
    T, L, d = 2000, 64, 5
    y = rng.standard_normal(T)
    X = np.empty((T, 2))
    X[:, 0] = np.roll(y, d)                 # x[t] = y[t - d]: the index leads by d steps
    X[:, 1] = np.roll(y, -d)                # the index lags
    X += 0.05 * rng.standard_normal((T, 2))
    rest = C.restate(X, y, L, bins=list(range(2, 6)))            # (2 pi f d < pi up to bin 6)
    f = np.arange(2, 6) / L
    assert np.all(rest["phase"][:, 0, 0] < 0) and np.all(rest["phase"][:, 1, 0] > 0)
    # (a shift within the segment loses d / L of the common signal to the neighbours: the estimate is near d, not at it)
    assert np.max(np.abs(-rest["phase"][:, 0, 0] / (2 * np.pi * f) - d)) < 1.0 and np.all(rest["coherence"][:, :, 0] > 0.5)


# ---- the cases and the restatement --------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_shapes_the_kernel_takes_another_path_at():
    cols, rows, groups = _hip.spectral_tile()
    assert (cols, rows, groups) == (C.C, C.R, C.GROUPS)
    Ls, Ns, qs = ({c[i] for c in C.CASES} for i in (4, 2, 3))
    assert Ls == {8, 9, 16, 64, 100, 4096} and Ns == {1, 3, cols - 1, cols, cols + 1, 4 * cols + 1} and qs == {0, 1, 2, 4}
    assert {c[9] for c in C.CASES} == set(C.PATTERNS) and {c[6] for c in C.CASES} == {"hann", "boxcar", "custom"} and {c[7] for c in C.CASES} == {"mean", None}
    t_kinds, s_kinds, b_kinds = set(), set(), set()
    for name, T, N, q, L, step, window, detrend, bins, pattern, ms in C.CASES:
        B = groups[q]
        assert -(-L // 4) <= step <= L <= T and len(set(bins)) == len(bins) and 0 <= min(bins) and max(bins) <= L // 2
        t_kinds |= {k for k, v in (("L", L), ("L+step-1", L + step - 1), ("L+step", L + step), ("3L+1", 3 * L + 1)) if T == v}
        s_kinds |= {k for k, v in (("L", L), ("L//2", L // 2), ("ceil(L/4)", -(-L // 4))) if step == v} | ({"non-divisor"} if L % step else set())
        b_kinds |= {k for k, v in (("one", 1), ("B-1", B - 1), ("B", B), ("B+1", B + 1), ("2B+1", 2 * B + 1)) if len(bins) == v}
        assert len(bins) == 1 or (0 in bins and L // 2 in bins and list(bins) != sorted(bins)), name
    assert t_kinds == {"L", "L+step-1", "L+step", "3L+1"} and s_kinds == {"L", "L//2", "ceil(L/4)", "non-divisor"}
    assert b_kinds == {"one", "B-1", "B", "B+1", "2B+1"}
    big = C.case_by_name("big")
    assert big[4] == 4096 and big[2] == 3
    w = C.case_window(C.case_by_name("three"))
    assert not np.allclose(w, w[::-1]) and not np.allclose(w[1:], w[1:][::-1])          # asymmetric, also as a periodic window


@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
def test_the_gap_patterns_are_what_they_say(case):
    name, T, N, q, L, step, window, detrend, bins, pattern, ms = case
    X = C.case_field(case)
    gone = np.isnan(X)
    K = C.segments_of(T, L, step)
    kn = C.reference(name, "float64")[0]["segments"]
    whole = np.array([[not gone[m * step:m * step + L, n].any() for n in range(N)] for m in range(K)])
    assert np.array_equal(kn, whole.sum(axis=0))
    if pattern == "none":
        assert not gone.any() and (kn == K).all()
    elif pattern == "scattered":
        assert 0.05 < gone.mean() < 0.2 and kn.min() == 0 and kn.max() >= min(K, 2) and len(set(kn.tolist())) >= min(K, 3)
    elif pattern == "step":
        assert gone.all(axis=1).sum() == 1 and gone.sum() == N and (kn == (1 if K == 2 else K - 2)).all()
    elif pattern == "column":
        assert gone[:, N // 3].all() and kn[N // 3] == 0 and gone[:, -1].sum() == 1 and 0 < kn[-1] < K and kn[0] == K
    elif pattern in ("single", "single-big"):
        assert kn[1] == 1 and (pattern == "single-big" or kn[N - 2] == ms - 1) and kn[0] == K
    elif pattern == "few":
        assert kn[3] == ms - 1 and kn[N - 2] == ms and kn[0] == K
    elif pattern == "overlap":
        rows = np.nonzero(gone.any(axis=1))[0]
        assert rows.min() >= step and rows.max() < L and (kn[0::3] <= K - 2).all() and (kn[1::3] == K).all()
    elif pattern == "constant":
        xp, present, cn = C.centred(X, True)
        assert (xp[:, 5] == 0.0).all() and (xp[:, N - 1] == 0.0).all() and gone[:L, N - 1].any() and kn[N - 1] == K - 1 and kn[5] == K
        rest = C.reference(name, "float64")[0]
        assert (rest["power"][:, 5] == 0.0).all() and (rest["power"][:, N - 1] == 0.0).all()
        assert not rest["live"][:, 5].any() and not rest["live"][:, N - 1].any()
        assert np.array_equal(rest["live"][:, 0].all(axis=-1), np.array(bins) != 0)          # (bin 0 under the boxcar: rounding noise, dead)
    assert np.isfinite(X[~gone]).all() and 5.0 < np.nanmean(X)          # the offset is there: the centring matters


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
def test_the_restatement_stays_within_the_bound_of_the_truth_and_agrees_on_every_integer(case, dtype):
    name, T, N, q = case[:4]
    rest, truth, allow, phase_ok = C.reference(name, dtype)
    assert np.array_equal(rest["segments"], truth["segments"]) and np.array_equal(rest["col_live"], truth["col_live"])
    report = {}
    for key in C.MAPS[:1 if q == 0 else None]:
        live = C.live_of(truth, key)
        assert np.array_equal(np.isnan(rest[key]), ~live), key
        assert np.isfinite(allow[key][live]).all() and (allow[key][live] >= 0).all()
        sel = phase_ok if key == "phase" else live
        report[key] = C.worst_ratio(rest[key], truth[key], allow[key], sel, circular=key == "phase")
        assert report[key] <= 1.0, (key, report[key])
        if dtype == "float64":
            assert report[key] <= 0.5, (key, report[key])          # (room for the device's fma against the restatement's multiply and add)
    if q:
        live = truth["live"]
        assert np.array_equal(rest["live"], live) and np.array_equal(np.isnan(rest["p"]), ~live)
        assert C.p_ratio(rest["p"], rest["coherence"], rest["ke"], live) <= 1.0
        assert np.all((rest["coherence"][live] >= 0) & (rest["coherence"][live] <= 1)) and np.all((rest["p"][live] >= 0) & (rest["p"][live] <= 1))
        left_out = float((live & ~phase_ok).sum()) / max(int(live.sum()), 1)
        report["phase left out"] = left_out
        assert left_out <= 0.05          # the planted signal keeps |C| above 2^10 of its bound: at most 5 % of the phases are not compared
    print(name, dtype, "error / bound:", {k: "%.3g" % v for k, v in report.items()})


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
def test_no_live_rule_of_a_committed_case_sits_on_its_threshold(case, dtype):
    """Conditions on the committed inputs: Sxx / R and Syy / Ry are exactly 0 or a factor 2^10 away from 2^-40 on either side, in the
    restatement and in the truth.  They let the GPU test demand exact NaN positions on every entry."""
    name = case[0]
    for res in C.reference(name, dtype)[:2]:
        acc = res["sums"]
        alive = acc["kn"] >= 1
        pairs = [(acc["sxx"][alive], np.broadcast_to(acc["r"][alive][:, None], acc["sxx"][alive].shape))]
        if acc["syy"].shape[-1]:
            pairs.append((acc["syy"][alive], np.broadcast_to(acc["ry"][alive][:, None, :], acc["syy"][alive].shape)))
        for s, r in pairs:
            assert (r >= 0).all() and ((r > 0) | (s == 0)).all()
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(r > 0, s / np.where(r > 0, r, 1), 0)
            on_edge = (s != 0) & (ratio > C.LIVE * 2.0 ** -10) & (ratio < C.LIVE * 2.0 ** 10)
            assert not on_edge.any(), (name, float(ratio[on_edge].min()))


def test_parseval_makes_r_the_mean_of_sxx_over_all_bins():
    """R_n = sum_m sum_j (w_j (x'_j - mu))^2 is the mean over the L two-sided bins of Sxx - the scale of the no-power rule"""
    rng = np.random.default_rng(2)
    for L, detrend in ((16, "mean"), (9, None), (9, "mean")):
        X = 10.0 + rng.standard_normal((3 * L, 4))
        rest = C.restate(X, None, L, L, "hann", detrend, None, 1.0, 1)
        sxx = rest["sums"]["sxx"]                                          # bins 0 .. L // 2
        mirror = sxx[:, 1:(L + 1) // 2]                                    # the negative frequencies
        assert np.allclose((sxx.sum(axis=1) + mirror.sum(axis=1)) / L, rest["sums"]["r"], rtol=1e-12)


# ---- the index rules of the kernels, against the definition -------------------------------------------------------------------------
@pytest.mark.parametrize("name", WALKED)
def test_the_walk_of_the_kernels_gives_the_bits_of_the_definition(name):
    case = C.case_by_name(name)
    X, index, kw = C.case_call(case)
    rest = C.reference(name, "float64")[0]
    yc = None if index is None else lagged.center_index(index)[0]
    w = kw["window"] if isinstance(kw["window"], np.ndarray) else welch_window(kw["window"], case[4])
    got = C.kernel_walk(X, rest["cn"], yc, w, rest["tables"], kw["bins"], case[4], kw["step"], kw["detrend"] == "mean")
    want = rest["sums"]
    assert np.array_equal(got[0], want["kn"])
    for g, key in zip(got[1:], ("sxx", "r", "syy", "cre", "cim", "ry")):
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint64), np.ascontiguousarray(want[key]).view(np.uint64)), key


def test_the_maps_of_a_bin_do_not_depend_on_the_other_bins_in_the_restatement():
    case = C.case_by_name("q2-plus")
    X, index, kw = C.case_call(case)
    whole = C.reference("q2-plus", "float64")[0]
    pick = [4, 1, 6]
    part = C.restate(X, index, case[4], **dict(kw, bins=[kw["bins"][i] for i in pick]))
    for key in C.MAPS + ("p",):
        assert np.array_equal(part[key], whole[key][pick], equal_nan=True), key
    assert np.array_equal(part["segments"], whole["segments"])


# ---- ABI and facade -------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entries_and_the_binding_has_them():
    for name, n_args in NEW.items():
        check_entry(name, n_args)
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version() == 16
    text = header_text(comments=True)                 # (the stage names stand in a comment)
    for stage in ("spectral_center", "spectral_index", "spectral_segments", "spectral_finish"):
        assert '"%s"' % stage in text, stage
    assert callable(_hip.Handle.spectral_maps) and (_hip.DETREND_NONE, _hip.DETREND_MEAN) == (0, 1)
    lib = _hip.load_library()
    import ctypes
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    g = (ctypes.c_int * 5)()
    assert lib.xmca_spectral_tile(ctypes.byref(a), ctypes.byref(b), None) == _hip.ERR_INVALID
    assert lib.xmca_spectral_tile(ctypes.byref(a), ctypes.byref(b), g) == 0 and (a.value, b.value, tuple(g)) == (256, 8, C.GROUPS)
    assert "spectral.h" in __import__("xmca_amd.build", fromlist=["HEADERS"]).HEADERS


def test_the_package_does_not_export_the_module():
    import xmca_amd
    assert "spectral_maps" not in xmca_amd.__all__ and "spectral" not in xmca_amd.__all__


def test_the_xarray_wrapper_has_the_parameters_of_spectral_maps():
    a = inspect.signature(spectral_maps).parameters
    b = inspect.signature(facade.spectral_maps).parameters
    assert list(a)[1:] == list(b)[1:] and list(b)[0] == "da"
    for name in list(a)[1:]:
        assert a[name].default == b[name].default and a[name].kind == b[name].kind, name


def test_the_xarray_wrapper_checks_before_the_device_and_wraps_the_maps():
    X = _field(T=48, N=6)
    da = xr.DataArray(X.reshape(48, 2, 3), dims=["time", "lat", "lon"],
                      coords={"time": np.arange(100, 148), "lat": [0.0, 1.0], "lon": [0.0, 1.0, 2.0]}, name="sst", attrs={"units": "K"})
    y = _index(T=48, q=2)
    index = xr.DataArray(y, dims=["time", "mode"], coords={"time": np.arange(100, 148)})
    with pytest.raises(ValueError, match="distinct"):
        facade.spectral_maps(da, index, nperseg=16, bins=[1, 1], handle=_NoDevice())
    with pytest.raises(AssertionError, match="device touched: spectral_maps"):
        facade.spectral_maps(da, index, nperseg=16, handle=_NoDevice())
    with pytest.raises(TypeError, match="DataArray"):
        facade.spectral_maps(da.values, index, nperseg=16, handle=_NoDevice())
    kw = dict(nperseg=16, step=4, bins=[3, 0, 8], fs=12.0, min_segments=1)
    out = facade.spectral_maps(da, index, handle=_Restated(), **kw)
    want = spectral_maps(X.reshape(48, 2, 3), y, handle=_Restated(), **kw)
    assert set(out) == set(want) == {"power", "segments", "freqs", "bins"} | set(C.CROSS)
    for key in C.CROSS:
        assert tuple(out[key].dims) == ("frequency", "lat", "lon", "index") and out[key].shape == (3, 2, 3, 2)
        assert np.array_equal(np.asarray(out[key].values), want[key], equal_nan=True)
        assert np.array_equal(np.asarray(out[key].coords["frequency"].values), want["freqs"])
        assert np.array_equal(np.asarray(out[key].coords["lon"].values), [0.0, 1.0, 2.0])
        assert np.array_equal(np.asarray(out[key].coords["index"].values), [0, 1])
    assert tuple(out["power"].dims) == ("frequency", "lat", "lon") and np.array_equal(np.asarray(out["power"].values), want["power"], equal_nan=True)
    assert tuple(out["segments"].dims) == ("lat", "lon") and np.array_equal(np.asarray(out["segments"].values), want["segments"])
    assert tuple(out["freqs"].dims) == ("frequency",) and np.array_equal(np.asarray(out["bins"].values), [3, 0, 8])
    assert np.isfinite(np.asarray(out["coherence"].values)).any()
    alone = facade.spectral_maps(da, nperseg=16, handle=_Restated())
    assert set(alone) == {"power", "segments", "freqs", "bins"} and alone["power"].shape == (9, 2, 3)
