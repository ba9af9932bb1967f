"""No device: `xmca_amd.lagged.lead_lag_maps` - the refusals of the Python layer, what reaches the handle, the numpy
restatement of tests/lead_lag_cases.py against its longdouble truth and the bound, the conditions on the committed cases that let
the GPU test demand exact integers everywhere, the restated p-value against scipy, the index rules of the moment kernel restated in
Python against the definition, the header and the xarray wrapper."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

import lead_lag_cases as C
from abi_cases import check_entry, header_abi_version, header_text
from xmca_amd import _hip, lagged
from xmca_amd.lagged import lead_lag_maps

try:
    import xarray as xr                      # the real package, where it exists
except Exception:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
    import xarray as xr

from xmca_amd import xarray as facade

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"xmca_lead_lag_maps": 22, "xmca_lead_lag_tile": 3}


class _NoDevice:
    """a handle that fails the test when anything reaches it"""

    def __getattr__(self, name):
        raise AssertionError("device touched: " + name)


class _Restated:
    """a handle that answers `lead_lag_maps` with the numpy restatement and records what it was handed"""
    device = 0

    def lead_lag_maps(self, X, Yc, lags, min_pairs, rho_y=None, alloc=None):
        self.got = dict(Yc=Yc, lags=lags, min_pairs=min_pairs, rho_y=rho_y, alloc=alloc)
        xp, present, cn, n0 = C.centred(X)
        m = C.moments(xp, present, Yc, [int(l) for l in lags])
        rho_x = C.lag1_field(xp, present, n0) if rho_y is not None else None
        f = C.finish(m, min_pairs, rho_x, rho_y)
        r = f["r"].astype(X.dtype)
        return r, f["slope"].astype(X.dtype), C.pvalue(r.astype(np.float64), f["dof"]), f["dof"].astype(np.int32), m["n"].astype(np.int32), rho_x


def _field(T=40, N=5, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, N)) + 10.0
    X[rng.random((T, N)) < 0.2] = np.nan
    return X


def _index(T=40, q=2, seed=5):
    return np.random.default_rng(seed).standard_normal((T, q)) + 3.0


def _maps(X=None, index=None, lags=(0, 1, -1), **kw):
    return lead_lag_maps(_field() if X is None else X, _index() if index is None else index, lags, handle=_NoDevice(), **kw)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_bad_fields_raise_before_any_device_work():
    for bad, match in ((np.ones(40), "spatial"), (np.ones((40, 5), dtype=np.int32), "float32 or float64"), (np.ones((40, 5)) * 1j, "float32 or float64"),
                       (np.empty((40, 0)), "empty"), (np.float64(3.0), "time first")):
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
    for bad, match in ((y[:39], "time steps"), (y[:, :0], "between 1 and 8"), (np.ones((40, 9)) * y[:, :1], "between 1 and 8"),
                       (y.reshape(40, 2, 1), "shape"), (nan, "NaN or an Inf"), (inf, "NaN or an Inf"), (const, "constant"),
                       (y * 1j, "real"), (np.array(["a"] * 40), "real"), (np.full(40, 7.0), "constant")):
        with pytest.raises(ValueError, match=match):
            _maps(index=bad)


def test_bad_lags_raise_before_any_device_work():
    for bad, match in (((), "empty"), ((0, 1, 0), "distinct"), ((0, 40), r"\[-\(T - 1\), T - 1\]"), ((-40,), r"\[-\(T - 1\), T - 1\]"),
                       ((0.0, 1.0), "integer"), ((True,), "integer"), (3, "sequence"), (("1",), "integer"),
                       (np.array([0.5]), "integer")):
        with pytest.raises(ValueError, match=match):
            _maps(lags=bad)
    X, y = _field(T=700, N=2), _index(T=700, q=2)
    with pytest.raises(ValueError, match="1024"):
        _maps(X, y, lags=range(-256, 257))          # 513 lags x 2 series
    with pytest.raises(AssertionError, match="device touched: lead_lag_maps"):
        _maps(X, y, lags=range(-256, 256))          # 512 x 2 = 1024 is taken


def test_bad_options_raise_before_any_device_work():
    for kw, match in ((dict(min_pairs=2), "min_pairs"), (dict(min_pairs=8.0), "min_pairs"), (dict(min_pairs=True), "min_pairs"),
                      (dict(min_pairs=None), "min_pairs"), (dict(dof="N"), "dof"), (dict(dof=1), "dof"), (dict(dof="ar1"), "dof")):
        with pytest.raises(ValueError, match=match):
            _maps(**kw)


def test_a_record_beyond_the_range_of_the_p_value_is_refused():
    class Long:          # (only the shape is looked at before the refusal)
        shape, ndim = (_hip.PVALUE_MAX_OBS + 1, 2), 2

        def __array__(self, dtype=None, copy=None):
            raise AssertionError("the field was converted")
    with pytest.raises(ValueError, match="time steps"):
        lead_lag_maps(Long(), np.arange(5.0), [0], handle=_NoDevice())


def test_valid_arguments_reach_the_handle_and_nothing_else_does():
    for kw in (dict(), dict(min_pairs=3), dict(dof="bretherton"), dict(lags=[39, -39]), dict(lags=np.array([2, -5], dtype=np.int16)),
               dict(index=_index()[:, 0]), dict(index=np.arange(40)), dict(X=_field().astype(np.float32).reshape(40, 5, 1))):
        with pytest.raises(AssertionError, match="device touched: lead_lag_maps"):
            _maps(**kw)


def test_the_index_is_centred_on_the_host_and_the_results_keep_the_callers_shapes():
    rec = _Restated()
    X, y = _field().reshape(40, 5, 1), _index(q=3)
    out = lead_lag_maps(X, y, [2, -1, 0, 7], min_pairs=5, handle=rec)
    mean = np.zeros(3)
    for row in y:
        mean = mean + row
    assert np.array_equal(rec.got["Yc"], y - mean / 40.0) and rec.got["Yc"].dtype == np.float64 and rec.got["rho_y"] is None
    assert rec.got["alloc"] is None and rec.got["min_pairs"] == 5 and list(rec.got["lags"]) == [2, -1, 0, 7]
    assert set(out) == {"r", "slope", "p", "dof", "pairs", "lags"}
    assert out["r"].shape == out["slope"].shape == out["p"].shape == out["dof"].shape == (4, 5, 1, 3) and out["pairs"].shape == (4, 5, 1)
    assert out["r"].dtype == out["slope"].dtype == np.float64 and out["p"].dtype == np.float64
    assert out["dof"].dtype == out["pairs"].dtype == np.int32 and out["lags"].dtype == np.int64 and list(out["lags"]) == [2, -1, 0, 7]
    out = lead_lag_maps(X.astype(np.float32), y[:, 0], [0], dof="bretherton", handle=rec)
    assert out["r"].shape == (1, 5, 1, 1) and out["r"].dtype == out["slope"].dtype == np.float32 and out["lag1"].shape == (5, 1)
    assert rec.got["rho_y"].shape == (1,) and np.array_equal(rec.got["rho_y"], C.lag1_index(rec.got["Yc"]))


def test_the_lag1_of_the_index_is_the_expression_of_the_field():
    for case in C.CASES[:6]:
        yc, _ = lagged.center_index(C.case_index(case))
        rho = lagged.lag1_index(yc)
        assert np.array_equal(rho, C.lag1_index(yc)) and np.all(np.abs(rho) <= 1.0)
        assert np.max(np.abs(rho - C.lag1_index(yc, np.longdouble))) < 1e-13
    assert 0.2 < lagged.lag1_index(lagged.center_index(C.case_index(C.case_by_name("long-lags")))[0])[0] < 0.9          # AR(1), phi = 0.6


def test_the_constants_are_those_of_the_kernel():
    src = open(os.path.join(REPO, "xmca_amd", "csrc", "lead_lag.h")).read()
    assert lagged.MAX_INDICES == 8 and re.search(r"LL_MAX_Q\s*=\s*8\b", src)
    assert lagged.MAX_ENTRIES == 1024 and re.search(r"LL_MAX_ENTRIES\s*=\s*1024\b", src)
    assert re.search(r"LL_LIVE\s*=\s*0x1p-40\b", src) and C.LIVE == 2.0 ** -40
    code = re.sub(r"//.*", "", src)
    assert "atomic" not in code and "__shared__" not in code


# ---- the cases and the restatement --------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_shapes_the_kernel_takes_another_path_at():
    cols, rows, groups = _hip.lead_lag_tile()
    assert (cols, rows, groups) == (C.C, C.R, C.GROUPS)
    Ts, Ns, qs = ({c[i] for c in C.CASES} for i in (1, 2, 3))
    assert Ts == {rows - 1, rows, rows + 1, 2 * rows + 1, 97, 300} and Ns == {1, cols - 1, cols, cols + 1, 4 * cols + 1}
    assert qs == {1, 2, 3, 5, 8} and {c[5] for c in C.CASES} == set(C.PATTERNS)
    lengths = {}
    for name, T, N, q, lags, pattern, min_pairs in C.CASES:
        G = groups[q - 1]
        lengths.setdefault(q, set()).add(len(lags))
        assert len(lags) in {1, G - 1, G, G + 1, 2 * G + 1} and len(set(lags)) == len(lags) and max(abs(l) for l in lags) <= T - 1
    kinds = set()
    for name, T, N, q, lags, pattern, min_pairs in C.CASES:
        G = groups[q - 1]
        kinds |= {k for k, n in (("one", 1), ("G-1", G - 1), ("G", G), ("G+1", G + 1), ("2G+1", 2 * G + 1)) if len(lags) == n}
    assert kinds == {"one", "G-1", "G", "G+1", "2G+1"}
    assert any(list(c[4]) != sorted(c[4]) for c in C.CASES) and any(min(c[4]) < 0 for c in C.CASES)
    for name in ("tiny-ends", "long-lags"):          # gap-free: T - |lag| pairs - one pair, exactly min_pairs, min_pairs - 1
        name, T, N, q, lags, pattern, min_pairs = C.case_by_name(name)
        assert pattern == "none" and {T - 1, -(T - 1), T - min_pairs, T - min_pairs + 1} <= set(lags)
        pairs = C.reference(name, "float64", "n")[0]["pairs"]
        assert np.array_equal(pairs, np.repeat([[T - abs(l)] for l in lags], N, axis=1))


@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
def test_the_gap_patterns_are_what_they_say(case):
    name, T, N, q, lags, pattern, min_pairs = case
    X = C.case_field(case)
    gone = np.isnan(X)
    xp, present, cn, n0 = C.centred(X)
    rho = C.lag1_field(xp, present, n0)
    if pattern == "none":
        assert not gone.any()
    elif pattern == "scattered":
        assert 0.05 < gone.mean() < 0.2 or N == 1
    elif pattern == "step":
        assert gone[T // 2].all() and not gone[T // 2 - 1].any()
    elif pattern == "column":
        assert gone[:, N // 3].all() and n0[N // 3] == 0 and cn[N // 3] == 0.0 and rho[N // 3] == 0.0
    elif pattern == "few":
        assert n0[3] == min_pairs - 1 and n0[N - 2] == min_pairs
    elif pattern == "run":
        runs = gone[:, 0].astype(int)
        assert runs.sum() > max(abs(l) for l in lags) and (N == 1 or not gone[:, 1].any())
    elif pattern == "edges":
        assert gone[:3].all() and gone[T - 2:].all() and not gone[3:T - 2].any()
    elif pattern == "alternate":
        assert n0[0] > min_pairs and rho[0] == 0.0 and rho[N // 2] == 0.0 and not (present[1:, 0] & present[:-1, 0]).any()
    elif pattern == "constant":
        assert (xp[:, 5] == 0.0).all() and (xp[:, N - 1] == 0.0).all() and gone[:, N - 1].any() and rho[5] == 0.0
        rest = C.reference(name, "float64", "n")[0]
        assert not rest["live"][:, 5].any() and not rest["live"][:, N - 1].any() and (rest["pairs"][:, 5] >= min_pairs).all()
    assert np.isfinite(X[~gone]).all() and 5.0 < np.nanmean(X)          # the offset is there: the centring matters


@pytest.mark.parametrize("dof", C.DOFS)
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
def test_the_restatement_stays_within_the_bound_of_the_truth_and_agrees_on_every_integer(case, dtype, dof):
    name, T, N, q, lags, pattern, min_pairs = case
    rest, truth, br, bs = C.reference(name, dtype, dof)
    live = truth["live"]
    assert np.array_equal(rest["pairs"], truth["pairs"]) and np.array_equal(rest["live"], live) and np.array_equal(rest["dof"], truth["dof"])
    assert np.array_equal(np.isnan(rest["r"]), ~live) and np.array_equal(np.isnan(rest["slope"]), ~live)
    assert np.array_equal(np.isnan(rest["p"]), ~live | (rest["dof"] < 3)) and (rest["dof"][~live] == 0).all()
    assert np.isfinite(br[live]).all() and np.isfinite(bs[live]).all() and (br[live] > 0).all()
    wr, ws = C.worst_ratio(rest["r"], truth["r"], br, live), C.worst_ratio(rest["slope"], truth["slope"], bs, live)
    print(name, dtype, dof, "live %d of %d" % (live.sum(), live.size), "error / bound: r %.3g slope %.3g" % (wr, ws))
    assert wr <= 1.0 and ws <= 1.0
    if dtype == "float64":
        assert wr <= 0.25 and ws <= 0.25          # (room for the device's fma against the restatement's multiply and add)


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
def test_no_integer_decision_of_a_committed_case_sits_on_its_threshold(case, dtype):
    """Conditions on the committed inputs: they let the GPU test demand exact `pairs`, `dof` and NaN positions on every entry."""
    name, T, N, q, lags, pattern, min_pairs = case
    for dof in C.DOFS:
        for res in C.reference(name, dtype, dof)[:2]:          # the float64 restatement and the longdouble truth
            m, f = res["moments"], res["centred"]
            enough = np.broadcast_to((m["n"] >= min_pairs)[..., None], f["live"].shape)
            with np.errstate(invalid="ignore", divide="ignore"):
                for c, s in ((np.broadcast_to(f["cxx"][..., None], f["live"].shape), np.broadcast_to(m["sxx"][..., None], f["live"].shape)),
                             (f["cyy"], m["syy"])):
                    ratio = np.where(s > 0, c / np.where(s > 0, s, 1), 0)
                    on_edge = enough & (c != 0) & (ratio < C.LIVE * 2.0 ** 10)          # exactly 0, or a factor 2^10 above 2^-40
                    assert not on_edge.any(), (name, dof, float(ratio[on_edge].min()))
            if dof == "bretherton":
                rho = np.broadcast_to(res["lag1"][None, :, None] * res["rho_y"][None, None, :], f["live"].shape)
                exact_zero = np.broadcast_to((res["lag1"] == 0)[None, :, None], f["live"].shape)
                assert not (f["live"] & ~exact_zero & (np.abs(rho) < 1e-9)).any()          # the sign of rho decides f = 1
                n = np.broadcast_to(m["n"][..., None], f["live"].shape)
                sel = f["live"] & (rho > 0)
                nf = res["nf"][sel]
                assert (np.abs(nf - np.round(nf)) > 1e-9 * n[sel]).all(), name
                assert (np.abs(rho[f["live"]]) < 1 - 1e-9).all()


def test_the_restated_p_value_is_scipys():
    import scipy.special
    worst = 0.0
    for name in ("tiny-ends", "two-pieces", "few", "long-lags", "q3-wide"):
        for dof in C.DOFS:
            rest = C.reference(name, "float64", dof)[0]
            ok = ~np.isnan(rest["p"])
            assert ok.any() and np.all((rest["p"][ok] >= 0) & (rest["p"][ok] <= 1))
            a = rest["dof"][ok] / 2 - 1
            ref = 2 * scipy.special.betainc(a, a, np.clip((1 - np.abs(rest["r"][ok])) / 2, 0, 1))
            big = ref >= 1e-290
            assert np.all(np.abs(rest["p"][ok][~big] - ref[~big]) <= 1e-289)
            worst = max(worst, float(np.max(np.abs(rest["p"][ok][big] - ref[big]) / ref[big])))
    print("restated p against scipy: worst relative difference %.3g" % worst)
    assert worst < 1e-11
    try:
        import mpmath
    except Exception:
        return
    mpmath.mp.dps = 40
    rest = C.reference("tiny-ends", "float64", "n")[0]
    for idx in list(zip(*np.nonzero(~np.isnan(rest["p"]))))[::97]:
        a = mpmath.mpf(int(rest["dof"][idx])) / 2 - 1
        want = 2 * mpmath.betainc(a, a, 0, (1 - abs(mpmath.mpf(float(rest["r"][idx])))) / 2, regularized=True)
        assert abs(rest["p"][idx] - float(want)) <= 1e-12 * float(want) + 1e-300


def test_a_dead_entry_and_a_short_dof_have_no_p_value():
    assert np.isnan(C.pvalue(np.array([0.3, np.nan, 0.3]), np.array([2, 10, 0]))).all()
    assert C.pvalue(np.array([1.0, -1.0]), np.array([5, 9])).tolist() == [0.0, 0.0]
    assert C.pvalue(np.array([0.0]), np.array([3]))[0] == pytest.approx(1.0, abs=1e-15)


# ---- the index rules of the moment kernel, against the definition -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny-one", "tiny-ends", "piece", "piece-plus", "q8-group", "q1-group", "q5-groups", "q8-plus", "run", "long-lags"])
def test_the_walk_of_the_moment_kernel_gives_the_bits_of_the_definition(name):
    case = C.case_by_name(name)
    X = C.case_field(case)
    yc, _ = lagged.center_index(C.case_index(case))
    xp, present, cn, n0 = C.centred(X)
    want = C.moments(xp, present, yc, list(case[4]))
    n, sx, sxx, sy, syy, sxy = C.kernel_walk(X, cn, yc, list(case[4]))
    assert np.array_equal(n, want["n"])
    for got, key in ((sx, "sx"), (sxx, "sxx"), (sy, "sy"), (syy, "syy"), (sxy, "sxy")):
        assert np.array_equal(got.view(np.uint64), want[key].view(np.uint64)), key


def test_the_output_of_a_lag_does_not_depend_on_the_other_lags_in_the_restatement():
    case = C.case_by_name("run")
    X, y, lags = C.case_field(case), C.case_index(case), list(case[4])
    whole = C.restate(X, y, lags, case[6], "bretherton")
    part = C.restate(X, y, lags[5:2:-1], case[6], "bretherton")
    for key in ("r", "slope", "p", "dof", "pairs"):
        assert np.array_equal(part[key], whole[key][5:2:-1], equal_nan=True), key


# ---- ABI and facade -------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entries_and_the_binding_has_them():
    for name, n_args in NEW.items():
        check_entry(name, n_args)
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version()
    text = header_text(comments=True)                 # (the stage names stand in a comment)
    for stage in ("lead_lag_center", "lead_lag_lag1", "lead_lag_moments", "lead_lag_finish"):
        assert '"%s"' % stage in text, stage
    assert callable(_hip.Handle.lead_lag_maps) and (_hip.DOF_N, _hip.DOF_BRETHERTON) == (0, 1)
    lib = _hip.load_library()
    import ctypes
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    g = (ctypes.c_int * 8)()
    assert lib.xmca_lead_lag_tile(ctypes.byref(a), ctypes.byref(b), None) == _hip.ERR_INVALID
    assert lib.xmca_lead_lag_tile(ctypes.byref(a), ctypes.byref(b), g) == 0 and (a.value, b.value, tuple(g)) == (256, 8, C.GROUPS)


def test_the_package_does_not_export_the_module():
    import xmca_amd
    assert "lead_lag_maps" not in xmca_amd.__all__ and "lagged" not in xmca_amd.__all__


def test_the_xarray_wrapper_has_the_parameters_of_lead_lag_maps():
    a = inspect.signature(lead_lag_maps).parameters
    b = inspect.signature(facade.lead_lag_maps).parameters
    assert list(a)[1:] == list(b)[1:] and list(b)[0] == "da"
    for name in list(a)[1:]:
        assert a[name].default == b[name].default and a[name].kind == b[name].kind, name


def test_the_xarray_wrapper_checks_before_the_device_and_wraps_the_maps():
    X = _field(T=24, N=6)
    da = xr.DataArray(X.reshape(24, 2, 3), dims=["time", "lat", "lon"],
                      coords={"time": np.arange(100, 124), "lat": [0.0, 1.0], "lon": [0.0, 1.0, 2.0]}, name="sst", attrs={"units": "K"})
    y = _index(T=24, q=2)
    index = xr.DataArray(y, dims=["time", "mode"], coords={"time": np.arange(100, 124)})
    with pytest.raises(ValueError, match="distinct"):
        facade.lead_lag_maps(da, index, [1, 1], handle=_NoDevice())
    with pytest.raises(AssertionError, match="device touched: lead_lag_maps"):
        facade.lead_lag_maps(da, index, [1, 0], handle=_NoDevice())
    with pytest.raises(TypeError, match="DataArray"):
        facade.lead_lag_maps(da.values, index, [0], handle=_NoDevice())
    lags = [2, -1, 0]
    out = facade.lead_lag_maps(da, index, lags, min_pairs=5, dof="bretherton", handle=_Restated())
    want = lead_lag_maps(X.reshape(24, 2, 3), y, lags, min_pairs=5, dof="bretherton", handle=_Restated())
    assert set(out) == set(want) == {"r", "slope", "p", "dof", "pairs", "lags", "lag1"}
    for key in ("r", "slope", "p", "dof"):
        assert tuple(out[key].dims) == ("lag", "lat", "lon", "index") and out[key].shape == (3, 2, 3, 2)
        assert np.array_equal(np.asarray(out[key].values), want[key], equal_nan=True)
        assert np.array_equal(np.asarray(out[key].coords["lag"].values), lags)
        assert np.array_equal(np.asarray(out[key].coords["lon"].values), [0.0, 1.0, 2.0])
        assert np.array_equal(np.asarray(out[key].coords["index"].values), [0, 1])
    assert tuple(out["pairs"].dims) == ("lag", "lat", "lon") and np.array_equal(np.asarray(out["pairs"].values), want["pairs"])
    assert tuple(out["lag1"].dims) == ("lat", "lon") and np.array_equal(np.asarray(out["lag1"].values), want["lag1"])
    assert tuple(out["lags"].dims) == ("lag",) and np.array_equal(np.asarray(out["lags"].values), lags)
    assert np.isfinite(np.asarray(out["r"].values)).any()
    one = facade.lead_lag_maps(da, y[:, 0], [0], handle=_Restated())
    assert one["r"].shape == (1, 2, 3, 1) and "lag1" not in one
