"""The xarray facade on the device: `xMCA.apply_weights` / `apply_coslat` on the resident field, `predict` and
`reconstructed_fields` with the coslat weights in the ingest and in the reconstruction epilogue (xmca_predict_weighted /
xmca_reconstruct_weighted).

1. `apply_coslat` crosses no PCIe and leaves the bits of the host route;
2. model level, the device route against the host route (`_transform_on_host`), the call list of tests/test_gpu_transform.py;
3. handle level against numpy: the weighted ingest bit for bit, the weighted epilogue to the float64 tolerance, no weights = the
   unweighted entry points to the bit;
4. a row at the pole (inverse weight sqrt(cos(90 deg)) = 7.8e-9) stays finite, column by column as accurate as the rest;
5. predict(training data) = pcs().

Fields: (72, 9, 14) with one masked grid point and (72, 9, 11); one field (40, 5, 53), N' = 265 = 256 + 9 = 4 * 64 + 9: neither
a multiple of the 256-thread block nor of the 64-lane wavefront."""
import os
import sys

import numpy as np
import pytest

try:
    import xarray as xr                      # the real package, where it exists
except Exception:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
    import xarray as xr

from xmca_amd import _hip
from xmca_amd.array import MCA
from xmca_amd.xarray import xMCA

pytestmark = pytest.mark.gpu

T = 72


def _da(values, lat, lon):
    return xr.DataArray(values, dims=['time', 'lat', 'lon'], coords={'time': np.arange(values.shape[0]), 'lat': lat, 'lon': lon})


def _pair(dtype=np.float64, lat_max=60.0, dyadic=False):
    """the two fields of tests/test_gpu_xarray_facade.py: four planted modes plus noise, one masked grid point on the left.
    dyadic: values rounded to multiples of 2^-16, so that every column sum - in any order - and with it the column mean is
    the same float64 on the host and on the device (the comparison of test 1 is about the weights, not about summation order)."""
    rng = np.random.default_rng(12)
    nlat, nlon = 9, 14
    lat = np.linspace(-lat_max, lat_max, nlat).astype(dtype)
    lon = np.linspace(0, 130, nlon)
    pcs = rng.standard_normal((T, 4)) * np.array([6.0, 4.0, 2.5, 1.5])
    a = (pcs @ rng.standard_normal((4, nlat * nlon)) + 0.4 * rng.standard_normal((T, nlat * nlon))).reshape(T, nlat, nlon)
    b = (pcs @ rng.standard_normal((4, nlat * (nlon - 3))) + 0.4 * rng.standard_normal((T, nlat * (nlon - 3)))).reshape(T, nlat, nlon - 3)
    if dyadic:
        a, b = np.round(a * 65536.0) / 65536.0, np.round(b * 65536.0) / 65536.0
    a[:, 2, 3] = np.nan
    return _da(a.astype(dtype), lat, lon), _da(b.astype(dtype), lat, lon[:-3])


def _single(lat=None, dyadic=False):
    rng = np.random.default_rng(13)
    t, nlat, nlon = 40, 5, 53
    lat = np.linspace(-70, 70, nlat) if lat is None else np.asarray(lat, dtype=np.float64)
    pcs = rng.standard_normal((t, 3)) * np.array([5.0, 3.0, 2.0])
    a = (2.0 + pcs @ rng.standard_normal((3, nlat * nlon)) + 0.4 * rng.standard_normal((t, nlat * nlon))).reshape(t, nlat, nlon)
    if dyadic:
        a = np.round(a * 65536.0) / 65536.0
    return (_da(a, lat, np.linspace(0, 340, nlon)),)


def _scale(a):
    return max(float(np.nanmax(np.abs(a))), 1e-300)


# ----------------------------------------------------------------------------------------------
# 1. apply_coslat on the resident field
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["pair", "single"])
def test_apply_coslat_crosses_no_pcie_and_has_the_bits_of_the_host_route(monkeypatch, which):
    fields = _pair(dyadic=True) if which == "pair" else _single(dyadic=True)
    count = {"get_field": 0, "set_field": 0}
    for name in count:
        def counted(self, *args, _name=name, _orig=getattr(_hip.Handle, name), **kwargs):
            count[_name] += 1
            return _orig(self, *args, **kwargs)
        monkeypatch.setattr(_hip.Handle, name, counted)
    xm = xMCA(*fields)
    dev = xm._device()
    after_ctor, owner = dict(count), dev.fields_owner
    assert after_ctor == {"get_field": 0, "set_field": len(fields)} and xm._store_is_raw and owner is not None
    xm.apply_coslat()
    assert count == after_ctor                       # no download, no upload
    assert xm._store_is_raw
    assert dev.fields_owner == owner
    assert xm._analysis['is_coslat_corrected']
    ref = xMCA(*fields, preprocess='host')
    ref.apply_coslat()
    got, exp = xm.fields(), ref.fields()
    for k in xm._keys:
        a, b = np.asarray(got[k].values), np.asarray(exp[k].values)
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.array_equal(a, b, equal_nan=True), (k, np.nanmax(np.abs(a - b)))
    assert np.isnan(np.asarray(got['left'].values)).any() == (which == "pair")


def test_apply_weights_falls_back_to_the_host_for_what_the_device_cannot_do():
    """a time-dependent weight and a dtype-promoting one: the reference's host code, the field leaves the device"""
    left, right = _pair(np.float32)
    w_time = xr.DataArray(np.linspace(1.0, 2.0, T).astype(np.float32), dims=['time'], coords={'time': np.arange(T)})
    w_f64 = xr.DataArray(np.linspace(0.5, 1.5, 9), dims=['lat'], coords={'lat': left.coords['lat'].values})
    for w, dtype in ((w_time, np.float32), (w_f64, np.float64)):
        xm, ref = xMCA(left, right), xMCA(left, right, preprocess='host')
        xm.apply_weights(left=w)
        ref.apply_weights(left=w)
        assert not xm._store_is_raw
        a, b = xm.fields()['left'].values, ref.fields()['left'].values
        assert a.dtype == b.dtype == dtype and a.shape == b.shape
        assert np.nanmax(np.abs(a - b)) <= 2e-6 * _scale(b)       # (float32 means: float64 sums on the device, float32 on the host)
    with pytest.raises(KeyError, match="Please use `left` or `right`"):
        xMCA(left, right).apply_weights(middle=w_f64)


# ----------------------------------------------------------------------------------------------
# 2. model level: device route against `_transform_on_host`
# ----------------------------------------------------------------------------------------------
def _model(name):
    if name == "single":
        fields = _single()
    else:
        fields = _pair(np.float32 if name == "f32" else np.float64)
    m = xMCA(*fields)
    if name == "norm_coslat":
        m.normalize()
        m.apply_coslat()
    elif name.startswith("coslat_norm"):
        m.apply_coslat()
        m.normalize()
    else:
        m.apply_coslat()
    m.solve(complexify=(name == "cplx_rot"))
    if name in ("coslat_rot", "coslat_norm_rot"):
        m.rotate(4, 2)
    elif name == "cplx_rot":
        m.rotate(4, 4)
    return m, fields


def _calls(fields):
    """the call list of tests/test_gpu_transform.py::_calls, the new data as DataArrays"""
    new = [_da(np.asarray(f.values)[:37] * f.dtype.type(1.1), f.coords['lat'].values, f.coords['lon'].values) for f in fields]
    calls = [("predict", dict(n=None)), ("predict", dict(n=3, scaling='eigen', phase_shift=0.4)),
             ("predict", dict(n=5, scaling='max')), ("predict", dict(n=4, scaling='std'))]
    calls += [("rec", dict(mode=mode, original_scale=o)) for mode in (None, 3, slice(2, 6)) for o in (True, False)]
    calls += [("recX", dict(mode=slice(2, 6), original_scale=True)), ("recX", dict(mode=0, original_scale=False))]
    return new, calls


def _run(m, new, calls):
    out = []
    for what, kw in calls:
        if what == "predict":
            res = m.predict(*new, **kw)
        elif what == "rec":
            res = m.reconstructed_fields(**kw)
        else:
            res = m._reconstructed_X(**kw)
        out.append({k: np.asarray(getattr(v, 'values', v)) for k, v in res.items()})
    return out


# (an unrotated model projects on all `rank` modes: where the null mode of the centered field has sigma = 0 exactly - coslat_norm,
#  f32 - the reference's 0 / 0 makes predict() and the all-mode reconstruction NaN in both routes; coslat_norm_rot mixes four modes
#  only, so that the numbers of a model with the flag cleared are compared in every call)
@pytest.mark.parametrize("name", ["coslat", "coslat_rot", "norm_coslat", "coslat_norm", "coslat_norm_rot", "cplx_rot", "f32", "single"])
def test_facade_device_route_matches_host_route(name):
    m, fields = _model(name)
    assert m._store_is_raw                                        # the weights never brought the field to the host
    assert m._analysis['is_coslat_corrected'] == (not name.startswith("coslat_norm"))
    assert (m._device_column_weights('left') is None) == name.startswith("coslat_norm")
    new, calls = _calls(fields)
    for k in m._keys:
        assert m._transform_vectors(k) is not None
    dev = _run(m, new, calls)
    assert m._V._pending == set(m._keys)            # the device route fetched nothing
    m._transform_on_host = True
    for k in m._keys:
        assert m._transform_vectors(k) is None
    host = _run(m, new, calls)
    tol = 2e-5 if fields[0].dtype == np.float32 else 1e-10
    for (what, kw), d, r in zip(calls, dev, host):
        for k in m._keys:
            a, b = d[k], r[k]
            assert a.shape == b.shape and a.dtype == b.dtype, (what, kw, k, a.dtype, b.dtype)
            assert np.array_equal(np.isnan(a), np.isnan(b)), (what, kw, k)
            if np.isfinite(b).any():          # (a float32 model whose null mode has sigma = 0: 0 / 0 makes both routes all NaN)
                err, scale = float(np.nanmax(np.abs(a - b))), _scale(b)
                print(name, what, kw, k, "max|a - b| = %.3e, scale(b) = %.3e" % (err, scale))
                assert err <= tol * scale, (what, kw, k, err / scale)
    if name.endswith("_rot") or name in ("coslat", "norm_coslat", "single"):      # the numbers of every call were compared
        assert all(np.isfinite(r[k]).any() for r in host for k in m._keys)


def test_subclass_with_its_own_scaling_and_no_hook_keeps_the_host_route():
    class Scaled(xMCA):
        def _scale_X(self, data_dict):
            return super()._scale_X(data_dict)

        _device_column_weights = MCA._device_column_weights       # the array class's: "nothing stated"

    m = Scaled(*_single())
    m.solve()
    assert m._transform_vectors('left') is None


# ----------------------------------------------------------------------------------------------
# 3. the weighted entry points against numpy
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h():
    handle = _hip.Handle(0)
    yield handle
    handle.close()


N_KEEP, N_FULL = 265, 271


def _solved(h, rng):
    X0 = rng.standard_normal((64, N_KEEP))
    h.set_field(0, X0 - X0.mean(axis=0))
    rank = h.solve(1)
    return h.vectors(0, rank, N_KEEP, np.float64).T


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_weighted_ingest_is_bitwise(h, dtype):
    rng = np.random.default_rng(5)
    _solved(h, rng)
    keep = np.sort(rng.choice(N_FULL, N_KEEP, replace=False))
    X = (5.0 + 3.0 * rng.standard_normal((41, N_FULL))).astype(dtype)
    mean = rng.standard_normal(N_KEEP).astype(dtype)
    std = rng.uniform(0.3, 3.0, N_KEEP).astype(dtype)
    w = rng.uniform(1e-3, 1.0, N_KEEP)
    # a selection matrix as vectors and the identity as mix: the output is the ingested block itself
    eye = np.eye(N_KEEP)
    got = h.predict(0, X, keep, mean, std, eye, eye, weight=w)
    x = X[:, keep].copy()
    x -= mean
    x /= std
    x *= w                                            # float64 w: the product in double, rounded to the data's dtype
    assert x.dtype == dtype
    assert np.array_equal(got, x.astype(np.float64))
    sel = eye[:, ::-1][:, :7]                         # seven columns, reversed
    got = h.predict(0, X, keep, mean, std, sel, np.eye(7), weight=w)
    assert np.array_equal(got, x[:, ::-1][:, :7].astype(np.float64))
    got = h.predict(0, np.ascontiguousarray(X[:, keep]), None, mean, None, eye, eye, weight=w)     # contiguous, no division
    x = X[:, keep] - mean
    x *= w
    assert np.array_equal(got, x.astype(np.float64))
    # no weights: the unweighted entry point; weights of one: its bits through the weighted one
    a = h.predict(0, X, keep, mean, std, eye, eye)
    assert np.array_equal(a, h.predict(0, X, keep, mean, std, eye, eye, weight=None))
    assert np.array_equal(a, h.predict(0, X, keep, mean, std, eye, eye, weight=np.ones(N_KEEP)))
    with pytest.raises(ValueError):
        h.predict(0, X, keep, mean, std, eye, eye, weight=np.ones(N_KEEP + 1))


@pytest.mark.parametrize("resident", [True, False])
def test_weighted_epilogue_matches_numpy(h, resident):
    rng = np.random.default_rng(6)
    V = _solved(h, rng)
    keep = np.sort(rng.choice(N_FULL, N_KEEP, replace=False))
    masked = np.setdiff1d(np.arange(N_FULL), keep)
    mean = rng.standard_normal(N_KEEP)
    std = rng.uniform(0.5, 2.0, N_KEEP)
    w = rng.uniform(0.05, 1.0, N_KEEP)
    for m in (0, 1, 7):
        B = rng.standard_normal((5, m))
        Vh = None if resident else V[:, :m]
        core = B @ V[:, :m].T
        for kw, ref in ((dict(mean=mean, std=std), core / w * std + mean), (dict(mean=mean), core / w + mean), (dict(), core / w)):
            got = h.reconstruct(0, B, Vh, N_KEEP, keep_idx=keep, N_full=N_FULL, inv_weight=w, **kw)
            assert got.shape == (5, N_FULL) and got.dtype == np.float64
            assert np.isnan(got[:, masked]).all() and not np.isnan(got[:, keep]).any()
            assert np.max(np.abs(got[:, keep] - ref)) <= 1e-10 * _scale(ref), (m, sorted(kw))
        got = h.reconstruct(0, B, Vh, N_KEEP, inv_weight=w)                    # compact
        assert got.shape == (5, N_KEEP) and np.max(np.abs(got - core / w)) <= 1e-10 * _scale(core / w)
        a = h.reconstruct(0, B, Vh, N_KEEP, keep_idx=keep, N_full=N_FULL, mean=mean, std=std)
        for none_or_one in (None, np.ones(N_KEEP)):
            b = h.reconstruct(0, B, Vh, N_KEEP, keep_idx=keep, N_full=N_FULL, mean=mean, std=std, inv_weight=none_or_one)
            assert np.array_equal(a, b, equal_nan=True)
    # an IEEE division: a zero weight gives inf / NaN as numpy does, nothing else moves
    w0 = w.copy()
    w0[3] = 0.0
    B = rng.standard_normal((5, 7))
    got = h.reconstruct(0, B, None if resident else V[:, :7], N_KEEP, inv_weight=w0)
    assert not np.isfinite(got[:, 3]).any() and np.isfinite(np.delete(got, 3, axis=1)).all()


# ----------------------------------------------------------------------------------------------
# 4. a row at the pole
# ----------------------------------------------------------------------------------------------
def test_pole_row_is_finite_and_accurate_per_column():
    lat = [-60.0, -30.0, 0.0, 45.0, 90.0]
    (field,) = _single(lat)
    m = xMCA(field)
    m.apply_coslat()
    m.solve()
    inv = m._device_column_weights('left')[1]
    assert inv.min() == np.sqrt(np.cos(np.deg2rad(90.0))) and 7.8e-9 < inv.min() < 7.9e-9
    # (39 = every mode but the null mode of the centered 40-step field, whose sigma = 0 makes both routes NaN: the reference's 0 / 0)
    for mode in (39, 3):
        m._transform_on_host = False
        a = np.asarray(m.reconstructed_fields(mode, original_scale=True)['left'].values)
        assert m._V._pending == {'left'}
        m._transform_on_host = True
        b = np.asarray(m.reconstructed_fields(mode, original_scale=True)['left'].values)
        assert a.shape == b.shape == field.shape and a.dtype == b.dtype
        assert np.isfinite(a[np.isfinite(b)]).all() and np.isfinite(b).all()
        a2, b2 = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
        err = np.max(np.abs(a2 - b2), axis=0) / np.max(np.abs(b2), axis=0)     # per column, relative to the column's own maximum
        print("mode", mode, "worst column: %.3e" % err.max(), "pole row: %.3e" % err.reshape(field.shape[1:])[-1].max())
        assert err.max() <= 1e-10
        if mode == 39:          # all modes: the pole row comes back (x sqrt((cos + 1e-6) / cos), the reference's quirk) - a large factor
            ratio = np.abs(b[:, -1] - b[:, -1].mean(axis=0)).max() / np.abs(field.values[:, -1] - field.values[:, -1].mean(axis=0)).max()
            assert 1e5 < ratio < 2e5


# ----------------------------------------------------------------------------------------------
# 5. predict(training data) = pcs()
# ----------------------------------------------------------------------------------------------
def test_predict_of_training_data_is_pcs():
    """`apply_coslat` weights the training field by sqrt(cos(lat) + 1e-6), `predict` the new data by sqrt(cos(lat)) - the
    reference's quirk - so the two differ by the relative 1e-6 / (2 cos(lat)) per grid point whatever computes them.  Its part
    common to all latitudes rescales the PCs, its variation over the grid mixes other modes in.  Latitudes within +-20 degrees
    (5.0e-7 ... 5.3e-7, variation 3e-8) and the four planted modes keep that - 0.6 of the bound in a float64 model of this
    very sequence in numpy - inside rtol = 1e-6, atol = 1e-8, so the bound is left to test the projection."""
    left, right = _pair(lat_max=20.0)
    m = xMCA(left, right)
    m.apply_coslat()
    m.solve()
    pcs = m.pcs(4)
    new = m.predict(left, right, n=4)
    assert m._V._pending == set(m._keys)
    for k in m._keys:
        a, b = np.asarray(new[k].values), np.asarray(pcs[k].values)
        assert a.shape == b.shape == (T, 4)
        print(k, "worst |a - b| / (atol + rtol |b|) = %.3f" % np.max(np.abs(a - b) / (1e-8 + 1e-6 * np.abs(b))))
        assert np.allclose(a, b, rtol=1e-6, atol=1e-8)
