"""The host half of the facade's device route (`xmca_amd.xarray.xMCA.apply_weights`, no GPU needed).

a. `xMCA._column_factor`: the per-grid-point factor of a time-independent weight equals what the host route multiplies with,
   `(field * weight)[0] / field[0]` at the kept points.  The field holds signed powers of two, so that product and quotient are
   exact and the comparison is `array_equal`, not a tolerance;
b. weights the device route must leave to the host (a time dimension, a foreign dimension, an unknown key) give None;
c. the library exports the two weighted entry points, the binding knows them, and the ABI number did not move."""
import os
import sys

import numpy as np
import pytest

from abi_cases import check_entry, header_abi_version

try:
    import xarray as xr                      # the real package, where it exists
except Exception:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
    import xarray as xr

from xmca_amd.xarray import xMCA

T, NLAT, NLON = 6, 5, 7
LAT = np.linspace(-80, 80, NLAT)
LON = np.linspace(0, 90, NLON)


def _field(dtype=np.float64):
    rng = np.random.default_rng(3)
    v = (rng.choice([-1.0, 1.0], (T, NLAT, NLON)) * 2.0 ** rng.integers(-3, 4, (T, NLAT, NLON))).astype(dtype)
    v[:, 1, 2] = np.nan                      # a masked grid point: the factor is taken at the kept points only
    return xr.DataArray(v, dims=['time', 'lat', 'lon'], coords={'time': np.arange(T), 'lat': LAT, 'lon': LON})


def _model(dtype=np.float64):
    field = _field(dtype)
    return xMCA(field, preprocess='host'), field


def _weights(dtype=np.float64):
    rng = np.random.default_rng(4)
    lat = xr.DataArray(LAT.astype(dtype), dims=['lat'], coords={'lat': LAT})
    return {
        "lat": np.sqrt(np.cos(np.deg2rad(lat)) + 1e-6),
        "lat_lon": xr.DataArray(rng.uniform(0.5, 2.0, (NLAT, NLON)).astype(dtype), dims=['lat', 'lon'], coords={'lat': LAT, 'lon': LON}),
        "lon_lat": xr.DataArray(rng.uniform(0.5, 2.0, (NLON, NLAT)).astype(dtype), dims=['lon', 'lat'], coords={'lat': LAT, 'lon': LON}),
        "scalar": 1.75,
    }


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["lat", "lat_lon", "lon_lat", "scalar"])
def test_column_factor_is_the_host_product(name, dtype):
    xm, field = _model(dtype)
    weight = _weights(dtype)[name]
    keep = xm._no_nan_index['left']
    assert keep.sum() == NLAT * NLON - 1
    factor = xm._column_factor('left', weight)
    assert factor is not None and factor.shape == (keep.sum(),)
    assert factor.dtype == dtype                              # no promotion: the device may apply it
    product = np.asarray((field * weight).data)
    assert product.shape == field.shape and product.dtype == dtype
    expect = (product[0] / field.values[0]).reshape(-1)[keep]
    assert np.array_equal(factor, expect)
    # ... and at every time step, which is what "time-independent" means
    for t in range(T):
        assert np.array_equal(field.values[t].reshape(-1)[keep] * factor, product[t].reshape(-1)[keep])


def test_float64_weight_on_float32_field_changes_the_dtype():
    """the reference promotes such a field to float64: the factor says so, and `apply_weights` then takes the host route"""
    xm, field = _model(np.float32)
    factor = xm._column_factor('left', _weights(np.float64)["lat"])
    assert factor is not None and factor.dtype == np.float64
    assert not xm._apply_weights_on_device({'left': _weights(np.float64)["lat"]})


def test_time_dependent_weight_has_no_device_route():
    xm, field = _model()
    for n in (T, 1):
        w = xr.DataArray(np.linspace(1.0, 2.0, n), dims=['time'], coords={'time': np.arange(n)})
        assert xm._column_factor('left', w) is None
    w = xr.DataArray(np.full((T, NLAT), 1.5), dims=['time', 'lat'], coords={'time': np.arange(T), 'lat': LAT})
    assert xm._column_factor('left', w) is None


def test_foreign_dimension_has_no_device_route():
    xm, field = _model()
    w = xr.DataArray(np.full((NLAT, 3), 1.5), dims=['lat', 'level'], coords={'lat': LAT, 'level': np.arange(3)})
    assert xm._column_factor('left', w) is None
    w = xr.DataArray(np.full(3, 1.5), dims=['level'], coords={'level': np.arange(3)})
    assert xm._column_factor('left', w) is None


def test_unknown_key_and_host_model_take_the_host_route():
    xm, field = _model()
    w = _weights()["lat"]
    assert xm._column_factor('right', w) is None and xm._column_factor('middle', w) is None
    assert not xm._apply_weights_on_device({'left': w})       # preprocess='host': nothing is resident
    with pytest.raises(KeyError, match="Please use `left` or `right`"):
        xm.apply_weights(middle=w)
    before = xm.fields()['left'].values
    xm.apply_weights(left=w)                                  # the reference's host code, unchanged
    after = xm.fields()['left'].values
    assert np.array_equal(after, np.asarray((xr.DataArray(before, dims=field.dims, coords=field.coords) * w).data), equal_nan=True)


def test_column_weights_hook():
    from xmca_amd.array import MCA
    xm, field = _model()
    assert MCA._device_column_weights(xm, 'left') is None
    assert xm._device_column_weights('left') is None
    xm.apply_coslat()
    fwd, inv = xm._device_column_weights('left')
    assert np.array_equal(fwd, xm._coslat_weights('left')) and np.array_equal(inv, fwd)      # sqrt(cos(lat)), without the 1e-6
    assert fwd.dtype == np.float64 and fwd.shape == (xm._no_nan_index['left'].sum(),)
    xm.normalize()                                            # clears the flag, as in the reference
    assert xm._device_column_weights('left') is None


def test_weighted_entry_points_are_exported_and_bound():
    from xmca_amd import _hip
    for name in ("xmca_predict_weighted", "xmca_reconstruct_weighted"):
        check_entry(name)
    # the arguments of the unweighted entry point plus one pointer
    for name in ("xmca_predict", "xmca_reconstruct"):
        res, args = _hip.SIGNATURES[name]
        wres, wargs = _hip.SIGNATURES[name + "_weighted"]
        assert wres is res and wargs[:-1] == args and wargs[-1] is _hip._vp


def test_abi_version_is_unchanged():
    from xmca_amd import _hip
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version()
