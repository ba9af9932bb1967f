"""CPU: xmca_get_maps is declared, exported and bound with the header's argument count under the unchanged ABI number, and the class
reaches it only with vectors resident on the device and without `_maps_on_host` (a stub device whose `maps` raises)."""
import numpy as np
import pytest

from abi_cases import check_entry, header_abi_version, header_define


def test_maps_entry_point_is_declared_exported_and_bound():
    from xmca_amd import _hip
    check_entry("xmca_get_maps", 15)
    assert hasattr(_hip.Handle, "maps")
    for name, value in (("XMCA_MAP_EOF", _hip.MAP_EOF), ("XMCA_MAP_AMPLITUDE", _hip.MAP_AMPLITUDE), ("XMCA_MAP_PHASE", _hip.MAP_PHASE),
                        ("XMCA_SCALE_NONE", _hip.SCALE_NONE), ("XMCA_SCALE_MAX", _hip.SCALE_MAX), ("XMCA_SCALE_STD", _hip.SCALE_STD)):
        assert header_define(name) == value, name


def test_abi_number_is_unchanged_by_the_added_entry_point():
    from xmca_amd import _hip
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version()


class _StubDevice:
    """Holds the 'resident' vectors of one model: `eofs` answers like xmca_get_eofs (no mixing matrix), `maps` records and raises."""

    def __init__(self, V):
        self.V = V                       # side -> (N', rank)
        self.maps_calls = 0

    def holds_result_of(self, holder):
        return True

    def eofs(self, side, N, m, W, dtype):
        assert W is None
        return np.array(self.V[side][:, :m], dtype=dtype, order='C')

    def vectors(self, side, n_modes, N, dtype):
        raise AssertionError("the vectors must not be fetched")

    def maps(self, *args, **kwargs):
        self.maps_calls += 1
        raise AssertionError("Handle.maps reached")


def _model(resident, masked=True, dtype=np.float64):
    from xmca_amd.array import MCA, _LazyVectors
    rng = np.random.default_rng(3)
    field = rng.standard_normal((12, 5, 7)).astype(dtype)
    if masked:
        field[:, 1, 2:5] = np.nan
    m = MCA(field, preprocess='host')
    N, r = m._fields['left'].shape[1], 6
    V = np.linalg.qr(rng.standard_normal((N, r)))[0].astype(dtype)
    sv = np.linspace(9.0, 1.0, r)
    stub = _StubDevice({0: V})
    m._handle_override = stub
    m._V = _LazyVectors(stub, {'left': (0, N)}, r, dtype) if resident else {'left': V}
    m._singular_values, m._variance = sv, sv
    m._var_idx = np.arange(r)
    m._norm = {'left': np.sqrt(sv)}
    m._analysis.update({'rank': r, 'n_rot': r, 'total_covariance': sv.sum(), 'total_squared_covariance': (sv ** 2).sum()})
    return m, stub, V


def _expected(m, V, q, scaling):
    e = np.full((m._n_variables['left'], q), np.nan)
    e[m._no_nan_index['left']] = V[:, :q]
    if scaling == 'max':
        e = e / np.nanmax(np.abs(e), axis=0)
    elif scaling == 'std':
        e = e / np.nanstd(e, axis=0)
    elif scaling == 'eigen':
        e = e * m._norm['left'][:q]
    return e.reshape(m._fields_spatial_shape['left'] + (q,))


@pytest.mark.parametrize("resident", [False, True])
def test_host_vectors_and_maps_on_host_never_reach_the_device_maps(resident):
    """injected host vectors (no device at all), and resident vectors under `_maps_on_host` (today's route: the device mixes, numpy
    scales and masks): the numpy code answers, with the reference's formulas"""
    m, stub, V = _model(resident)
    if resident:
        m._maps_on_host = True
    for scaling in ('None', 'max', 'std', 'eigen'):
        got = m.eofs(3, scaling=scaling)['left']
        want = _expected(m, V, 3, scaling)
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
        assert np.allclose(got, want, rtol=1e-14, atol=0, equal_nan=True), scaling
    amp = m.spatial_amplitude(3, scaling='max')['left']
    want = np.abs(_expected(m, V, 3, 'None'))
    assert np.allclose(amp, want / np.nanmax(want, axis=(0, 1)), rtol=1e-14, atol=0, equal_nan=True)
    ph = m.spatial_phase(3)['left']
    assert np.array_equal(ph[~np.isnan(ph)], np.where(_expected(m, V, 3, 'None')[~np.isnan(ph)] < 0, np.pi, 0.0))
    assert stub.maps_calls == 0
    with pytest.raises(ValueError):
        m.eofs(3, scaling='bogus')


def test_resident_vectors_take_the_device_maps():
    """... and without the switch every scaled, masked, amplitude or phase request goes to `Handle.maps` (the stub's raises); only the
    bare eofs of an unmasked field stay with xmca_get_eofs"""
    m, stub, V = _model(True)
    calls = [lambda: m.eofs(3, scaling='max'), lambda: m.eofs(3, scaling='std'), lambda: m.eofs(3, scaling='eigen'), lambda: m.eofs(3),
             lambda: m.spatial_amplitude(3), lambda: m.spatial_amplitude(3, scaling='max'), lambda: m.spatial_phase(3)]
    for i, call in enumerate(calls):
        with pytest.raises(AssertionError, match="Handle.maps reached"):
            call()
        assert stub.maps_calls == i + 1
    m, stub, V = _model(True, masked=False)
    assert np.array_equal(m.eofs(3)['left'].reshape(-1, 3), V[:, :3]) and stub.maps_calls == 0
    with pytest.raises(AssertionError, match="Handle.maps reached"):
        m.eofs(3, scaling='max')
    with pytest.raises(ValueError):
        m.eofs(3, scaling='bogus')


def test_float32_std_keeps_the_reference_arithmetic():
    """a float32 result scaled by 'std' is divided by numpy's float32 `nanstd`, as the reference does: the device's float64 sums are
    another number at large N.  Every other request of the float32 model goes to the device"""
    m, stub, V = _model(True, dtype=np.float32)
    got = m.eofs(3, scaling='std')['left']
    e = np.full((m._n_variables['left'], 3), np.nan, dtype=np.float32)
    e[m._no_nan_index['left']] = V[:, :3]
    want = (e / np.nanstd(e, axis=0)).reshape(got.shape)
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True) and stub.maps_calls == 0
    for call in (lambda: m.eofs(3, scaling='max'), lambda: m.eofs(3), lambda: m.spatial_amplitude(3, scaling='max')):
        with pytest.raises(AssertionError, match="Handle.maps reached"):
            call()
    assert stub.maps_calls == 3
