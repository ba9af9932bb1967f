"""CPU: `extended_eofs` without a device - the argument rules on a handle stub that fails on any device call, the
identity behind the device route (lag-summed, doubly centred Gram matrix against the SVD of the explicitly embedded, centred
matrix; tests/extended_eofs_cases.py), the gap condition of every vector-comparison case, the three ABI entries, and the facade
on a recorder."""
import inspect
import os
import sys

import numpy as np
import pytest

import extended_eofs_cases as C
from abi_cases import check_entry, header_abi_version
from xmca_amd import _hip
from xmca_amd.array import MCA

try:
    import xarray as xr                      # the real package, where it exists
except Exception:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
    import xarray as xr

from xmca_amd.xarray import xMCA

NEW = {"xmca_extended_eofs": 9, "xmca_lag_gram": 7, "xmca_lag_gram_tile": 0}
# bounds of the identity: 30-100 x the 1e-15 / 6e-14 / 2e-12 measured when the identity was derived
BOUND_LAM, BOUND_EOFS, BOUND_PCS = 1e-13, 1e-11, 1e-10


class _NoDevice:
    """a handle that fails the test when anything reaches it"""

    def __getattr__(self, name):
        raise AssertionError("device touched: " + name)


def _model(T=12, N=7, two=False):
    rng = np.random.default_rng(5)
    fields = [rng.standard_normal((T, N))] + ([rng.standard_normal((T, N + 1))] if two else [])
    return MCA(*fields, handle=_NoDevice(), preprocess="host")


# ---- argument rules -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, -1, 2.5, True, "3", np.float64(4.0), None])
def test_bad_embedding_and_tau_raise_before_any_device_work(bad):
    m = _model()
    with pytest.raises(ValueError, match="embedding"):
        m.extended_eofs(bad)
    with pytest.raises(ValueError, match="tau"):
        m.extended_eofs(2, tau=bad)


@pytest.mark.parametrize("M,tau", [(12, 1), (13, 1), (4, 4), (2, 11), (100, 100)])
def test_a_window_of_fewer_than_two_steps_is_refused(M, tau):
    with pytest.raises(ValueError, match="at least 2"):
        _model(T=12).extended_eofs(M, tau=tau, n_modes=1)


@pytest.mark.parametrize("bad", [0, -2, 1.0, False, "2", None, np.float32(2)])
def test_bad_n_modes_raise_before_any_device_work(bad):
    with pytest.raises(ValueError, match="n_modes"):
        _model().extended_eofs(2, n_modes=bad)


def test_n_modes_is_bounded_by_the_rank_of_the_centred_embedded_matrix():
    # T' - 1 binds: T = 12, M = 3, tau = 2 -> T' = 8, M N = 21
    with pytest.raises(ValueError, match="n_modes"):
        _model(T=12, N=7).extended_eofs(3, tau=2, n_modes=8)
    # M N binds: T = 12, N = 2, M = 2 -> T' = 11, M N = 4
    with pytest.raises(ValueError, match="n_modes"):
        _model(T=12, N=2).extended_eofs(2, n_modes=5)
    # the default of 10 modes is checked like a given one
    with pytest.raises(ValueError, match="n_modes"):
        _model(T=12, N=7).extended_eofs(3, tau=2)


def test_two_fields_and_complex_models_are_refused():
    with pytest.raises(ValueError, match="one field"):
        _model(two=True).extended_eofs(2, n_modes=1)
    m = _model()
    m._analysis['is_complex'] = True
    with pytest.raises(ValueError, match="complex"):
        m.extended_eofs(2, n_modes=1)


def test_signatures():
    p = inspect.signature(MCA.extended_eofs).parameters
    assert list(p) == ["self", "embedding", "tau", "n_modes"]
    assert [p[k].default for k in list(p)[2:]] == [1, 10]
    q = inspect.signature(MCA.solve).parameters
    assert list(q) == ["self", "complexify", "extend", "period", "n_modes"]
    assert [q[k].default for k in list(q)[1:]] == [False, False, 1, None]


# ---- the identity -------------------------------------------------------------------------------------------------------
def _cases():
    out = [(name, C.case_field(T, N, seed), M, tau, k) for name, T, N, M, tau, k, seed in C.IDENTITY_CASES + [C.LARGE_CASE]]
    name, T, shape, masked, M, tau, k, seed = C.MASKED_CASE
    out.append((name, C.masked_field(T, shape, masked, seed)[1], M, tau, k))
    out.append(("40x23_M1", C.case_field(40, 23, 0), 1, 1, 3))
    return out


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_every_vector_case_has_the_gap_the_comparison_needs(case):
    _, X, M, tau, k = case
    gaps = C.relgaps(C.svd_truth(X, M, tau, k)["lam"], k)
    assert gaps.min() >= C.MIN_RELGAP, gaps


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_lag_summed_centred_gram_route_is_the_svd_of_the_embedded_matrix(case):
    _, X, M, tau, k = case
    ref, res = C.svd_truth(X, M, tau, k), C.gram_route(X, M, tau, k)
    n = min(len(ref["lam"]), X.shape[1] * M)
    assert np.max(np.abs(res["lam"][:n] - ref["lam"][:n])) <= BOUND_LAM * ref["lam"][0]
    err = C.errors(res, ref)
    assert err["eofs"] <= BOUND_EOFS and err["pcs"] <= BOUND_PCS, err
    assert np.allclose(np.sum(res["eofs"] ** 2, axis=(0, 1)), 1.0, atol=1e-12)


@pytest.mark.parametrize("case", [c for c in CASES if c[2] > 1 and c[0] != C.LARGE_CASE[0]], ids=lambda c: c[0])
def test_the_route_without_the_centring_is_wrong_by_orders_of_magnitude(case):
    """the trend of the inputs makes the window means differ from lag to lag: leaving H K H out must be visible (the large case,
    one step of 800, is there for the eigensolver's route and moves its means too little to count here)"""
    _, X, M, tau, k = case
    ref, res = C.svd_truth(X, M, tau, k), C.gram_route(X, M, tau, k, center=False)
    err = C.errors(res, ref)
    assert abs(res["lam"][0] - ref["lam"][0]) > 1e6 * BOUND_LAM * ref["lam"][0]
    assert err["eofs"] > 1e6 * BOUND_EOFS


def test_the_input_generator_moves_the_window_means():
    """means of the embedded columns in units of their standard deviation: at least 0.1 in every case (the shortest shift, 3 of 40
    steps), above 1 where the windows are half the record apart"""
    worst = {}
    for name, T, N, M, tau, k, seed in C.E2E_CASES:
        Y = C.embed(C.case_field(T, N, seed), M, tau)
        worst[name] = (np.abs(Y.mean(axis=0)) / Y.std(axis=0)).max()
    assert min(worst.values()) > 0.1 and max(worst.values()) > 1.0, worst


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_bound_and_the_abi_number_stays():
    for name, n_args in NEW.items():
        check_entry(name, n_args)
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version()


def test_the_tile_is_a_constant_of_the_build_known_without_a_device():
    tile = _hip.lag_gram_tile()
    assert isinstance(tile, int) and tile >= 8 and tile == _hip.lag_gram_tile()


# ---- facade -------------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the handle: owns the fields, records the one device call and answers it from the numpy truth"""

    def __init__(self, X):
        self.X = X
        self.calls = []
        self.fields_owner = None

    def extended_eofs(self, T, N, M, tau, k, keep_idx, N_full):
        self.calls.append((T, N, M, tau, k, None if keep_idx is None else tuple(keep_idx), N_full))
        ref = C.svd_truth(self.X, M, tau, k)
        eofs = np.full((M, N_full, k), np.nan)
        eofs[:, slice(None) if keep_idx is None else keep_idx] = ref["eofs"]
        return ref["lam"], ref["pcs"], eofs


def test_facade_wraps_patterns_with_a_lag_dimension_and_pcs_over_the_first_windows():
    T, nlat, nlon, M, tau, k = 20, 3, 4, 3, 2, 2
    rng = np.random.default_rng(7)
    v = rng.standard_normal((T, nlat, nlon))
    v[:, 1, 2] = np.nan
    time = np.arange(100, 100 + T)
    lat, lon = np.linspace(-10, 10, nlat), np.linspace(0, 30, nlon)
    xm = xMCA(xr.DataArray(v, dims=['time', 'lat', 'lon'], coords={'time': time, 'lat': lat, 'lon': lon}), preprocess='host')
    keep = xm._no_nan_index['left']
    rec = _Recorder(np.asarray(xm._fields['left'], dtype=np.float64))
    xm._handle_override = rec
    rec.fields_owner = xm._owner_key()
    out = xm.extended_eofs(M, tau=tau, n_modes=k)
    Tp = T - (M - 1) * tau
    assert rec.calls == [(T, int(keep.sum()), M, tau, k, tuple(np.flatnonzero(keep)), nlat * nlon)]
    e = out['eofs']['left']
    assert list(e.dims) == ['lag', 'lat', 'lon', 'mode'] and e.values.shape == (M, nlat, nlon, k)
    assert np.array_equal(np.asarray(e.coords['lag']), np.arange(M) * tau)
    assert np.array_equal(np.asarray(e.coords['lat']), lat) and np.array_equal(np.asarray(e.coords['lon']), lon)
    assert list(np.asarray(e.coords['mode'])) == [1, 2]
    assert np.isnan(e.values[:, 1, 2, :]).all() and np.isnan(e.values).sum() == M * k
    p = out['pcs']
    assert list(p.dims) == ['time', 'mode'] and p.values.shape == (Tp, k)
    assert np.array_equal(np.asarray(p.coords['time']), time[:Tp])
    assert isinstance(out['singular_values'], np.ndarray) and out['singular_values'].shape == (k,)
    assert isinstance(out['explained_variance'], np.ndarray) and out['explained_variance'].shape == (k,)
    ref = C.svd_truth(rec.X, M, tau, k)
    assert np.allclose(out['singular_values'], ref['singular_values'], rtol=1e-12)
    assert np.allclose(out['explained_variance'], ref['explained_variance'], rtol=1e-12)
    assert np.all(np.diff(out['explained_variance']) < 0) and 0 < out['explained_variance'].sum() <= 100.0
