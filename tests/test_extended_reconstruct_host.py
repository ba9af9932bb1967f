"""CPU: `extended_reconstruct` without a device - the argument rules on a handle stub that fails on any device
call, the identity behind the device route (diag(1 / c) A~ P from the eigenvectors of the doubly centred lag sum against the
diagonal averaging of the truncated SVD; tests/extended_reconstruct_cases.py), completeness with all modes, the two deliberate
mistakes, the conditions the cases need, the three ABI entries, and the facade on a recorder."""
import inspect
import os
import sys

import numpy as np
import pytest

import extended_eofs_cases as E
import extended_reconstruct_cases as C
from abi_cases import check_entry, header_abi_version
from xmca_amd import _hip
from xmca_amd.array import MCA

try:
    import xarray as xr                      # the real package, where it exists
except Exception:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
    import xarray as xr

from xmca_amd.xarray import xMCA

NEW = {"xmca_extended_reconstruct": 14, "xmca_lag_expand": 9, "xmca_lag_window_means": 4}
BOUND = 1e-12                 # x max|X|: route against truth, and completeness (measured: <= 1e-14)


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
        m.extended_reconstruct(bad)
    with pytest.raises(ValueError, match="tau"):
        m.extended_reconstruct(2, tau=bad)


@pytest.mark.parametrize("M,tau", [(12, 1), (13, 1), (4, 4), (2, 11), (100, 100)])
def test_a_window_of_fewer_than_two_steps_is_refused(M, tau):
    with pytest.raises(ValueError, match="at least 2"):
        _model(T=12).extended_reconstruct(M, tau=tau, mode=1)


@pytest.mark.parametrize("M,tau", [(2, 7), (2, 9), (3, 5)])
def test_a_shift_that_leaves_time_steps_in_no_window_is_refused(M, tau):
    """T = 12: T' = 5, 3, 2 - at least 2, but below tau"""
    assert 2 <= 12 - (M - 1) * tau < tau
    with pytest.raises(ValueError, match="no window"):
        _model(T=12).extended_reconstruct(M, tau=tau, mode=1)


def test_abutting_windows_pass_the_argument_rules():
    """tau = T' is the last accepted shift: the call gets as far as the device"""
    with pytest.raises(AssertionError, match="device touched"):
        _model(T=12).extended_reconstruct(2, tau=6, mode=1)


@pytest.mark.parametrize("bad", [1.0, "2", True, [1, 2], (1, 2), np.float32(2)])
def test_a_mode_of_the_wrong_type_is_refused(bad):
    with pytest.raises(ValueError, match="mode"):
        _model().extended_reconstruct(2, mode=bad)


@pytest.mark.parametrize("bad", [0, -2, slice(3, 2), slice(0, 2), slice(5, 5, -1)])
def test_an_empty_selection_is_refused(bad):
    with pytest.raises(ValueError, match="mode"):
        _model().extended_reconstruct(2, mode=bad)


def test_a_selection_past_the_rank_of_the_centred_embedded_matrix_is_refused():
    # T' - 1 binds: T = 12, M = 3, tau = 2 -> T' = 8, M N = 21: modes 1..7
    for bad in (8, slice(7, 8), slice(8, None)):
        with pytest.raises(ValueError, match="mode"):
            _model(T=12, N=7).extended_reconstruct(3, tau=2, mode=bad)
    # M N binds: T = 12, N = 2, M = 2 -> T' = 11, M N = 4
    with pytest.raises(ValueError, match="mode"):
        _model(T=12, N=2).extended_reconstruct(2, mode=5)
    # ... and the largest selections get as far as the device
    for good in (7, slice(7, 7), None):
        with pytest.raises(AssertionError, match="device touched"):
            _model(T=12, N=7).extended_reconstruct(3, tau=2, mode=good)


def test_two_fields_and_complex_models_are_refused():
    with pytest.raises(ValueError, match="one field"):
        _model(two=True).extended_reconstruct(2, mode=1)
    m = _model()
    m._analysis['is_complex'] = True
    with pytest.raises(ValueError, match="complex"):
        m.extended_reconstruct(2, mode=1)


def test_a_subclass_that_scales_on_its_own_must_say_how():
    """the finish runs on the device: a `_scale_X_inverse` the device cannot see is refused, not silently left out"""
    class Scaled(MCA):
        def _scale_X_inverse(self, data_dict):
            return data_dict

    rng = np.random.default_rng(5)
    m = Scaled(rng.standard_normal((12, 7)), handle=_NoDevice(), preprocess="host")
    with pytest.raises(ValueError, match="_device_column_weights"):
        m.extended_reconstruct(2, mode=1)
    with pytest.raises(AssertionError, match="device touched"):
        m.extended_reconstruct(2, mode=1, original_scale=False)


def test_signature():
    p = inspect.signature(MCA.extended_reconstruct).parameters
    assert list(p) == ["self", "embedding", "tau", "mode", "original_scale"]
    assert [p[k].default for k in list(p)[2:]] == [1, None, True]
    assert list(inspect.signature(xMCA.extended_reconstruct).parameters) == list(p)


def test_mode_indices_follow_reconstructed_fields():
    assert list(C.mode_indices(None, 4)) == [0, 1, 2, 3] and list(C.mode_indices(3, 9)) == [0, 1, 2]
    assert list(C.mode_indices(slice(2, 3), 9)) == [1, 2] and list(C.mode_indices(slice(2, None), 4)) == [1, 2, 3]


# ---- the identity -------------------------------------------------------------------------------------------------------
def _group_cases():
    out = [(name, E.case_field(T, N, seed), M, tau) for name, T, N, M, tau, seed in C.GROUP_CASES + [C.LARGE_CASE]]
    name, T, shape, masked, M, tau, k, seed = C.MASKED_CASE
    out.append((name, E.masked_field(T, shape, masked, seed)[1], M, tau))
    return out


GROUPS = _group_cases()
COMPLETE = [("%dx%d_M%d_t%d" % c, C.full_field(c[0], c[1], 0), c[2], c[3]) for c in C.COMPLETE_CASES]


@pytest.mark.parametrize("case", GROUPS, ids=lambda c: c[0])
def test_every_mode_group_case_has_the_gap_the_comparison_needs(case):
    _, X, M, tau = case
    gaps = E.relgaps(E.svd_truth(X, M, tau, 3)["lam"], 3)
    assert gaps.min() >= E.MIN_RELGAP, gaps


@pytest.mark.parametrize("case", COMPLETE, ids=lambda c: c[0])
def test_every_completeness_case_has_full_numerical_rank(case):
    _, X, M, tau = case
    assert C.tail_ratio(X, M, tau) >= C.MIN_TAIL_RATIO


def test_the_geometric_spectrum_is_no_completeness_case():
    """why the completeness cases have inputs of their own: the 0.8^i spectrum of `case_field` leaves the trailing eigenvectors
    of the Gram route undetermined"""
    name, T, N, M, tau, seed = C.LARGE_CASE
    assert C.tail_ratio(E.case_field(T, N, seed), M, tau) < 1e-30


@pytest.mark.parametrize("means", [False, True], ids=["R", "R+m"])
@pytest.mark.parametrize("case", GROUPS, ids=lambda c: c[0])
def test_route_is_the_diagonal_average_of_the_truncated_svd(case, means):
    _, X, M, tau = case
    worst = 0.0
    for group in C.MODE_GROUPS:
        modes = C.mode_indices(group, C.n_modes(X, M, tau))
        worst = max(worst, np.abs(C.route(X, M, tau, modes, means=means) - C.truth(X, M, tau, modes, means=means)).max())
    print(case[0], "worst |route - truth| / max|X| = %.3g" % (worst / np.abs(X).max()))
    assert worst <= BOUND * np.abs(X).max()


@pytest.mark.parametrize("case", GROUPS[:5], ids=lambda c: c[0])
def test_components_add_up(case):
    _, X, M, tau = case
    one, pair, three = (C.truth(X, M, tau, C.mode_indices(g, 30)) for g in (slice(1, 1), slice(2, 3), 3))
    assert np.abs(one + pair - three).max() <= BOUND * np.abs(X).max()


@pytest.mark.parametrize("case", COMPLETE, ids=lambda c: c[0])
def test_all_modes_with_the_window_means_give_the_field_back(case):
    _, X, M, tau = case
    modes = np.arange(C.n_modes(X, M, tau))
    scale = np.abs(X).max()
    err_route = np.abs(C.route(X, M, tau, modes) - X).max()
    err_truth = np.abs(C.truth(X, M, tau, modes, means=True) - X).max()
    print(case[0], "completeness: route %.3g, truth %.3g (x max|X|)" % (err_route / scale, err_truth / scale))
    assert err_route <= BOUND * scale and err_truth <= BOUND * scale


@pytest.mark.parametrize("case", [c for c in COMPLETE if c[2] > 1], ids=lambda c: c[0])
def test_without_the_window_means_the_field_is_missed_by_orders_of_magnitude(case):
    _, X, M, tau = case
    modes = np.arange(C.n_modes(X, M, tau))
    assert np.abs(C.route(X, M, tau, modes, means=False) - X).max() >= 1e6 * BOUND * np.abs(X).max()


@pytest.mark.parametrize("case", [c for c in COMPLETE if c[2] > 1], ids=lambda c: c[0])
def test_dividing_by_the_number_of_lags_is_wrong_by_orders_of_magnitude(case):
    """c_t < M at both ends of the record (everywhere, where the windows abut)"""
    _, X, M, tau = case
    modes = np.arange(C.n_modes(X, M, tau))
    assert np.abs(C.route(X, M, tau, modes, divide='M') - X).max() >= 1e6 * BOUND * np.abs(X).max()


def test_counts():
    assert list(C.counts(6, 3, 1)) == [1, 2, 3, 3, 2, 1]
    assert list(C.counts(8, 2, 4)) == [1] * 8
    assert list(C.counts(7, 2, 3)) == [1, 1, 1, 2, 1, 1, 1]
    assert list(C.counts(9, 2, 6)) == [1, 1, 1, 0, 0, 0, 1, 1, 1]          # tau > T': the embedding the call refuses


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_bound_and_the_abi_number_stays():
    for name, n_args in NEW.items():
        check_entry(name, n_args)
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version()


# ---- facade -------------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the handle: owns the fields, records the one device call and answers it from the numpy truth"""

    def __init__(self, X):
        self.X = X
        self.calls = []
        self.fields_owner = None

    def extended_reconstruct(self, T, N, M, tau, modes, add_means, keep_idx=None, N_full=None, mean=None, std=None, inv_weight=None,
                             alloc=None):
        self.calls.append(dict(T=T, N=N, M=M, tau=tau, modes=list(modes), add_means=add_means, keep_idx=keep_idx, N_full=N_full, mean=mean,
                               std=std, inv_weight=inv_weight, alloc=alloc))
        R = C.truth(self.X, M, tau, modes, means=add_means)
        if inv_weight is not None:
            R = R / inv_weight
        if std is not None:
            R = R * std
        if mean is not None:
            R = R + mean
        out = np.full((T, N_full), np.nan)
        out[:, slice(None) if keep_idx is None else keep_idx] = R
        return out


def _facade():
    T, nlat, nlon = 20, 3, 4
    rng = np.random.default_rng(7)
    v = rng.standard_normal((T, nlat, nlon)) + 5.0
    v[:, 1, 2] = np.nan
    time = np.arange(100, 100 + T)
    lat, lon = np.linspace(-40, 40, nlat), np.linspace(0, 30, nlon)
    return v, time, lat, lon, xr.DataArray(v, dims=['time', 'lat', 'lon'], coords={'time': time, 'lat': lat, 'lon': lon})


def test_facade_returns_the_fields_own_dims_and_coords_and_passes_the_arguments_through():
    v, time, lat, lon, da = _facade()
    T, nlat, nlon = v.shape
    M, tau = 3, 2
    xm = xMCA(da, preprocess='host')
    xm.apply_coslat()
    keep = xm._no_nan_index['left']
    rec = _Recorder(np.asarray(xm._fields['left'], dtype=np.float64))
    xm._handle_override = rec
    rec.fields_owner = xm._owner_key()
    out = xm.extended_reconstruct(M, tau=tau, mode=slice(2, 3))
    call, = rec.calls
    assert (call['T'], call['N'], call['M'], call['tau'], call['modes'], call['add_means']) == (T, int(keep.sum()), M, tau, [1, 2], True)
    assert np.array_equal(call['keep_idx'], np.flatnonzero(keep)) and call['N_full'] == nlat * nlon
    assert call['std'] is None and call['alloc'] is None
    assert np.allclose(np.asarray(call['mean']).reshape(-1), v.reshape(T, -1)[:, keep].mean(axis=0))
    weights = np.sqrt(np.cos(np.deg2rad(np.repeat(lat, nlon))))[keep]
    assert np.allclose(call['inv_weight'], weights) and call['inv_weight'].shape == (int(keep.sum()),)
    r = out['left']
    assert list(r.dims) == ['time', 'lat', 'lon'] and r.values.shape == (T, nlat, nlon) and r.values.dtype == np.float64
    assert np.array_equal(np.asarray(r.coords['time']), time)
    assert np.array_equal(np.asarray(r.coords['lat']), lat) and np.array_equal(np.asarray(r.coords['lon']), lon)
    assert np.isnan(r.values[:, 1, 2]).all() and np.isnan(r.values).sum() == T
    # all modes (apply_coslat weights by sqrt(cos + 1e-6) and the inverse divides by sqrt(cos), as in the reference: the field
    # comes back to that difference only)
    full = xm.extended_reconstruct(M, tau=tau)['left']
    assert rec.calls[-1]['modes'] == list(range(min(T - (M - 1) * tau - 1, M * int(keep.sum()))))
    assert np.nanmax(np.abs(full.values - v)) <= 1e-5 * np.nanmax(np.abs(v))
    # the units solve() sees: no means, no factors
    xm.extended_reconstruct(M, tau=tau, mode=2, original_scale=False)
    last = rec.calls[-1]
    assert last['modes'] == [0, 1] and last['add_means'] is False
    assert last['mean'] is None and last['std'] is None and last['inv_weight'] is None


def test_normalised_model_passes_its_standard_deviations():
    v, time, lat, lon, da = _facade()
    xm = xMCA(da, preprocess='host')
    xm.normalize()
    keep = xm._no_nan_index['left']
    rec = _Recorder(np.asarray(xm._fields['left'], dtype=np.float64))
    xm._handle_override = rec
    rec.fields_owner = xm._owner_key()
    full = xm.extended_reconstruct(2, tau=3)['left']
    call, = rec.calls
    assert call['inv_weight'] is None
    assert np.allclose(np.asarray(call['std']).reshape(-1), v.reshape(v.shape[0], -1)[:, keep].std(axis=0))
    assert np.nanmax(np.abs(full.values - v)) <= 1e-12 * np.nanmax(np.abs(v))
