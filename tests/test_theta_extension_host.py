"""The Theta fore/back-cast extension without a device: the numpy restatement (tests/theta_cases.py) against closed forms, the
decomposition X_im = G0 X + B C of `_hip.theta_imag_parts` against the direct route (concatenate, scipy.signal.hilbert, trim,
remove_mean), the new entry points of the C ABI, and the argument checks of `solve`."""
import numpy as np
import pytest

import theta_cases as tc
from abi_cases import check_entry, header_abi_version
from xmca_amd import _hip
from xmca_amd.array import MCA

NEW_SYMBOLS = {"xmca_complexify_theta": 5, "xmca_theta_fit": 4, "xmca_get_field_imag": None}


def _one(f, key):
    return f[key][..., 0]


def test_linear_column_has_no_season_and_its_own_slope():
    """y = a + b t: the moving average of a line is the line, so s = 0 exactly up to rounding and b0 = b; SSE falls with alpha all
    the way (a level that lags a ramp), so alpha ends at the upper bound."""
    for m, n in ((1, 7), (4, 13), (5, 20), (12, 24)):
        t = np.arange(n, dtype=np.float64)
        y = (0.75 * t - 3.0)[:, None]
        f = tc.fit(y - y.mean(), m)
        assert np.abs(f["s"]).max() < 1e-13
        assert abs(_one(f, "b0") - 0.75) < 1e-13
        assert abs(_one(f, "alpha") - tc.ALPHA_HI) < 1e-15
        assert np.abs(np.diff(tc.forecast(f, n, m)[:, 0]) - 0.95 * 0.75).max() < 1e-12      # the forecast: a line of slope 0.95 b0


def test_periodic_pattern_over_whole_cycles_is_recovered():
    """A zero-mean pattern of period m over whole cycles: the moving average vanishes, d = y, s is the pattern; z = 0, so b0 = 0, every
    candidate ties at SSE = 0 and the lowest alpha wins."""
    rng = np.random.default_rng(3)
    for m, cycles in ((2, 2), (3, 4), (4, 2), (12, 3)):
        pat = rng.standard_normal(m)
        pat -= pat.mean()
        y = np.tile(pat, cycles)[:, None]
        f = tc.fit(y, m)
        assert np.abs(f["s"][:, 0] - pat).max() < 1e-14
        assert abs(_one(f, "b0")) < 1e-14 and abs(_one(f, "level")) < 1e-14
        n = m * cycles
        assert np.abs(tc.forecast(f, n, m)[:, 0] - y[:, 0]).max() < 1e-13          # (n + h) mod m = h mod m: the pattern goes on


def test_all_zero_column():
    for m, n in ((1, 2), (2, 4), (4, 9), (12, 25)):
        pair = tc.fits(np.zeros((n, 3)), m)
        for f in pair:
            assert np.all(f["alpha"] == tc.ALPHA_LO) and np.all(f["b0"] == 0) and np.all(f["level"] == 0) and np.all(f["s"] == 0)
            assert np.all(tc.forecast(f, n, m) == 0)
        assert np.all(tc.analytic_signal(np.zeros((n, 3)), m, pair) == 0)


def test_alpha_lands_where_the_columns_are_built_to_put_it():
    X = tc.columns(48, 12, 1, seed=11)
    a = tc.fit(X, 1)["alpha"]
    assert np.all(a[1::6] < 0.2)                      # white noise: the mean is the best level
    assert np.all(a[2::6] > 0.6)                      # a random walk: the last value is
    assert np.all(a[4::6] == tc.ALPHA_LO)             # the constant grid point
    lo_hits = np.sum(a == tc.ALPHA_LO)
    assert lo_hits >= 2 and np.sum((a > 0.01) & (a < 0.99)) >= 2


def test_requires_two_seasons():
    with pytest.raises(ValueError):
        tc.seasonal_means(np.zeros((7, 1)), 4)


@pytest.mark.parametrize("T,m", [(24, 12), (25, 4), (37, 5), (48, 1), (9, 4), (6, 3), (5, 2)])
def test_decomposition_equals_the_direct_route(T, m):
    """X_im = G0 X + B C with the parts the product uploads, against hilbert of [pre; y; post]: 1e-12 of max |X_im|."""
    X = tc.columns(T, 30, m, seed=7 * T + m)
    pair = tc.checked_fits(X, m)
    col3, hbar, B = _hip.theta_imag_parts(T, m)
    assert B.shape == (T, 2 * (2 + m)) and col3.shape == (3 * T,) and hbar.shape == (T,)
    idx = (np.arange(T)[:, None] - np.arange(T)[None, :]) % (3 * T)
    G0 = col3[idx] - hbar[None, :]
    C = np.concatenate([tc.coefficients(pair[0], T, m), tc.coefficients(pair[1], T, m)])
    ref = tc.analytic_signal(X, m, pair)
    assert np.abs(G0 @ X + B @ C - ref.imag).max() <= 1e-12 * np.abs(ref.imag).max()
    assert np.abs(ref.real - X).max() <= 1e-12 * np.abs(X).max()          # the real part: the centred field itself
    # the basis reproduces the restated forecast
    F = _hip.theta_forecast_basis(T, m)
    assert np.abs(F @ C[:2 + m] - tc.forecast(pair[0], T, m)).max() <= 1e-12 * np.abs(X).max()


def test_test_columns_meet_the_condition_on_the_inputs():
    """No first-round choice hinges on rounding: the gap to any second minimum is >= 1e-6 for every column the device tests fit."""
    for m in tc.M_VALUES:
        for T in tc.lengths(m):
            tc.checked_fits(tc.columns(T, 130, m, seed=100 * m + T), m)


def test_new_entry_points_are_declared_exported_and_bound():
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version()
    for name, n_args in NEW_SYMBOLS.items():
        check_entry(name, n_args)


@pytest.mark.parametrize("period", [0, -3, 2.0, 13, True, None, "12"])
def test_solve_refuses_a_bad_period(period):
    m = MCA(np.random.default_rng(0).standard_normal((25, 6)), preprocess="host")
    with pytest.raises(ValueError, match="period"):
        m.solve(complexify=True, extend="theta", period=period)


def test_n_modes_is_checked_before_period():
    m = MCA(np.random.default_rng(0).standard_normal((25, 6)), preprocess="host")
    with pytest.raises(ValueError, match="n_modes"):
        m.solve(complexify=True, extend="theta", period=0, n_modes=0)


def test_parts_refuse_a_bad_period():
    with pytest.raises(ValueError):
        _hip.theta_imag_parts(7, 4)
    with pytest.raises(ValueError):
        _hip.theta_imag_parts(8, 0)
