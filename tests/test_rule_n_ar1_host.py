"""CPU: the red-noise (AR(1)) option of rule_n without a device - the ABI entries, the numpy twin against the definition, the
argument errors of `MCA.rule_n(noise=, phi=)`, the forwarding of `ar1=` and the segment rule of the filter."""
import numpy as np
import pytest

import ar1_cases as A
from abi_cases import check_entry, header_abi_version
from oracle.philox_numpy import surrogate
from xmca_amd import _hip, dist
from xmca_amd.array import MCA

NEW = {"xmca_lag1_autocorrelation": 3, "xmca_rule_n_ar1": 19, "xmca_rule_n_ar1_sharded": 19, "xmca_surrogate_ar1": 9,
       "xmca_ar1_segments": 4}


def test_new_entries_are_declared_exported_and_bound_and_the_abi_number_stays():
    for name, n_args in NEW.items():
        check_entry(name, n_args)
    # the red entries take the arguments of the white ones and then the phi pair
    for white, red in [("xmca_rule_n", "xmca_rule_n_ar1"), ("xmca_rule_n_sharded", "xmca_rule_n_ar1_sharded")]:
        assert _hip.SIGNATURES[red][1][:-2] == _hip.SIGNATURES[white][1]
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version()


def test_twin_phi_zero_is_the_white_surrogate_bit_for_bit():
    e = surrogate(37 * 11, 5, 2, 1).reshape(37, 11)
    assert np.array_equal(A.ar1_filter(e, 0.0), e)
    assert np.array_equal(A.ar1_filter(e, np.zeros(11), np.float32), e.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("phi", [-0.5, 0.3, 0.9])
def test_twin_is_stationary_with_unit_variance_and_lag_one_phi(phi):
    """asymptotic standard errors of the sample lag-1 autocorrelation and the sample variance of an AR(1) series, five of each"""
    T = 20000
    x = A.ar1_filter(surrogate(T, 20240607, 0, 0).reshape(T, 1), phi)
    assert abs(A.lag1(x)[0] - phi) <= 5 * np.sqrt((1 - phi * phi) / T)
    assert abs(x.var() - 1.0) <= 5 * np.sqrt(2 * (1 + phi * phi) / ((1 - phi * phi) * T))


def test_twin_lag1_of_a_constant_column_is_zero():
    x = np.column_stack([np.full(9, 2.5), np.arange(9.0)])
    phi = A.lag1(x)
    assert phi[0] == 0.0 and np.isfinite(phi[1]) and abs(phi[1]) < 1


def _masked_model():
    """an unsolved model of two fields, 5 x 4 grid points of which three are masked on the left; 7 on the right"""
    rng = np.random.default_rng(3)
    left = rng.standard_normal((30, 5, 4))
    left[:, 0, 1] = left[:, 2, 3] = left[:, 4, 0] = np.nan
    return MCA(left, rng.standard_normal((30, 7)))


def test_argument_errors_come_before_any_device_call():
    two = _masked_model()
    one = MCA(np.random.default_rng(4).standard_normal((30, 6)))
    n_keep = 17
    bad_everywhere = [
        dict(noise='red'),                                           # unknown noise
        dict(noise='white', phi=0.5),                                # phi without the red null
        dict(noise='ar1', phi=1.0), dict(noise='ar1', phi=-1.0),     # |phi| >= 1
        dict(noise='ar1', phi=np.nan), dict(noise='ar1', phi=np.inf),
    ]
    for kw in bad_everywhere:
        for m in (one, two):
            with pytest.raises(ValueError):
                m.rule_n(3, seed=1, **kw)
    bad_two = [
        {'left': 0.5},                                               # a field is missing
        {'left': 0.5, 'right': 0.2, 'middle': 0.1},
        (0.5, None), (0.5, 0.2, 0.1),
        np.full(20, 0.5),                                            # a bare array for two fields
        {'left': np.full((5, 5), 0.5), 'right': 0.2},                # wrong shape
        {'left': np.full(n_keep + 1, 0.5), 'right': 0.2},
        {'left': 0.5, 'right': np.full(6, 0.2)},
        {'left': np.full(n_keep, np.nan), 'right': 0.2},             # NaN at kept points
        {'left': np.where(np.arange(20) == 7, 1.5, 0.5).reshape(5, 4), 'right': 0.2},     # |phi| >= 1 at a kept point
    ]
    for phi in bad_two:
        with pytest.raises(ValueError):
            two.rule_n(3, seed=1, noise='ar1', phi=phi)
    nan_at_kept = np.full((5, 4), 0.5)
    nan_at_kept[1, 1] = np.nan
    with pytest.raises(ValueError):
        two.rule_n(3, seed=1, noise='ar1', phi={'left': nan_at_kept, 'right': 0.2})
    for phi in [(0.5, 0.2), {'left': 0.5, 'right': 0.2}, np.full(7, 0.5)]:       # a phi for a right field the model lacks
        with pytest.raises(ValueError):
            one.rule_n(3, seed=1, noise='ar1', phi=phi)


def test_phi_forms_resolve_to_one_value_per_surrogate_column():
    two = _masked_model()
    keep = two._no_nan_index['left']
    assert keep.sum() == 17
    grid = np.linspace(-0.9, 0.9, 20).reshape(5, 4)
    as_returned = np.where(keep.reshape(5, 4), grid, np.nan)          # NaN at masked points, as `lag1_autocorrelation` returns it
    want = np.where(keep, grid.reshape(-1), 0.0)                      # masked columns stay white
    for form in (grid, grid.reshape(-1), as_returned, as_returned.reshape(-1), grid.reshape(-1)[keep]):
        left, right = two._phi_columns({'left': form, 'right': 0.25})
        assert left.dtype == np.float64 and np.array_equal(left, want)
        assert np.array_equal(right, np.full(7, 0.25))
    left, right = two._phi_columns(0.5)
    assert np.array_equal(left, np.where(keep, 0.5, 0.0)) and np.array_equal(right, np.full(7, 0.5))
    left, right = two._phi_columns((0.1, np.full(7, -0.2)))
    assert np.array_equal(left, np.where(keep, 0.1, 0.0)) and np.array_equal(right, np.full(7, -0.2))
    one = MCA(np.random.default_rng(4).standard_normal((30, 6)))
    for form in (0.3, np.full(6, 0.3), (0.3, None), {'left': np.full(6, 0.3)}):
        left, right = one._phi_columns(form)
        assert right is None and np.array_equal(left, np.full(6, 0.3))


def test_lag1_autocorrelation_needs_a_solved_model():
    with pytest.raises(RuntimeError, match="solve"):
        _masked_model().lag1_autocorrelation()
    with pytest.raises(RuntimeError, match="solve"):
        _masked_model().rule_n(3, seed=1, noise='ar1')               # phi=None estimates it


class _Recorder:
    """stands in for the handle: records how rule_n was called"""
    device = 0

    def __init__(self):
        self.calls = []

    def rule_n(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        n_out = args[-1]
        n = args[10] - args[9]
        return np.ones((n, n_out)), np.ones(n, dtype=np.int32)


def _solved_stand_in(handle):
    m = MCA(np.random.default_rng(5).standard_normal((12, 4)))
    m._handle_override = handle
    m._singular_values = np.arange(4.0, 0.0, -1.0)
    m._analysis['rank'] = 4
    m._get_variance = lambda *args, **kwargs: np.arange(4.0, 0.0, -1.0)
    return m


def test_the_white_call_never_sees_the_new_keyword():
    rec = _Recorder()
    m = _solved_stand_in(rec)
    for kw in (dict(), dict(noise='white'), dict(noise='white', phi=None)):
        m.rule_n(3, seed=1, **kw)
    assert len(rec.calls) == 3 and all(kwargs == {} for _, kwargs in rec.calls)
    m.rule_n(3, seed=1, noise='ar1', phi=0.25)
    (left, right) = rec.calls[-1][1]['ar1']
    assert right is None and np.array_equal(left, np.full(4, 0.25))


def test_sharded_rule_n_forwards_ar1_only_when_it_is_set():
    from test_dist_gloo import StubDevice
    args = dict(T=10, Nx=4, Ny=3, n_fields=2, complexify=False, rotated=False, p=0, power=0, tol=1e-8, seed=5, dtype=np.float64, n_out=3)
    sp, kept = dist.sharded_rule_n(StubDevice(), 6, **args)          # a device that does not know the keyword
    assert sp.shape == (6, 3) and kept.shape == (6,)
    sp, kept = dist.sharded_rule_n(StubDevice(), 6, ar1=None, **args)
    assert sp.shape == (6, 3)
    rec = _Recorder()
    pair = (np.linspace(-0.5, 0.5, 4), np.full(3, 0.1))
    dist.sharded_rule_n(rec, 6, ar1=pair, **args)
    got = rec.calls[-1][1]['ar1']
    assert got[0] is pair[0] and got[1] is pair[1]

    class Sharded(_Recorder):
        def rule_n_sharded(self, comm, *args, **kwargs):
            self.calls.append((args, kwargs))
            return None, None

    rec = Sharded()
    dist.sharded_rule_n(rec, 6, comm=object(), **args)
    assert rec.calls[-1][1] == {}
    dist.sharded_rule_n(rec, 6, comm=object(), ar1=pair, **args)
    assert rec.calls[-1][1]['ar1'][0] is pair[0]


def test_handle_checks_the_phi_pair_before_the_library_is_called():
    for ar1, n_fields in [((np.zeros(4), None), 2), ((np.zeros(4), np.zeros(3)), 1), ((np.zeros(5), np.zeros(3)), 2),
                          ((np.array([0.0, 1.0, 0.0, 0.0]), np.zeros(3)), 2), ((np.array([0.0, np.nan, 0.0, 0.0]), np.zeros(3)), 2),
                          (np.zeros(4), 1)]:
        with pytest.raises(ValueError):
            _hip._phi_pair("rule_n", ar1, 4, 3, n_fields)
    left, right = _hip._phi_pair("rule_n", ([0.5, 0, 0, -0.5], None), 4, 0, 1)
    assert right is None and left.dtype == np.float64 and left.flags.c_contiguous


@pytest.mark.parametrize("T", [1, 2, 3, 1000, 2920, 5000])
@pytest.mark.parametrize("N", [1, 64, 10000])
def test_segments_cover_the_time_axis_once(T, N):
    seg = _hip.ar1_segments(T, N)
    assert seg[0][0] == 0 and seg[-1][1] == T
    for (b0, e0), (b1, e1) in zip(seg, seg[1:]):
        assert e0 == b1
    lengths = [e - b for b, e in seg]
    assert all(n >= 1 for n in lengths) and len(set(lengths[:-1])) <= 1 and lengths[-1] <= lengths[0]
    assert seg == _hip.ar1_segments(T, N)                             # a function of the shape alone


def test_segments_split_time_where_columns_alone_leave_the_device_empty():
    assert len(_hip.ar1_segments(1000, 64)) > 1 and len(_hip.ar1_segments(5000, 20000)) > 1
    assert len(_hip.ar1_segments(16, 64)) == 1
    assert len(_hip.ar1_segments(5000, 1 << 20)) == 1                 # wide enough: no carry pass
    with pytest.raises(ValueError):
        _hip.ar1_segments(0, 5)
