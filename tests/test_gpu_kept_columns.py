"""GPU: the kept-column seam shared by the masked outputs - `Handle.maps` (EOFs, no scaling), `Handle.correlation_maps`,
`Handle.reconstruct` and `Handle.extended_eofs`.  The C ABI checks `keep_idx` / `N_full` and uploads the inverse map in one place
for all of them, so each output is called without a mask and with three masks on the same resident real float64 field and solve:

  * the kept rows (columns) of the masked output are the unmasked output to the bit - both come from the same kernels, the mask
    only scatters - and every other row (column) is NaN;
  * a decreasing pair, a repeated index, an index equal to N_full and N_full = N - 1 are refused with ERR_INVALID (ValueError)
    before any stage of the device runs, and the handle answers a valid call afterwards.

T = 12, N = 5, three modes, embedding = 2 with tau = 1, N_full = 7."""
import numpy as np
import pytest

from xmca_amd import _hip

pytestmark = pytest.mark.gpu

T, N, N_FULL, MODES, EMBEDDING, TAU = 12, 5, 7, 3, 2, 1
MASKS = {"first_two_dropped": [2, 3, 4, 5, 6], "last_two_dropped": [0, 1, 2, 3, 4], "alternating_ends": [0, 2, 3, 4, 6]}
REFUSED = {"decreasing_pair": ([0, 3, 2, 4, 6], N_FULL), "repeated_index": ([0, 2, 2, 4, 6], N_FULL),
           "index_equal_to_N_full": ([0, 2, 3, 4, 7], N_FULL), "N_full_below_N": (None, N - 1)}


def _maps(hip, keep_idx, n_full):
    return (hip.maps(0, N, MODES, None, None, keep_idx, n_full, _hip.MAP_EOF, _hip.SCALE_NONE, np.float64),)


def _correlation_maps(hip, keep_idx, n_full):
    Y = np.random.default_rng(12).standard_normal((T, MODES))
    return hip.correlation_maps(0, Y, keep_idx, n_full, np.float64)


def _reconstruct(hip, keep_idx, n_full):
    B = np.random.default_rng(13).standard_normal((T, MODES))
    return (hip.reconstruct(0, B, None, N, keep_idx=keep_idx, N_full=n_full),)


def _extended_eofs(hip, keep_idx, n_full):
    return (hip.extended_eofs(T, N, EMBEDDING, TAU, MODES, keep_idx, n_full)[2],)


# entry -> (call returning the masked arrays, their masked axis)
ENTRIES = {"maps": (_maps, 0), "correlation_maps": (_correlation_maps, 0), "reconstruct": (_reconstruct, 1),
           "extended_eofs": (_extended_eofs, 1)}


@pytest.fixture
def solved(hip):
    """The handle with the T x N field resident and solved"""
    X = np.random.default_rng(11).standard_normal((T, N))
    hip.set_field(0, X - X.mean(axis=0))
    assert hip.solve(1) >= MODES
    return hip


@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_masked_output_is_the_unmasked_one_scattered(solved, entry, mask):
    call, axis = ENTRIES[entry]
    keep = np.array(MASKS[mask])
    dropped = np.setdiff1d(np.arange(N_FULL), keep)
    plain = call(solved, None, N)
    masked = call(solved, keep, N_FULL)
    assert len(plain) == len(masked)
    for a, b in zip(plain, masked):
        assert a.shape[axis] == N and b.shape[axis] == N_FULL and np.isfinite(a).all()
        assert np.array_equal(np.take(b, keep, axis=axis), a)
        assert np.isnan(np.take(b, dropped, axis=axis)).all()


@pytest.mark.parametrize("case", sorted(REFUSED))
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_bad_kept_columns_are_refused_before_the_device_runs(solved, entry, case):
    call, _ = ENTRIES[entry]
    keep, n_full = REFUSED[case]
    valid = np.array(MASKS["alternating_ends"])
    before = _maps(solved, valid, N_FULL)[0]
    stages = solved.timings()
    with pytest.raises(ValueError):
        call(solved, None if keep is None else np.array(keep), n_full)
    assert solved.timings() == stages                   # (no stage of the device was entered)
    assert np.array_equal(_maps(solved, valid, N_FULL)[0], before, equal_nan=True)
