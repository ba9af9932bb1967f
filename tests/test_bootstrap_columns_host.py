"""CPU: the plumbing of `bootstrapping(axis=1)` that needs no device - the two column entry points in the header, the binding
table and the built library (added at ABI 14; the number is 15 since the kernel-test entries), and the index composition `compose_bootstrap_indices` against `block_bootstrap(axis=1)`
applied cumulatively the way the reference's loop applies it (xmca/array.py:1902-1928)."""
import re

import numpy as np
import pytest

from abi_cases import check_entry, header_abi_version
from xmca_amd.array import compose_bootstrap_indices
from xmca_amd.tools.array import block_bootstrap

NEW = ("xmca_bootstrap_runs_columns", "xmca_bootstrap_runs_columns_extended")


def test_column_entries_are_declared_bound_and_exported_at_abi_14():
    from xmca_amd import _hip
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version()
    for name, row in zip(NEW, ("xmca_bootstrap_runs", "xmca_bootstrap_runs_extended")):
        check_entry(name)
        assert _hip.SIGNATURES[name] == _hip.SIGNATURES[row]          # the same argument order as the row entries


def _host_loop(fields, n_runs, on_left, on_right, block_size, replace):
    """The resampling of the kept host loop (array.py `bootstrapping`, = xmca/array.py:1902-1928), replicate by replicate."""
    X = [f.copy() for f in fields]
    out = []
    for _ in range(n_runs):
        if on_left and not on_right:
            X[0] = block_bootstrap(X[0], axis=1, block_size=block_size, replace=replace)
        elif on_right and not on_left:
            X[1] = block_bootstrap(X[1], axis=1, block_size=block_size, replace=replace)
        elif on_left and on_right:
            n_left = X[0].shape[1]
            both = block_bootstrap(np.concatenate(X, axis=1), axis=1, block_size=block_size, replace=replace)
            X = [both[:, :n_left], both[:, n_left:]] if len(X) == 2 else [both]
        out.append([x.copy() for x in X])
    return out


# widths (Nl, Nr): divisible by 1, 2 and 5 on each side and in sum; (15, 5) and (3, 7) put the seam inside a block of 2 / 5
SHAPES = [(20, 10), (15, 5), (3, 7)]


@pytest.mark.parametrize("replace", [True, False])
@pytest.mark.parametrize("block_size", [1, 2, 5])
@pytest.mark.parametrize("sides", ["left", "right", "both"])
@pytest.mark.parametrize("seed", [0, 7])
def test_composed_indices_reproduce_the_cumulative_host_resampling(seed, sides, block_size, replace):
    on_left, on_right = sides in ("left", "both"), sides in ("right", "both")
    checked = 0
    for n_l, n_r in SHAPES:
        space = {"left": n_l, "right": n_r, "both": n_l + n_r}[sides]
        if space % block_size:
            continue
        # every entry distinct, so equal arrays mean equal indices
        fields = [np.arange(6 * n_l, dtype=np.float64).reshape(6, n_l), 1000.0 + np.arange(6 * n_r, dtype=np.float64).reshape(6, n_r)]
        np.random.seed(seed)
        want = _host_loop(fields, 3, on_left, on_right, block_size, replace)
        np.random.seed(seed)
        il, ir = compose_bootstrap_indices(3, 1, 6, [n_l, n_r], on_left, on_right, block_size, replace)
        assert (il is None) == (not on_left) and (ir is None) == (not on_right)
        concat = np.concatenate(fields, axis=1)
        for run in range(3):
            got = [fields[0] if il is None else concat[:, il[run]], fields[1] if ir is None else concat[:, ir[run]]]
            assert np.array_equal(got[0], want[run][0]) and np.array_equal(got[1], want[run][1]), (n_l, n_r, run)
        for idx, n in ((il, n_l), (ir, n_r)):
            assert idx is None or (idx.shape == (3, n) and idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < n_l + n_r)
        checked += 1
    assert checked >= 1
    if sides == "both" and block_size in (2, 5):          # the seam case took part: Nl no multiple of the block size
        assert any(n_l % block_size and not (n_l + n_r) % block_size for n_l, n_r in SHAPES)


def test_single_field_resamples_its_own_columns_for_left_and_for_both():
    x = np.arange(24, dtype=np.float64).reshape(2, 12)
    for on_right in (False, True):
        np.random.seed(3)
        want = _host_loop([x], 3, True, on_right, 3, True)
        np.random.seed(3)
        il, ir = compose_bootstrap_indices(3, 1, 2, [12], True, on_right, 3, True)
        assert ir is None
        for run in range(3):
            assert np.array_equal(x[:, il[run]], want[run][0])


def test_rows_are_composed_as_before_and_neither_side_draws_nothing():
    np.random.seed(2)
    il, ir = compose_bootstrap_indices(2, 0, 8, [5, 4], True, True, 2, True)
    np.random.seed(2)
    x = np.arange(8)
    for run in range(2):
        x = block_bootstrap(x[:, None], axis=0, block_size=2)[:, 0]
        assert np.array_equal(il[run], x) and np.array_equal(ir[run], x)
    state = np.random.get_state()[1].copy()
    assert compose_bootstrap_indices(2, 1, 8, [5, 4], False, False, 3, True) == (None, None)
    assert np.array_equal(np.random.get_state()[1], state)


def test_the_reference_errors():
    with pytest.raises(ValueError, match=re.escape("Length of data array (12) must be a multiple of block size 5")):
        compose_bootstrap_indices(2, 1, 40, [12, 9], True, False, 5, True)
    with pytest.raises(ValueError, match=re.escape("Length of data array (21) must be a multiple of block size 2")):
        compose_bootstrap_indices(2, 1, 40, [12, 9], True, True, 2, True)          # N is Nl + Nr when both sides are resampled
    with pytest.raises(ValueError, match=re.escape("Length of data array (9) must be a multiple of block size 2")):
        compose_bootstrap_indices(2, 1, 40, [12, 9], False, True, 2, True)
    with pytest.raises(ValueError, match=re.escape("No bootstrapping possible. There is no right field. Set `on_right=False`.")):
        compose_bootstrap_indices(2, 1, 40, [12], False, True, 1, True)
    with pytest.raises(ValueError, match=re.escape("2 not a valid axis. either 0 or 1.")):
        compose_bootstrap_indices(2, 2, 40, [12, 9], True, False, 1, True)


def test_errors_are_raised_by_bootstrapping_before_any_device_work():
    """The model is never solved and no device exists here: the two ValueErrors must come first."""
    from xmca_amd.array import MCA
    rng = np.random.default_rng(0)
    m = MCA(rng.standard_normal((30, 12)), rng.standard_normal((30, 9)))
    m._device = lambda: None
    m._get_min_mode = lambda n, rotated=True: 4
    m._get_X = lambda original_scale=False, real=True: {'left': rng.standard_normal((30, 12)), 'right': rng.standard_normal((30, 9))}
    with pytest.raises(ValueError, match=re.escape("Length of data array (21) must be a multiple of block size 2")):
        m.bootstrapping(2, n_modes=4, axis=1, on_left=True, on_right=True, block_size=2)
    single = MCA(rng.standard_normal((30, 12)))
    single._device = lambda: None
    single._get_min_mode = lambda n, rotated=True: 4
    single._get_X = lambda original_scale=False, real=True: {'left': rng.standard_normal((30, 12))}
    with pytest.raises(ValueError, match="There is no right field"):
        single.bootstrapping(2, n_modes=4, axis=1, on_left=False, on_right=True)
    with pytest.raises(ValueError, match=re.escape("3 not a valid axis. either 0 or 1.")):
        single.bootstrapping(2, n_modes=4, axis=3)
