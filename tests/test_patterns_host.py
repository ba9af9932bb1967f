"""CPU: the p-value entry points are declared, exported and bound with the header's argument counts; the host constant of the
p-value kernel (-ln a - ln B(a, a), xmca_pvalue_log_norm) against mpmath-derived values (tests/golden/pvalue_truth.npz)."""
import os

import numpy as np
import pytest

from abi_cases import check_entry
from golden_inputs import GOLDEN_DIR

NEW = ["xmca_pearson_pvalues", "xmca_pvalue_log_norm", "xmca_correlation_maps"]


@pytest.mark.parametrize("name", NEW)
def test_pvalue_entry_points_are_declared_exported_and_bound(name):
    check_entry(name)


def test_abi_number_covers_the_new_entry_points():
    from xmca_amd import _hip
    assert _hip.ABI_VERSION >= 13 and _hip.load_library().xmca_abi_version() == _hip.ABI_VERSION
    assert hasattr(_hip.Handle, "pearson_pvalues") and hasattr(_hip.Handle, "correlation_maps")


def test_log_normaliser_against_mpmath_values():
    from xmca_amd import _hip
    g = np.load(os.path.join(GOLDEN_DIR, "pvalue_truth.npz"))
    assert set(g["log_norm_n_obs"]) >= {3, 4, 5, 8, 60, 300, 1200, 2920, 5000}
    for n_obs, want in zip(g["log_norm_n_obs"], g["log_norm"]):
        got = _hip.pvalue_log_norm(int(n_obs))
        assert abs(got - want) <= 4 * np.spacing(abs(want)), (n_obs, got, want)
    assert _hip.pvalue_log_norm(4) == 0.0                 # a = 1: B(1, 1) = 1
    for bad in (2, 0, -1, _hip.PVALUE_MAX_OBS + 1):
        with pytest.raises(ValueError):
            _hip.pvalue_log_norm(bad)


def test_truth_fixture_is_what_the_contract_needs():
    g = np.load(os.path.join(GOLDEN_DIR, "pvalue_truth.npz"))
    assert g["r"].shape == g["p"].shape == g["n_obs"].shape and g["tail_r"].shape == g["tail_p"].shape
    assert np.all(g["p"] >= 1e-290) and np.all(g["p"] <= 1.0) and np.all(g["tail_p"] < 1e-290) and np.all(g["tail_p"] >= 0)
    assert np.all(np.abs(g["r"]) < 1) and np.all(np.abs(g["tail_r"]) < 1)
    for n_obs in (3, 4, 5, 8, 60, 300, 1200, 2920, 5000):
        assert np.sum(g["n_obs"] == n_obs) + np.sum(g["tail_n_obs"] == n_obs) == 100
        assert np.sum(g["n_obs"] == n_obs) >= 40
    # scipy - the reference's function - agrees with the truth away from its own weak spot, the deep tail
    from xmca_amd.array import _two_sided_p
    for n_obs in np.unique(g["n_obs"]):
        sel = (g["n_obs"] == n_obs) & (g["p"] >= 1e-250)
        assert np.allclose(_two_sided_p(g["r"][sel], n_obs), g["p"][sel], rtol=2e-12, atol=0)
