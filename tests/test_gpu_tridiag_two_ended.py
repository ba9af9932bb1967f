"""GPU: `trd_bisect_kernel` counts from both ends and joins the two chains at row m = n // 2 (csrc/tridiag.h).  The inputs of
tests/tridiag_two_ended.py aim at that junction: reversed matrices, orders at which either half crosses the eight-row block, e = 0
on either side of row m, a spectrum that lies in one half, and the smallest orders.  Through `Handle.tridiag_eigenvalues`, each
held to 4 * max(r, 1) eps * bnorm of the longdouble bisection, r the error of the one-ended restatement `restate_values` on the same
input - the figure and the margin of tests/test_gpu_tridiag_stage.py."""
import numpy as np
import pytest

import tridiag_stage_cases as C
import tridiag_two_ended as T

pytestmark = pytest.mark.gpu

MARGIN = 4.0


@pytest.fixture(scope="module")
def device_values(hip):
    """name -> what the device returns for the input (descending, the caller's scale), computed once"""
    return {c.name: hip.tridiag_eigenvalues(c.d, c.e) for c in T.junction_cases()}


@pytest.mark.parametrize("name", T.junction_names())
def test_eigenvalues_at_the_junction_stay_within_four_times_the_restatement(name, device_values):
    c = T.junction_case(name)
    lam = device_values[name]
    assert lam.shape == (c.n,) and lam.dtype == np.float64 and np.all(np.isfinite(lam))
    err = T.junction_errors(name, np.asarray(lam, dtype=C.LD)[::-1] * C.LD(c.f))
    r = T.junction_restated_error(name)
    print("%s: device %.3f, restatement %.3f eps bnorm" % (name, err.max(), r))
    assert np.all(err <= MARGIN * max(r, 1.0)), (name, float(err.max()), r, int(np.argmax(err)))
    assert np.all(np.diff(lam) <= 0.0), name                                     # non-increasing


@pytest.mark.parametrize("name", ["reversed_random_n130", "half_random_n17_e_zero_below", "spectrum_in_the_lower_half"])
def test_eigenvalues_at_the_junction_repeat_their_bits_and_do_not_see_the_sign_of_e(name, hip, device_values):
    c = T.junction_case(name)
    assert np.array_equal(hip.tridiag_eigenvalues(c.d, c.e), device_values[name]), name
    assert np.array_equal(hip.tridiag_eigenvalues(c.d, -c.e), device_values[name]), name
    flip = np.where(np.arange(c.n - 1) % 3 == 0, -1.0, 1.0)
    assert np.array_equal(hip.tridiag_eigenvalues(c.d, flip * c.e), device_values[name]), name
