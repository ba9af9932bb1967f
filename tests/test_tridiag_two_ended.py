"""Host: the two-ended Sturm count of `trd_bisect_kernel` as restated in tests/tridiag_two_ended.py, against the longdouble truth of
tests/tridiag_stage_cases.py.  The restatement rounds as the one-ended one does (one multiply-add pair per row, exact power-of-two
rescales) over chains of half the length, so it is held to the same figure the one-ended restatement reaches on these cases:
below 1 eps * bnorm, on every case of the stage tests and on every input that aims at the junction.  No GPU."""
import numpy as np
import pytest

import tridiag_stage_cases as C
import tridiag_two_ended as T


@pytest.mark.parametrize("name", C.names())
def test_the_two_ended_restatement_stays_below_one_eps_on_the_stage_cases(name):
    c = C.case(name)
    idx = C.value_index(c)
    lam = T.restate_values_two_ended(c.ds, c.es, None if c.stride == 1 else idx)
    err = C.value_errors(name, lam, idx)
    print("%s: two-ended %.3f, one-ended %.3f eps bnorm" % (name, err.max(), C.restated_value_error(name)))
    assert np.all(err < 1.0), (name, float(err.max()), int(np.argmax(err)))
    assert np.all(np.diff(lam) >= 0.0), name                                    # monotone in k


@pytest.mark.parametrize("name", T.junction_names())
def test_the_two_ended_restatement_stays_below_one_eps_at_the_junction(name):
    c = T.junction_case(name)
    lam = T.restate_values_two_ended(c.ds, c.es)
    err = T.junction_errors(name, lam)
    print("%s: two-ended %.3f, one-ended %.3f eps bnorm" % (name, err.max(), T.junction_restated_error(name)))
    assert np.all(err < 1.0), (name, float(err.max()), int(np.argmax(err)))
    assert np.all(np.diff(lam) >= 0.0), name


def test_the_count_is_the_one_ended_count_where_nothing_rounds():
    """small integers: every minor is exact in both forms, so the two counts agree at every point, zeros at the junction included"""
    d = np.array([2.0, -1.0, 3.0, 0.0, 1.0, -2.0, 4.0])
    e = np.array([1.0, 2.0, 0.0, 1.0, 3.0, 1.0])
    e2 = np.maximum(e * e, C.E2_FLOOR)
    x = np.arange(-8.0, 8.5, 0.5)
    ref = np.array([np.count_nonzero(np.linalg.eigvalsh(np.diag(d) + np.diag(e, 1) + np.diag(e, -1)) < xi - 1e-9) for xi in x])
    cnt = T.two_ended_count(d, e2, x)
    on = np.array([np.min(np.abs(np.linalg.eigvalsh(np.diag(d) + np.diag(e, 1) + np.diag(e, -1)) - xi)) < 1e-9 for xi in x])
    assert np.array_equal(cnt[~on], ref[~on]), (cnt, ref)
    assert np.all(np.diff(cnt) >= 0)
    assert T.two_ended_count(np.array([-3.0]), np.zeros(0), np.array([-4.0, -2.0])).tolist() == [0, 1]      # n = 1: no backward part
