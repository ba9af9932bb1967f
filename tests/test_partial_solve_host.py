"""`MCA.solve(n_modes=k)` without a device: the argument rules, the unchanged signature, the planted inputs of
tests/test_gpu_partial_solve.py (their gaps keep the guard of the partial eigenvector stage from extending the set) and the
guard's constants as the sources state them."""
import inspect
import os
import re

import numpy as np
import pytest

from partial_solve_cases import (GUARD_RELGAP, JACOBI_CASE, ONE_FIELD_CASES, TWO_FIELD_CASE, TWO_FIELD_CPLX_CASE, case_seed,
                                 gram_spectrum, planted_fields)
from xmca_amd.array import MCA
from xmca_amd.xarray import xMCA

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoDevice:
    """a handle that fails the test when solve() reaches it"""

    def __getattr__(self, name):
        raise AssertionError("device touched: " + name)


@pytest.mark.parametrize("bad", [0, -1, 2.5, True, "3", np.float64(4.0)])
def test_bad_n_modes_raises_before_any_device_work(bad):
    m = MCA(np.random.default_rng(0).standard_normal((12, 30)), handle=_NoDevice(), preprocess="host")
    with pytest.raises(ValueError, match="n_modes"):
        m.solve(n_modes=bad)
    with pytest.raises(ValueError, match="n_modes"):
        m.solve(complexify=True, extend="theta", period=4, n_modes=bad)


def test_signature_keeps_its_defaults_and_the_facade_inherits_it():
    p = inspect.signature(MCA.solve).parameters
    assert list(p) == ["self", "complexify", "extend", "period", "n_modes"]
    assert [p[k].default for k in list(p)[1:]] == [False, False, 1, None]
    assert xMCA.solve is MCA.solve


@pytest.mark.parametrize("case", ONE_FIELD_CASES + [TWO_FIELD_CASE, TWO_FIELD_CPLX_CASE, JACOBI_CASE], ids=lambda c: c[0])
def test_planted_inputs_have_the_gaps_the_route_tests_rely_on(case):
    """relative gaps of about 0.36 in sigma^2 behind each of the k leading modes, on the float64 Gram spectrum: the guard
    (relative gap above 1e-3, and eps ||T|| / gap below (3/4) 0.3^2) has no reason to extend the set, n_eigvec == k"""
    name, T, Ns, cplx, dtype, ks = case
    for k in ks:
        for X in planted_fields(T, Ns, k, case_seed(name, k), dtype):
            lam = gram_spectrum(X, cplx)
            gaps = (lam[:k] - lam[1:k + 1]) / lam[:k]
            # (the Hilbert transforms of the planted series are orthogonal to 1 / sqrt(T) only: the analytic spectrum moves a little)
            lo, hi = (0.2, 0.5) if cplx else (0.3, 0.42)
            assert np.all(gaps > lo) and np.all(gaps < hi), (name, k, gaps.min(), gaps.max())
            assert gaps[k - 1] > 100 * GUARD_RELGAP
            assert 2.220446049250313e-16 * lam[0] <= 0.75 * 0.3 ** 2 * (lam[k - 1] - lam[k])


def test_tied_pair_lies_below_the_guards_relative_gap():
    k = 10
    X = planted_fields(800, (1000,), k, case_seed("t800", k), tie=(k - 1, 1e-9))[0]
    lam = gram_spectrum(X)
    # (the noise splits the planted tie: a relative gap of about 2e-5 in sigma^2 is left)
    assert (lam[k - 1] - lam[k]) / lam[k - 1] < GUARD_RELGAP / 10
    assert (lam[k] - lam[k + 1]) / lam[k] > 0.3              # ... and the set of k + 1 is clear of the rest


def test_guard_constants_are_the_ones_the_tests_assume():
    src = open(os.path.join(REPO, "xmca_amd", "csrc", "jacobi.h")).read()
    assert float(re.search(r"TRD_PARTIAL_RELGAP = ([0-9.e+-]+);", src).group(1)) == GUARD_RELGAP
    assert re.search(r"TRD_PARTIAL_LEAK = 0\.75 \* 0\.3 \* 0\.3;", src)
    assert int(re.search(r"TRD_PARTIAL_CAP = (\d+);", src).group(1)) == 32
