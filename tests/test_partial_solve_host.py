"""`MCA.solve(n_modes=k)` without a device: the argument rules, the unchanged signature, the planted inputs of
tests/test_gpu_partial_solve.py (their gaps keep the guard of the partial eigenvector stage from extending the set) and the
guard's constants as the sources state them.  The guard itself (`xmca_partial_count`: trd_partial_count and the `repeated` test
on the leading values, as hermitian_evd takes them) against the model of oracle/partial_guard.py on random spectra and at its
boundaries, and the spectra of tests/test_gpu_partial_eigh.py against the routes stated for them."""
import inspect
import os
import re

import numpy as np
import pytest

import partial_eigh_cases as E
from oracle import partial_guard as G
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


# ------------------------------------------------------------------------------------------------
# the guard of the partial stage: library against model
# ------------------------------------------------------------------------------------------------
def _both(lam, n_lead):
    from xmca_amd import _hip
    lam = np.asarray(lam, dtype=np.float64)
    kp = G.partial_count(lam, n_lead)
    return _hip.partial_count(lam, n_lead), (kp, G.repeated_leading(lam, kp))


def _random_spectrum(rng):
    """descending, n = 4 .. 400: log-uniform magnitudes over up to 30 decades, all positive / all negative / mixed, with planted
    ties (exact copies) and clusters of 1 .. 40 further values at relative spacing 1e-8 .. 1e-2"""
    n = int(rng.integers(4, 401))
    lam = 10.0 ** rng.uniform(-rng.uniform(0.5, 30.0), 0.0, n)
    sign = rng.integers(0, 3)
    if sign == 1:
        lam = -lam
    elif sign == 2:
        lam = lam * rng.choice([-1.0, 1.0], n)
    lam = np.sort(lam)[::-1]
    for _ in range(int(rng.integers(0, 4))):
        i, w = int(rng.integers(0, n - 1)), int(rng.integers(1, 41))
        rel = 10.0 ** rng.uniform(-8, -2)
        for j in range(i + 1, min(i + 1 + w, n)):
            lam[j] = lam[j - 1] - rel * abs(lam[j - 1])
        lam = np.sort(lam)[::-1]
    for _ in range(int(rng.integers(0, 3))):
        i = int(rng.integers(0, n - 1))
        lam[i + 1:i + 1 + int(rng.integers(1, 4))] = lam[i]
        lam = np.sort(lam)[::-1]
    if rng.integers(0, 8) == 0:
        lam[int(rng.integers(0, n))] = 0.0
        lam = np.sort(lam)[::-1]
    return lam


def test_guard_equals_its_model_on_random_spectra():
    rng = np.random.default_rng(20261019)
    extended = everything = repeated = 0
    for _ in range(1000):
        lam = _random_spectrum(rng)
        n = lam.size
        for n_lead in {0, 1, n - 1, n, int(rng.integers(1, n)), int(rng.integers(1, max(2, n // 4))), int(rng.integers(1, max(2, n // 8)))}:
            lib, model = _both(lam, n_lead)
            assert lib == model, (n, n_lead, lib, model, lam.tolist())
            extended += n_lead < model[0] < n
            everything += model[0] == n and 1 <= n_lead < n and 4 * n_lead <= n
            repeated += model[1]
    # (the generator reaches every outcome often: extensions inside the cap, a cap or n / 4 overrun, bit-equal leading values)
    assert extended > 200 and everything > 200 and repeated > 200, (extended, everything, repeated)


_POW2 = 2.0 ** -np.arange(16.0)                              # relative gaps of 1/2, ||A|| = 1: both rules clear behind every mode
_AT_1E3 = np.array([4000, 2000, 1000, 999, 500, 250, 120, 60, 30, 15, 7, 3, 1, .5, .25, .1])       # 1000 - 999 == 1e-3 * 1000 in doubles
_NEG_AT_1E3 = -np.array([.1, .25, .5, 1000, 1001, 2000, 4000, 8000, 1e4, 2e4, 4e4, 8e4, 1e5, 2e5, 4e5, 8e5])
_ABS_ALONE = np.r_[1.0, 0.5, 4e-15, 2e-15, -np.linspace(0.25, 0.9, 12)]                             # gap 2e-15 behind mode 3: relative 1/2, eps / gap = 0.11
_LONG = 2.0 ** -np.arange(40.0)                             # the same down to 1e-12: gaps still a hundred times eps / 0.0675
_ZERO = np.r_[3.0, 2.0, 1.0, 0.0, -np.arange(1.0, 21.0)]
_ZEROS = np.r_[3.0, 2.0, 1.0, 0.0, 0.0, -np.arange(1.0, 20.0)]


def _with(lam, i, v):
    out = np.array(lam, dtype=np.float64)
    out[i] = v
    return out


@pytest.mark.parametrize("name,lam,n_lead,want", [
    ("none wanted", _POW2, 0, (16, False)),
    ("one", _POW2, 1, (1, False)),
    ("all but one: no longer thin", _POW2, 15, (16, False)),
    ("all", _POW2, 16, (16, False)),
    ("more than all", _POW2, 17, (16, False)),
    ("4 k == n", _POW2, 4, (4, False)),
    ("4 k == n + 1", _POW2[:15], 4, (15, False)),
    ("relative gap on the threshold is not above it", _AT_1E3, 3, (4, False)),
    ("... an ulp wider", _with(_AT_1E3, 3, np.nextafter(999.0, 0.0)), 3, (3, False)),
    ("... an ulp narrower", _with(_AT_1E3, 3, np.nextafter(999.0, 1000.0)), 3, (4, False)),
    ("negative values, on the threshold: relative to |lam_k|", _NEG_AT_1E3, 4, (16, False)),           # extended to 5 > 16 / 4
    ("negative values, an ulp wider", _with(_NEG_AT_1E3, 4, np.nextafter(-1001.0, -2000.0)), 4, (4, False)),
    ("negative values, an ulp narrower", _with(_NEG_AT_1E3, 4, np.nextafter(-1001.0, 0.0)), 4, (16, False)),
    ("all negative, ||A|| from the last value", -2.0 ** np.arange(16.0), 4, (4, False)),
    ("absolute rule alone closes the cut", _ABS_ALONE, 3, (4, False)),
    ("... and leaves it open at twice the gap", _with(_ABS_ALONE, 3, 0.0), 3, (3, False)),            # eps / 4e-15 = 0.056
    ("n_lead + 32 == n - 1, clear only behind the last cut", np.r_[E.clustered(35, 2, 32)[:34], 1e-3], 2, (35, False)),
    ("n_lead + 32 == n - 1, never clear", E.clustered(35, 2, 33), 2, (35, False)),
    ("cluster as wide as the cap", E.clustered(200, 10, 32), 10, (42, False)),
    ("cluster one wider than the cap", E.clustered(200, 10, 33), 10, (200, False)),
    ("cluster ends past n / 4", E.clustered(160, 10, 31), 10, (160, False)),
    ("lam[k-1] == 0 in front of a gap", _ZERO, 4, (4, False)),
    ("lam[k-1] == lam[k] == 0: extended, and repeated", _ZEROS, 4, (5, True)),
    ("tie inside the set", np.r_[2.0, 2.0, _LONG], 5, (5, True)),
    ("tie of the neighbour with the value behind it is not looked at", np.r_[_LONG[:6], _LONG[5], _LONG[6:]], 5, (5, False)),
    ("tie at the cut: extended, and repeated", np.r_[_LONG[:6], _LONG[5], _LONG[6:]], 6, (7, True)),
    ("all vectors: a tie anywhere", np.r_[_LONG, _LONG[-1]], 11, (41, True)),
    ("the last bit of the largest value is a tie", np.r_[2.0, np.nextafter(2.0, 0.0), _LONG], 2, (2, True)),
    ("the bit above it is none", np.r_[np.nextafter(2.0, 3.0), 2.0, _LONG], 2, (2, False)),
], ids=lambda v: v if isinstance(v, str) else None)
def test_guard_at_its_boundaries(name, lam, n_lead, want):
    """hand-worked from DESIGN.md 2.10: the answer is stated, and library and model both give it"""
    lib, model = _both(lam, n_lead)
    assert lib == want and model == want, (lib, model, want)


def test_guard_rejects_an_empty_spectrum():
    from xmca_amd import _hip
    assert _hip.load_library().xmca_partial_count(None, 4, 1, None) == -1
    lam = np.ones(1)
    assert _hip.load_library().xmca_partial_count(lam.ctypes.data, 0, 1, None) == -1
    assert _hip.partial_count([5.0], 1) == (1, False)


# ------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_partial_eigh.py, on LAPACK's spectrum
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.CASES, ids=repr)
def test_gpu_cases_have_the_routes_stated_for_them(case):
    """The guard model on numpy's eigenvalues of each matrix gives the k' the GPU test expects, and no gap it looks at lies
    within a factor 10 of the threshold it is compared with (relative 1e-3 |lam|, absolute eps ||A|| / 0.0675, 2.2e-16 ||A|| of
    the `repeated` test): the device's eigenvalues differ from LAPACK's by ~n eps ||A||, far less.  A closed cut needs ONE rule
    to fail by that factor, a `repeated` verdict one pair that far below the bound.  Cases that cannot have the margin are
    declared route free - and have to be: a stated route without margin, or a free one with it, fails here."""
    lam_ref = E.reference(case)[0]
    n = lam_ref.size
    assert 130 <= n <= 1100 and 1 <= case.k < n
    lam = lam_ref
    if case.planted is not None:
        assert np.max(np.abs(case.planted - lam_ref)) < 1e-14 * np.max(np.abs(lam_ref))
        lam = case.planted
    kp = G.partial_count(lam, case.k)
    rep = G.repeated_leading(lam, kp)
    full_stage = case.tridiag is not None and case.vec_min_n is not None and (kp == n or rep)
    m = G.margin(lam, case.k, full_route=full_stage, exact_ties=case.planted is not None)
    if case.route_free:
        assert m < E.ROUTE_MARGIN, m
        return
    assert m >= E.ROUTE_MARGIN, m
    if case.vec_min_n is None:
        assert n < 768 and (case.n_eigvec, case.tridiag) == (n, 0)         # below the threshold of the route: the sweeps, whatever the gaps
        return
    assert case.n_eigvec == (n if rep else kp), (kp, rep)
    if case.tridiag is not None:
        # the sweeps follow bit-equal values - among the leading k' + 1, or anywhere when all vectors are formed
        assert case.tridiag == (0 if rep or (kp == n and G.repeated_leading(lam, n)) else 1)
