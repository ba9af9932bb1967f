"""CPU: `extended_rule_n` without a device - the argument rules on a handle stub that fails on any device call,
the identities behind the device route (Lambda_k(X) = lambda_k; the shift sum of one thin product against the explicitly embedded
surrogate; tests/extended_rule_n_cases.py), the gap condition of every case, the planted-signal case decided on the CPU, and the
ABI entries."""
import inspect
import os
import sys

import numpy as np
import pytest

import ar1_cases as A
import extended_rule_n_cases as C
from abi_cases import check_entry, header_abi_version
from xmca_amd import _hip
from xmca_amd.array import MCA

try:
    import xarray as xr                      # noqa: F401  (the real package, where it exists)
except Exception:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
    import xarray as xr                      # noqa: F401

from xmca_amd.xarray import xMCA

NEW = {"xmca_extended_rule_n": 11, "xmca_extended_project": 7, "xmca_lag_project": 7, "xmca_lag_project_tile": 2}
# the identities in float64: sums of at most M N = 900 products and T' = 119 squares, measured at 2e-15 and below
BOUND_IDENTITY = 1e-13


class _NoDevice:
    """a handle that fails the test when anything reaches it"""

    def __getattr__(self, name):
        raise AssertionError("device touched: " + name)


def _model(T=12, N=7, two=False):
    rng = np.random.default_rng(5)
    fields = [rng.standard_normal((T, N))] + ([rng.standard_normal((T, N + 1))] if two else [])
    return MCA(*fields, handle=_NoDevice(), preprocess="host")


# ---- argument rules -----------------------------------------------------------------------------------------------------
def test_signatures_of_the_class_and_the_facade_agree():
    p = inspect.signature(MCA.extended_rule_n).parameters
    assert list(p) == ["self", "embedding", "tau", "n_runs", "n_modes", "seed", "phi"]
    assert [p[k].default for k in list(p)[2:]] == [1, 100, 10, None, None]
    q = inspect.signature(xMCA.extended_rule_n).parameters
    assert list(q) == list(p) and [q[k].default for k in q] == [p[k].default for k in p]


@pytest.mark.parametrize("bad", [0, -1, 2.5, True, "3", np.float64(4.0), None])
def test_bad_embedding_and_tau_raise_before_any_device_work(bad):
    m = _model()
    with pytest.raises(ValueError, match="embedding"):
        m.extended_rule_n(bad, n_modes=1, phi=0.5)
    with pytest.raises(ValueError, match="tau"):
        m.extended_rule_n(2, tau=bad, n_modes=1, phi=0.5)


@pytest.mark.parametrize("M,tau", [(12, 1), (4, 4), (2, 11)])
def test_a_window_of_fewer_than_two_steps_is_refused(M, tau):
    with pytest.raises(ValueError, match="at least 2"):
        _model(T=12).extended_rule_n(M, tau=tau, n_modes=1)


@pytest.mark.parametrize("bad", [0, -2, 1.0, False, "2", None, 11])
def test_bad_n_modes_raise_before_any_device_work(bad):
    with pytest.raises(ValueError, match="n_modes"):
        _model().extended_rule_n(2, n_modes=bad)
    with pytest.raises(ValueError, match="n_modes"):          # the default of 10 modes is checked like a given one: T' - 1 = 7
        _model().extended_rule_n(3, tau=2)


@pytest.mark.parametrize("bad", [0, -3, 2.0, True, "5", None])
def test_bad_n_runs_raise_before_any_device_work(bad):
    with pytest.raises(ValueError, match="n_runs"):
        _model().extended_rule_n(2, n_runs=bad, n_modes=2)


def test_two_fields_and_complex_models_are_refused():
    with pytest.raises(ValueError, match="one field"):
        _model(two=True).extended_rule_n(2, n_modes=1)
    m = _model()
    m._analysis['is_complex'] = True
    with pytest.raises(ValueError, match="complex"):
        m.extended_rule_n(2, n_modes=1)


@pytest.mark.parametrize("bad", [1.0, -1.0, np.nan, np.inf, np.zeros(3), "red", {"right": 0.5}])
def test_a_bad_phi_is_refused_before_any_device_work(bad):
    with pytest.raises(ValueError, match="phi"):
        _model().extended_rule_n(2, n_modes=2, n_runs=3, seed=1, phi=bad)


def test_the_binding_refuses_bad_shapes_without_a_library_call():
    h = _hip.Handle.__new__(_hip.Handle)              # no device behind it: every check below comes first
    with pytest.raises(ValueError, match="n_modes"):
        h.extended_rule_n(12, 7, 2, 1, 11, np.zeros(7), 0, 2, 1)
    with pytest.raises(ValueError, match="phi"):
        h.extended_rule_n(12, 7, 2, 1, 2, np.zeros(6), 0, 2, 1)
    with pytest.raises(ValueError, match="run"):
        h.extended_rule_n(12, 7, 2, 1, 2, np.zeros(7), 3, 2, 1)
    with pytest.raises(ValueError, match="shape"):
        h.extended_project(12, 7, 2, 1, 2, np.zeros((12, 6)), False)
    with pytest.raises(ValueError, match="lag_project"):
        h.lag_project(np.zeros((12, 5)), 2, 1, 3)
    with pytest.raises(ValueError, match="lag_project"):
        h.lag_project(np.zeros((4, 6)), 2, 4, 3)


# ---- the identities -----------------------------------------------------------------------------------------------------
def _cases():
    out = [(name, C.separated_field(T, N, seed), M, tau, k) for name, T, N, M, tau, k, seed in C.CASES]
    name, T, shape, masked, M, tau, k, seed = C.MASKED_CASE
    out.append((name, C.masked_separated_field(T, shape, masked, seed)[1], M, tau, k))
    return out


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_every_case_has_the_gap_a_projection_on_single_vectors_needs(case):
    _, X, M, tau, k = case
    for dtype in (np.float64, np.float32):            # (the float32 tests decompose the rounded field)
        gaps = C.relgaps(C.patterns(X.astype(dtype).astype(np.float64), M, tau, k)[0], k)
        assert gaps.min() >= C.MIN_RELGAP, gaps


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_projecting_the_data_returns_its_eigenvalues(case):
    _, X, M, tau, k = case
    lam, V = C.patterns(X, M, tau, k)
    assert np.allclose(np.sum(V * V, axis=0), 1.0, atol=1e-12)
    assert np.max(np.abs(C.truth(V, X, M, tau) - lam[:k])) <= BOUND_IDENTITY * lam[0]
    assert np.max(np.abs(C.shift_sum(V, X, M, tau) - lam[:k])) <= BOUND_IDENTITY * lam[0]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_the_shift_sum_of_one_thin_product_is_the_explicit_embedding(case):
    _, X, M, tau, k = case
    T, N = X.shape
    lam, V = C.patterns(X, M, tau, k)
    d = X.std(axis=0, ddof=1)
    for run in range(2):
        R = C.red_surrogate(T, N, A.cycled_phi(N) * 0.9, C.SEED, run) * d
        ref = C.truth(V, R, M, tau)
        assert ref.min() > 0
        assert np.max(np.abs(C.shift_sum(V, R, M, tau) - ref)) <= BOUND_IDENTITY * max(lam[0], ref.max())
    # folding d into the patterns is scaling the surrogate
    Vd = V * np.tile(d, M)[:, None]
    R1 = C.red_surrogate(T, N, 0.3, C.SEED, 5)
    assert np.max(np.abs(C.shift_sum(Vd, R1, M, tau) - C.truth(V, R1 * d, M, tau))) <= BOUND_IDENTITY * lam[0]


def test_the_shift_sum_without_the_centring_is_wrong():
    """a surrogate with a mean: leaving H out must be visible, or the tests of the centring would show nothing"""
    name, T, N, M, tau, k, seed = C.CASES[1]
    lam, V = C.patterns(C.separated_field(T, N, seed), M, tau, k)
    R = C.red_surrogate(T, N, 0.9, C.SEED, 0)
    Q = C.embed(R, M, tau) @ V
    assert np.max(np.abs(np.sum(Q * Q, axis=0) - C.truth(V, R, M, tau))) > 1e-3 * C.truth(V, R, M, tau).max()


def test_the_planted_pair_stands_out_on_the_cpu_with_room_to_spare():
    """the field and the seed of the GPU test, decided here: modes 1-2 are never reached by a surrogate (the largest stays below a
    tenth of lambda), and every noise mode is exceeded by some runs and not by others, with at least 5 of 40 on either side"""
    lam, runs = C.planted_truth()
    p = C.PLANTED
    assert runs.shape == (p["n_runs"], p["k"])
    assert runs[:, :2].max() < 0.1 * lam[1]
    above = (runs[:, 2:] >= lam[2:]).sum(axis=0)
    assert np.all(above >= 5) and np.all(above <= p["n_runs"] - 5), above


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_bound_and_the_abi_number_stays():
    for name, n_args in NEW.items():
        check_entry(name, n_args)
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version()


def test_the_tile_is_a_constant_of_the_build_known_without_a_device():
    rows, cols = _hip.lag_project_tile()
    assert rows >= 8 and cols >= 8 and (rows, cols) == _hip.lag_project_tile()
