"""CPU: `xmca_amd.gaps.fill_gaps(embedding=, tau=)` without a device (M-SSA gap filling) - the numpy restatement
the GPU tests compare with (tests/lagged_fill_gaps_cases.py: its two float64 routes agree, at M = 1 it is the DINEOF restatement,
two planted mistakes are told from it, it bridges wholly missing time steps where DINEOF cannot), every new argument rule on a
handle stub that fails on any device call, the two ABI entries, and the facade over tests/fake_xarray."""
import inspect
import os
import sys

import numpy as np
import pytest

import fill_gaps_cases as D
import lagged_fill_gaps_cases as C
from abi_cases import check_entry, header_abi_version, header_text
from xmca_amd import _hip, gaps

try:
    import xarray as xr                      # the real package, where it exists
except Exception:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
    import xarray as xr

from xmca_amd import xarray as facade

NEW = {"xmca_fill_gaps_lagged": 17, "xmca_gap_lag_fill_step": 13}
ALL_CASES = C.CASES + [C.LARGE_CASE, C.EDGE_CASE]


class _NoDevice:
    """a handle that fails the test when anything reaches it"""

    def __getattr__(self, name):
        raise AssertionError("device touched: " + name)


def _field(T=24, N=7, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, N))
    X[rng.random((T, N)) < 0.2] = np.nan
    X[0, :] = 1.0                     # (every column keeps a value)
    return X


def _fill(X, n_modes=2, **kw):
    return gaps.fill_gaps(X, n_modes, handle=_NoDevice(), **kw)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=C.case_name)
def test_the_two_routes_of_the_restatement_agree(case):
    a, b = C.reference(case, route="gram"), C.reference(case, route="svd")
    bound = 1e-12 * float(np.nanmax(np.abs(C.case_field(case)[0])))
    print("delta %.3e (bound %.3e)" % (np.max(np.abs(a["field"] - b["field"])), bound))
    assert np.max(np.abs(a["field"] - b["field"])) <= bound
    assert np.max(np.abs(a["history"] - b["history"])) <= bound
    assert np.max(np.abs(a["lam"] / b["lam"] - 1)) <= 1e-10
    assert len(a["history"]) == C.iterations_of(case)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
@pytest.mark.parametrize("route", ["gram", "svd"])
def test_one_window_is_the_dineof_restatement(case, route):
    T, N, k, M, tau, frac, dead = case
    X = C.case_field(case)[0]
    a = C.mssa_fill(X, k, 1, 1, 10, 0.0, route=route)
    b = D.dineof(X, k, 10, 0.0, route=route)
    bound = 1e-13 * float(np.nanmax(np.abs(X)))
    assert np.max(np.abs(a["field"] - b["field"])) <= bound and np.max(np.abs(a["history"] - b["history"])) <= bound
    assert np.max(np.abs(a["lam"] / b["lam"] - 1)) <= 1e-12


@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
@pytest.mark.parametrize("mistake", ["by_M", "no_shift"])
def test_a_planted_mistake_is_told_from_the_other_route(case, mistake):
    """dividing by M instead of c_t, and dropping the shift t - j tau: both miss the svd route by at least 1e6 delta"""
    wrong = C.reference(case, mistake=mistake)["field"]
    miss = float(np.max(np.abs(wrong - C.reference(case, route="svd")["field"])))
    print("miss %.3e, delta %.3e" % (miss, C.route_delta(case)))
    assert miss >= 1e6 * C.route_delta(case)


def test_averaged_counts_the_windows_that_hold_a_time_step():
    for T, M, tau in ((10, 3, 2), (10, 1, 1), (80, 2, 40), (150, 24, 3), (7, 3, 1)):
        Tp, count = C.windows(T, M, tau)
        brute = np.array([sum(1 for j in range(M) if 0 <= t - j * tau < Tp) for t in range(T)])
        assert Tp == T - (M - 1) * tau and np.array_equal(count, brute) and count.min() >= 1
    Z, P = np.ones((1, 6)), np.ones((3, 4))
    assert np.array_equal(C.averaged(Z, P, 10, 3, 2), np.ones((10, 4)))          # every copy equal: the average is the copy


@pytest.mark.parametrize("case", C.DEAD_CASES, ids=C.case_name)
def test_the_restatement_bridges_dead_time_steps_and_dineof_cannot(case):
    X, truth, rows = C.case_field(case)
    assert rows.size == case[6] and np.isnan(X[rows]).all()
    lagged = C.dead_step_ratio(C.reference(case)["field"], X, truth, rows)
    plain = C.dead_step_ratio(C.reference(case, embedded=False)["field"], X, truth, rows)
    print("dead steps: M-SSA %.3f, DINEOF %.3f of the column-mean fill" % (lagged, plain))
    assert lagged <= C.DEAD_RATIO
    assert plain >= C.DINEOF_DEAD_RATIO


def test_the_cross_validation_curve_has_wide_gaps_and_chooses_the_largest_candidate():
    curve = [C.reference(C.CV_CASE, cv=True, k=k)["cv_rms"] for k in C.CV_CANDIDATES]
    print("cv curve", curve)
    assert curve[0] > 1.2 * curve[1] > 1.2 * 1.2 * curve[2]


def test_the_convergence_case_converges_well_inside_the_limit():
    T, N, k, M, tau, frac, dead = C.CONVERGENCE_CASE
    out = C.mssa_fill(C.case_field(C.CONVERGENCE_CASE)[0], k, M, tau, 300, C.CONVERGENCE_TOL)
    print("iterations", out["iterations"], out["history"][-2:])
    assert out["converged"] and 10 < out["iterations"] < 100
    # the step is clear of the threshold on both sides, so that rounding cannot move it
    assert out["history"][-1] < 0.9 * C.CONVERGENCE_TOL and out["history"][-2] > 1.1 * C.CONVERGENCE_TOL


def test_every_case_is_what_its_note_says():
    for case in ALL_CASES + [C.CONVERGENCE_CASE]:
        T, N, k, M, tau, frac, dead = case
        X = C.case_field(case)[0]
        Tp = T - (M - 1) * tau
        assert np.isfinite(X).any(axis=0).all() and np.isnan(X).any() and Tp >= 2 and tau <= Tp and 1 <= k <= min(Tp, M * N) - 1
    assert C.LARGE_CASE[0] - (C.LARGE_CASE[3] - 1) * C.LARGE_CASE[4] >= 768
    T, N, k, M, tau, frac, dead = C.EDGE_CASE
    assert T - (M - 1) * tau < 768 <= T
    T, N, k, M, tau, frac, dead = C.CASES[5]
    assert (M - 1) * tau > C.TILE_ROWS
    T, N, k, M, tau, frac, dead = C.CASES[6]
    assert tau == T - (M - 1) * tau and C.windows(T, M, tau)[1].max() == 1


# ---- argument rules -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["embedding", "tau"])
@pytest.mark.parametrize("bad", [0, -1, 2.0, "2", None, True])
def test_bad_embedding_and_tau_raise_before_any_device_work(name, bad):
    kw = {"embedding": 2, "tau": 1}
    kw[name] = bad
    with pytest.raises(ValueError, match=name):
        _fill(_field(), **kw)


def test_too_few_windows_raise():
    with pytest.raises(ValueError, match="T'"):
        _fill(_field(T=24), embedding=24, tau=1)          # T' = 1
    with pytest.raises(ValueError, match="T'"):
        _fill(_field(T=24), embedding=5, tau=6)           # T' = 0
    with pytest.raises(ValueError, match="T'"):
        _fill(_field(T=24), embedding=30, tau=2)          # T' < 0


def test_a_stride_above_the_windows_raises():
    with pytest.raises(ValueError, match="outside every window"):
        _fill(_field(T=24), embedding=2, tau=13)          # T' = 11 < tau: the steps 11 and 12 lie in no window
    with pytest.raises(AssertionError, match="device touched: fill_gaps_lagged"):
        _fill(_field(T=24), embedding=2, tau=12)          # tau = T' is allowed


def test_n_modes_is_bounded_by_the_windows_and_the_embedded_columns():
    X = _field(T=24, N=7)
    with pytest.raises(ValueError, match="n_modes"):
        _fill(X, 5, embedding=20, tau=1)                   # T' = 5: n_modes <= 4
    with pytest.raises(AssertionError, match="device touched: fill_gaps_lagged"):
        _fill(X, 4, embedding=20, tau=1)
    Y = _field(T=24, N=2)
    with pytest.raises(ValueError, match="n_modes"):
        _fill(Y, 4, embedding=2, tau=1)                    # M N = 4: n_modes <= 3
    with pytest.raises(AssertionError, match="device touched: fill_gaps_lagged"):
        _fill(Y, 3, embedding=2, tau=1)                    # ... above min(T, N) - 1 = 1, the rule of one window
    with pytest.raises(ValueError, match="n_modes"):
        _fill(Y, 3)
    with pytest.raises(ValueError, match="n_modes"):
        _fill(X, (1, 5), embedding=20, tau=1, cv_fraction=0.1)


def test_the_old_rules_hold_with_an_embedding():
    X = _field()
    with pytest.raises(ValueError, match="max_iter"):
        _fill(X, embedding=3, max_iter=0)
    with pytest.raises(ValueError, match="tol"):
        _fill(X, embedding=3, tol=-1.0)
    with pytest.raises(ValueError, match="cross-validation"):
        _fill(X, (1, 2), embedding=3)
    with pytest.raises(ValueError, match="float"):
        _fill(X.astype(np.complex128), embedding=3)
    bad = X.copy()
    bad[3, 2] = np.inf
    with pytest.raises(ValueError, match="Inf"):
        _fill(bad, embedding=3)


def test_one_window_takes_the_old_entry_and_more_take_the_new_one():
    with pytest.raises(AssertionError, match=r"device touched: fill_gaps$"):
        _fill(_field(), 2, embedding=1, tau=5)             # (tau means nothing with one window)
    with pytest.raises(AssertionError, match=r"device touched: fill_gaps_lagged$"):
        _fill(_field(), 2, embedding=3, tau=2, cv_fraction=0.1, seed=1)


def test_the_new_arguments_come_last_with_defaults_of_one():
    names = list(inspect.signature(gaps.fill_gaps).parameters)
    assert names[-2:] == ["embedding", "tau"] and names[:8] == ["X", "n_modes", "max_iter", "tol", "cv_fraction", "cv_idx", "seed", "handle"]
    for name in ("embedding", "tau"):
        assert inspect.signature(gaps.fill_gaps).parameters[name].default == 1


# ---- ABI and facade -------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entries_and_the_binding_has_them():
    for name, n_args in NEW.items():
        check_entry(name, n_args)
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version()
    assert '"gap_lag_gram"' in header_text(comments=True)                 # (the stage name stands in a comment)
    for method in ("fill_gaps_lagged", "gap_lag_fill_step"):
        assert callable(getattr(_hip.Handle, method))
    from abi_cases import header_arguments
    old, new = header_arguments("xmca_fill_gaps"), header_arguments("xmca_fill_gaps_lagged")
    assert [a for a in new if a not in ("int embedding", "int tau")] == old and len(old) == 15


def test_the_facade_passes_the_embedding_through():
    a = inspect.signature(gaps.fill_gaps).parameters
    b = inspect.signature(facade.fill_gaps).parameters
    assert list(a)[1:] == list(b)[1:] and all(a[n].default == b[n].default for n in ("embedding", "tau"))
    da = xr.DataArray(_field(T=24, N=6).reshape(24, 2, 3), dims=["time", "lat", "lon"],
                      coords={"time": np.arange(24), "lat": [0.0, 1.0], "lon": [0.0, 1.0, 2.0]})
    with pytest.raises(ValueError, match="outside every window"):
        facade.fill_gaps(da, 2, handle=_NoDevice(), embedding=2, tau=13)
    with pytest.raises(ValueError, match="embedding"):
        facade.fill_gaps(da, 2, handle=_NoDevice(), embedding=0)
    with pytest.raises(AssertionError, match="device touched: fill_gaps_lagged"):
        facade.fill_gaps(da, 2, handle=_NoDevice(), embedding=3, tau=2)
    with pytest.raises(AssertionError, match=r"device touched: fill_gaps$"):
        facade.fill_gaps(da, 2, handle=_NoDevice())


class _Recorder:
    """a handle that records the call of the lagged entry and answers with the plane's column means"""

    def __init__(self):
        self.calls = []

    def fill_gaps_lagged(self, plane, k, M, tau, max_iter, tol, cv_idx=None):
        self.calls.append((plane.shape, k, M, tau, max_iter, tol, None if cv_idx is None else len(cv_idx)))
        filled = np.where(np.isfinite(plane), plane, np.nanmean(plane, axis=0))
        return filled, np.array([0.5, 0.25]), (None if cv_idx is None else 0.125 * k), np.arange(k, 0, -1.0)


def test_the_result_names_the_embedding_and_scales_the_eigenvalues_by_the_windows():
    X = _field(T=24, N=7)
    X[:, 2] = np.nan
    h = _Recorder()
    out = gaps.fill_gaps(X, 3, max_iter=9, tol=0.0, handle=h, embedding=4, tau=2)
    assert h.calls == [((24, 6), 3, 4, 2, 9, 0.0, None)]
    assert out["embedding"] == 4 and out["tau"] == 2 and out["n_modes"] == 3 and out["iterations"] == 2
    assert np.array_equal(out["singular_values"], np.array([3.0, 2.0, 1.0]) / (24 - 3 * 2 - 1))
    assert np.isnan(out["field"][:, 2]).all() and np.isfinite(np.delete(out["field"], 2, axis=1)).all()
    h = _Recorder()
    out = gaps.fill_gaps(X, (1, 2), max_iter=9, tol=0.0, handle=h, embedding=4, tau=2, cv_fraction=0.1, seed=0)
    assert [c[1] for c in h.calls] == [1, 2, 1] and h.calls[-1][-1] is None and out["n_modes"] == 1 and out["cv_curve"] == {1: 0.125, 2: 0.25}
    da = xr.DataArray(X, dims=["time", "x"], coords={"time": np.arange(24), "x": np.arange(7)})
    out = facade.fill_gaps(da, 3, handle=_Recorder(), embedding=4, tau=2)
    assert out["embedding"] == 4 and out["tau"] == 2 and isinstance(out["field"], xr.DataArray)
