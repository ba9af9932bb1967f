"""CPU: `xmca_amd.gaps.fill_gaps` without a device - the numpy restatement the GPU tests compare with
(tests/fill_gaps_cases.py: its two float64 routes agree, its changes shrink, it recovers the removed values), every argument
rule on a handle stub that fails on any device call, the four ABI entries, and the signature of the xarray wrapper."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

import fill_gaps_cases as C
from abi_cases import check_entry, header_abi_version, header_text
from xmca_amd import _hip, gaps

try:
    import xarray as xr                      # the real package, where it exists
except Exception:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
    import xarray as xr

from xmca_amd import xarray as facade

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"xmca_fill_gaps": 15, "xmca_gap_center": 9, "xmca_gap_fill_step": 11, "xmca_gap_fill_tile": 2}
# Two float64 routes to the same truncation differ by rounding that the iteration carries along: 4e-15 to 5e-14 on the k = r cases
# after 25 iterations, 1.1e-13 on the ill-conditioned k > r case (max|X| ~ 9 to 12).  1e-11 is a hundred times the worst of them.
ROUTE_BOUND = 1e-11


class _NoDevice:
    """a handle that fails the test when anything reaches it"""

    def __getattr__(self, name):
        raise AssertionError("device touched: " + name)


def _field(T=12, N=7, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, N))
    X[rng.random((T, N)) < 0.2] = np.nan
    X[0, :] = 1.0                     # (every column keeps a value)
    return X


def _fill(X, n_modes=2, **kw):
    return gaps.fill_gaps(X, n_modes, handle=_NoDevice(), **kw)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.STATE_CASES + [C.ILL_CONDITIONED_CASE], ids=C.case_name)
def test_the_two_routes_of_the_restatement_agree(case):
    a, b = C.reference(case, route="gram"), C.reference(case, route="svd")
    assert np.max(np.abs(a["field"] - b["field"])) <= ROUTE_BOUND
    assert np.max(np.abs(a["history"] - b["history"])) <= ROUTE_BOUND
    assert np.max(np.abs(a["lam"] / b["lam"] - 1)) <= 1e-10


@pytest.mark.parametrize("case", C.STATE_CASES, ids=C.case_name)
def test_the_changes_do_not_grow_after_the_first_step(case):
    h = C.reference(case)["history"]
    assert len(h) == C.STATE_ITERATIONS and np.all(np.diff(h[1:]) <= 0), h


@pytest.mark.parametrize("case", C.MAIN_CASES, ids=C.case_name)
def test_the_restatement_recovers_the_removed_values(case):
    T, N, r, k, frac = case
    X, truth = C.case_field(T, N, r, frac)
    out = C.dineof(X, k, 300, 1e-8)
    assert C.recovery_ratio(out["field"], X, truth) <= C.RECOVERY_RATIO
    present = np.isfinite(X)
    assert np.array_equal(out["field"][present], X[present]) and np.isfinite(out["field"]).all()


def test_the_convergence_case_takes_the_pinned_number_of_steps():
    T, N, r, k, frac = C.CONVERGENCE_CASE
    out = C.dineof(C.case_field(T, N, r, frac)[0], k, 300, C.CONVERGENCE_TOL)
    assert out["converged"] and out["iterations"] == C.CONVERGENCE_ITERATIONS


def test_the_cross_validation_curve_has_a_clear_minimum():
    """the candidates test on the device pins the chosen k: the two smallest values must be more than 5 % apart"""
    T, N, r, k, frac = C.CV_CASE
    X = C.case_field(T, N, r, frac)[0]
    idx = C.cv_indices(X, C.CV_SHARE, C.CV_SEED)
    curve = sorted(C.dineof(X, kk, 60, 1e-5, cv_idx=idx)["cv_rms"] for kk in C.CV_CANDIDATES)
    assert curve[1] > 1.05 * curve[0], curve


def test_every_case_keeps_a_value_in_every_column_and_k_inside_the_rule():
    assert C.LARGE_CASE[0] >= 768 > max(c[0] for c in C.STATE_CASES)          # both eigensolver routes are among the cases
    for case in C.STATE_CASES + [C.ILL_CONDITIONED_CASE, C.LARGE_CASE]:
        T, N, r, k, frac = case
        X = C.case_field(T, N, r, frac)[0]
        assert np.isfinite(X).any(axis=0).all() and np.isnan(X).any() and 1 <= k <= min(T, N) - 1
    assert any(k > C.MODE_CHUNK for _, _, k in C.KERNEL_SHAPES) and any(k == 1 for _, _, k in C.KERNEL_SHAPES)


# ---- argument rules -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, -1, 7, 100, 2.0, "2", None, True, (), (2, 2), (3, 2), (0, 1), (1, 7), (1, 2.0)])
def test_bad_n_modes_raise_before_any_device_work(bad):
    with pytest.raises(ValueError, match="n_modes"):
        _fill(_field(T=12, N=7), bad, cv_fraction=0.1)


def test_n_modes_is_bounded_by_the_columns_that_hold_a_value():
    X = _field(T=12, N=7)
    X[:, [1, 4]] = np.nan                       # five columns left: n_modes <= 4
    with pytest.raises(ValueError, match="n_modes"):
        _fill(X, 5)
    with pytest.raises(ValueError, match="n_modes"):
        _fill(_field(T=4, N=9), 4)              # T binds


@pytest.mark.parametrize("bad", [0, -3, 2.5, "10", None, True])
def test_bad_max_iter_raises(bad):
    with pytest.raises(ValueError, match="max_iter"):
        _fill(_field(), max_iter=bad)


@pytest.mark.parametrize("bad", [-1e-9, float("nan"), float("inf"), -float("inf")])
def test_bad_tol_raises(bad):
    with pytest.raises(ValueError, match="tol"):
        _fill(_field(), tol=bad)


def test_bad_fields_raise():
    with pytest.raises(ValueError, match="float"):
        _fill(np.arange(24).reshape(6, 4))
    with pytest.raises(ValueError, match="float"):
        _fill(_field().astype(np.complex128))
    with pytest.raises(ValueError, match="float"):
        _fill(_field().astype(np.float16))
    with pytest.raises(ValueError, match="spatial"):
        _fill(np.arange(6.0))
    with pytest.raises(ValueError, match="no finite"):
        _fill(np.full((6, 4), np.nan))
    X = _field()
    X[3, 2] = np.inf
    with pytest.raises(ValueError, match="Inf"):
        _fill(X)
    X[3, 2] = -np.inf
    with pytest.raises(ValueError, match="Inf"):
        _fill(X)


def test_torch_tensors_are_refused_as_out_of_scope(monkeypatch):
    try:
        import torch
        tensor = torch.zeros(6, 4, dtype=torch.float64)
    except Exception:          # no torch here: a tensor is whatever the imported `torch` module calls Tensor
        import types
        torch = types.ModuleType("torch")
        torch.Tensor = type("Tensor", (), {})
        monkeypatch.setitem(sys.modules, "torch", torch)
        tensor = torch.Tensor()
    with pytest.raises(ValueError, match="out of scope"):
        _fill(tensor)


def test_bad_cross_validation_sets_raise():
    X = _field(T=12, N=7)
    present = np.flatnonzero(np.isfinite(X).reshape(-1))
    missing = np.flatnonzero(np.isnan(X).reshape(-1))
    with pytest.raises(ValueError, match="not both"):
        _fill(X, cv_fraction=0.1, cv_idx=present[:3])
    with pytest.raises(ValueError, match="out of range"):
        _fill(X, cv_idx=[present[0], X.size])
    with pytest.raises(ValueError, match="out of range"):
        _fill(X, cv_idx=[-1, present[0]])
    with pytest.raises(ValueError, match="repeated"):
        _fill(X, cv_idx=[present[0], present[1], present[0]])
    with pytest.raises(ValueError, match="missing value"):
        _fill(X, cv_idx=[present[0], missing[0]])
    with pytest.raises(ValueError, match="cv_idx"):
        _fill(X, cv_idx=[])
    with pytest.raises(ValueError, match="cv_idx"):
        _fill(X, cv_idx=[1.0, 2.0])
    with pytest.raises(ValueError, match="cv_idx"):
        _fill(X, cv_idx=[[1, 2]])
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="cv_fraction"):
            _fill(X, cv_fraction=bad)
    with pytest.raises(ValueError, match="withholds nothing"):
        _fill(X, cv_fraction=1e-6)


def test_candidates_need_a_cross_validation_set():
    with pytest.raises(ValueError, match="cross-validation"):
        _fill(_field(), (1, 2))


def test_valid_arguments_reach_the_handle_and_nothing_else_does():
    with pytest.raises(AssertionError, match="device touched: fill_gaps"):
        _fill(_field(), 2, cv_fraction=0.1, seed=1)


def test_withheld_indices_follow_the_kept_columns():
    """a flat index into T x N_full becomes one into the plane of the kept columns; cv_fraction draws with default_rng(seed)"""
    X = _field(T=6, N=5).reshape(6, 5)
    X[:, 1] = np.nan
    idx = np.array([0 * 5 + 0, 2 * 5 + 2, 5 * 5 + 4])
    X.reshape(-1)[idx] = 3.0
    flat, keep, plane, ks, many, withheld = gaps._prepare(X, 2, 10, 1e-5, None, idx, None)
    assert list(keep) == [0, 2, 3, 4] and plane.shape == (6, 4) and not many and ks == (2,)
    assert list(withheld) == [0 * 4 + 0, 2 * 4 + 1, 5 * 4 + 3] and np.all(plane.reshape(-1)[withheld] == 3.0)
    a = gaps._prepare(X, 2, 10, 1e-5, 0.25, None, 4)[5]
    b = gaps._prepare(X, 2, 10, 1e-5, 0.25, None, 4)[5]
    where = np.flatnonzero(np.isfinite(plane).reshape(-1))
    assert np.array_equal(a, b) and a.size == round(0.25 * where.size) and np.isin(a, where).all() and np.unique(a).size == a.size
    assert np.array_equal(a, np.sort(np.random.default_rng(4).choice(where, size=a.size, replace=False)))


# ---- ABI and facade -------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entries_and_the_binding_has_them():
    for name, n_args in NEW.items():
        check_entry(name, n_args)
    assert header_abi_version() == _hip.ABI_VERSION
    text = header_text(comments=True)                 # (the stage names stand in a comment)
    for stage in ("gap_center", "gap_eigh", "gap_project", "gap_fill", "gap_finish"):
        assert '"%s"' % stage in text, stage
    for method in ("fill_gaps", "gap_center", "gap_fill_step"):
        assert callable(getattr(_hip.Handle, method))


def test_the_tile_constants_of_the_cases_are_those_of_the_library():
    assert _hip.gap_fill_tile() == (C.TILE_ROWS, C.TILE_COLS)
    src = open(os.path.join(REPO, "xmca_amd", "csrc", "gap_fill.h")).read()
    assert re.search(r"GAP_KC\s*=\s*%d\b" % C.MODE_CHUNK, src)


def test_the_package_does_not_export_the_module():
    import xmca_amd
    assert "fill_gaps" not in xmca_amd.__all__ and "gaps" not in xmca_amd.__all__


def test_the_xarray_wrapper_has_the_parameters_of_fill_gaps():
    a = inspect.signature(gaps.fill_gaps).parameters
    b = inspect.signature(facade.fill_gaps).parameters
    assert list(a)[1:] == list(b)[1:] and list(b)[0] == "da"
    for name in list(a)[1:]:
        assert a[name].default == b[name].default and a[name].kind == b[name].kind, name


def test_the_xarray_wrapper_checks_before_the_device_and_wants_a_dataarray():
    da = xr.DataArray(_field(T=12, N=6).reshape(12, 2, 3), dims=["time", "lat", "lon"],
                      coords={"time": np.arange(12), "lat": [0.0, 1.0], "lon": [0.0, 1.0, 2.0]})
    with pytest.raises(ValueError, match="n_modes"):
        facade.fill_gaps(da, 0, handle=_NoDevice())
    with pytest.raises(AssertionError, match="device touched: fill_gaps"):
        facade.fill_gaps(da, 2, handle=_NoDevice())
    with pytest.raises(TypeError, match="DataArray"):
        facade.fill_gaps(da.values, 2, handle=_NoDevice())
