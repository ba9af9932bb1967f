"""GPU: `xmca_amd.prepare.anomalies` / `remove` - the mask, solve and residual kernels of csrc/regress.h around the
GEMM's moments.  The numpy restatement and the cases: tests/anomalies_cases.py (T in {17, 33, 49, 130}, N in {1, 63, 64, 65, 257},
k in {1, 2, 6, 13, 16}; six deterministic gap patterns whose fitted mask follows from integer counts).

Bounds.  float64: BOUND64 of max|X| - 8 x the worst restatement-to-device difference of the field measured on an MI355X over every
case, pattern and dtype (profiles/anomalies_accuracy.json: 1.26e-14; the factor is the margin for other inputs' rounding at the
condition numbers up to ~14 of these bases), far below the 1e-11 above which a difference is a fault to explain.  float32:
BOUND32_ULPS = 1 float32 spacing at max|X| - both sides round a float64 residual no larger than max|X| once, and the float64 values
differ by far less than a spacing (measured: 0.5).  Coefficients are float64 whatever the field's dtype and take BOUND64.  The
reference-free figures take the same bounds: the residual's weighted mean along a basis column, |sum_present b r| / sum_present |b|
(entries each within e of the exact residual keep it within e), and the coefficients of a second application (measured: 4.4e-16 and
1.3e-15 of max|X| in float64; 0.07 and 0.13 spacings in float32)."""
import numpy as np
import pytest

import anomalies_cases as C
from xmca_amd import _hip, gaps
from xmca_amd.array import MCA
from xmca_amd.prepare import anomalies, remove, time_basis

pytestmark = pytest.mark.gpu

BOUND64 = 1.0113e-13          # x max|X| (profiles/anomalies_accuracy.json, bounds.float64_of_max_abs_X)
BOUND32_ULPS = 1.0            # float32 spacings at max|X| (bounds.float32_ulps_of_max_abs_X)
DTYPES = ["float64", "float32"]
RUNS = [(case, pattern) for case in C.CASES for pattern in C.patterns_of(case)]


def _run_name(run):
    return C.case_name(run[0]) + "-" + run[1]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _bound(dtype):
    """the bound of a field figure in the units of `anomalies_cases.figures`"""
    return BOUND64 if np.dtype(dtype) == np.float64 else BOUND32_ULPS


def test_the_float64_bound_is_below_the_level_of_a_fault():
    assert BOUND64 < 1e-11


def test_the_cases_know_the_tile_of_the_library():
    rows, cols = _hip.reg_residual_tile()
    assert max(c[0] for c in C.CASES) > 2 * rows > rows > min(c[0] for c in C.CASES) and max(c[1] for c in C.CASES) == cols + 1


# ---- against the restatement, and the checks that need no reference ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", RUNS, ids=_run_name)
def test_against_the_restatement(hip, run, dtype):
    case, pattern = run
    X, expected = C.case_field(case, pattern, dtype)
    B = C.basis_of(case)
    out = anomalies(X, handle=hip, **C.BASES[case[2]])
    assert out["field"].shape == X.shape and out["field"].dtype == X.dtype and isinstance(out["field"], np.ndarray)
    assert out["coefficients"].shape == (case[2], case[1]) and out["coefficients"].dtype == np.float64
    assert out["fitted"].dtype == bool and np.array_equal(out["fitted"], expected)          # every column, exactly
    assert np.array_equal(out["basis"], B)
    # NaN positions: those of X in a fitted column, everything elsewhere
    assert np.array_equal(np.isnan(out["field"][:, expected]), np.isnan(X[:, expected])) and np.isnan(out["field"][:, ~expected]).all()
    assert np.isfinite(out["coefficients"][:, expected]).all() and np.isnan(out["coefficients"][:, ~expected]).all()
    again = anomalies(out["field"], basis=B, handle=hip)
    assert np.array_equal(again["fitted"], expected)
    fig = C.figures(case, pattern, dtype, out, again)
    print(_run_name(run), dtype, fig)
    assert fig["field"] <= _bound(dtype)
    assert fig["coefficients"] <= BOUND64
    assert fig["orthogonality"] <= _bound(dtype)
    assert fig["refit"] <= _bound(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", [((130, 257, 13), "random"), ((49, 257, 16), "few"), ((33, 64, 13), "phase"), ((17, 1, 1), "none"),
                                 ((130, 63, 16), "none")], ids=_run_name)
def test_a_repeated_call_and_remove_give_the_same_bits(hip, run, dtype):
    case, pattern = run
    X = C.case_field(case, pattern, dtype)[0]
    a = anomalies(X, handle=hip, **C.BASES[case[2]])
    b = anomalies(X, handle=hip, **C.BASES[case[2]])
    assert np.array_equal(_bits(a["field"]), _bits(b["field"])) and np.array_equal(_bits(a["coefficients"]), _bits(b["coefficients"]))
    r = remove(X, a["basis"], a["coefficients"], handle=hip)
    assert r.dtype == X.dtype and np.array_equal(_bits(r), _bits(a["field"]))


def test_remove_subtracts_a_fitted_model_from_later_time_steps(hip):
    """the model of the first 49 steps, evaluated on the next 17 by `time_basis(start=, span=)`, against numpy"""
    T, T2, N = 49, 17, 65
    X = C.case_field((T, N, 13), "random")[0]
    out = anomalies(X, period=12, trend=True, handle=hip)
    rng = np.random.default_rng(4)
    Y = 15.0 + rng.standard_normal((T2, N))
    Y[3, 5] = np.nan
    B2 = time_basis(T2, period=12, trend=True, start=T, span=T)
    got = remove(Y, B2, out["coefficients"], handle=hip)
    want = Y - B2 @ out["coefficients"]
    assert C.max_abs_diff(got, want) <= BOUND64 * np.nanmax(np.abs(Y))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(33, 63), (130, 257)], ids=str)
def test_the_mean_alone_is_the_centring_of_gap_center(hip, shape, dtype):
    case = shape + (1,)
    X = C.case_field(case, "random", dtype)[0]
    mean, mask, A, scale = hip.gap_center(X)
    out = anomalies(X, handle=hip)
    present = np.isfinite(X)
    unit = np.nanmax(np.abs(X)) if dtype == "float64" else C.ulp32(np.nanmax(np.abs(X)))
    assert np.array_equal(mask.astype(bool), ~present) and out["fitted"].all()
    assert np.max(np.abs(out["field"].astype(np.float64)[present] - A[present])) <= _bound(dtype) * unit
    assert np.max(np.abs(out["coefficients"][0] - mean)) <= BOUND64 * np.nanmax(np.abs(X))


# ---- the kernels alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(17, 1), (33, 65), (130, 257), (1, 1100)], ids=str)
def test_the_mask_pass_alone(hip, shape, dtype):
    rng = np.random.default_rng(shape[0] + shape[1])
    X = rng.standard_normal(shape).astype(dtype)
    X[rng.random(shape) < 0.3] = np.nan
    X[0, -1] = np.nan
    mask, wide, missing = hip.reg_mask(X)
    assert mask.dtype == np.uint8 and np.array_equal(mask, np.isnan(X).astype(np.uint8)) and missing == int(np.isnan(X).sum())
    assert np.array_equal(_bits(wide), _bits(np.where(np.isnan(X), 0.0, X.astype(np.float64))))
    full = np.ones(shape, dtype=dtype)
    assert hip.reg_mask(full)[2] == 0


@pytest.mark.parametrize("k", [1, 2, 3, 6, 13, 16])
def test_the_solve_kernel_alone(hip, k):
    """random well-posed normal matrices per column against numpy.linalg.solve; the count rule, a zero diagonal entry, a pivot just
    below and just above the criterion, a NaN; and one matrix shared by all columns"""
    N = 130
    rng = np.random.default_rng(k)
    G = rng.standard_normal((N, 3 * k + 2, k))
    A = np.einsum("ntk,ntl->nkl", G, G)
    rhs = rng.standard_normal((k, N))
    low = np.tril_indices(k)
    normal = np.empty((k * (k + 1) // 2 + 1, N))
    normal[:-1] = A[:, low[0], low[1]].T
    normal[-1] = 3 * k + 2
    expected = np.ones(N, dtype=bool)
    normal[-1, 5] = k - 1                        # too few present values
    expected[5] = False
    normal[-1, 6] = k                            # just enough
    normal[k * (k + 1) // 2 - 1, 7] = 0.0        # the last diagonal entry zero: the pivot is not above 1e-8 x 0
    expected[7] = False
    normal[0, 8] = np.nan
    expected[8] = False
    if k >= 2:                                   # columns 9, 10: [[1, c], [c, 1]] in the leading block, pivot share 1 - c^2
        for n, share, ok in ((9, 0.5e-8, False), (10, 2e-8, True)):
            A[n] = np.eye(k)
            A[n, 1, 0] = A[n, 0, 1] = np.sqrt(1.0 - share)
            normal[:-1, n] = A[n][low]
            expected[n] = ok
    coef, fitted = hip.reg_solve(normal, rhs)
    assert np.array_equal(fitted, expected) and np.isnan(coef[:, ~expected]).all()
    for n in np.flatnonzero(expected):
        want = np.linalg.solve(A[n], rhs[:, n])
        cond = np.linalg.cond(A[n])
        assert np.max(np.abs(coef[:, n] - want)) <= 64 * k * cond * 2.0 ** -53 * np.max(np.abs(want)), (n, cond)
    c1, f1 = hip.reg_solve(normal[:, 0].copy(), rhs)
    assert f1.all()
    want = np.linalg.solve(A[0], rhs)
    assert np.max(np.abs(c1 - want)) <= 64 * k * np.linalg.cond(A[0]) * 2.0 ** -53 * np.max(np.abs(want))
    assert np.array_equal(_bits(c1[:, 0]), _bits(coef[:, 0]))          # shared or per column: the same arithmetic


def test_the_entry_points_refuse_bad_arguments_before_any_launch(hip):
    """XMCA_ERR_INVALID from the C entries themselves (the Python layer checks the same things earlier): k outside [1, 16], T < 1,
    N < 1, a bad dtype, a negative stride; the handle stays usable"""
    X, B = np.ones((20, 3)), np.zeros((20 * 17,))
    B[:40] = np.stack([np.ones(20), np.arange(20) / 20.0], axis=1).reshape(-1)          # (the 20 x 2 basis the good calls read)
    field, coef, fit = np.empty((20, 3)), np.empty((17, 3)), np.empty(3, dtype=np.uint8)
    p = _hip._ptr

    def regress(T=20, N=3, stride_t=3, stride_n=1, dtype=_hip.XMCA_F64, k=2):
        return hip._lib.xmca_column_regress(hip._h, p(X), _hip.HOST, T, N, stride_t, stride_n, dtype, p(B), k, p(field), _hip.HOST, p(coef), p(fit))
    assert regress() == 0
    for bad in (dict(k=0), dict(k=17), dict(T=0), dict(N=0), dict(dtype=7), dict(stride_t=-1), dict(stride_n=-1)):
        assert regress(**bad) == _hip.ERR_INVALID, bad
    for k in (0, 17):
        assert hip._lib.xmca_column_residual(hip._h, p(X), _hip.HOST, 20, 3, 3, 1, _hip.XMCA_F64, p(B), k, p(coef), p(field),
                                             _hip.HOST) == _hip.ERR_INVALID
        assert hip._lib.xmca_reg_solve(hip._h, p(np.ones(200 * 3)), 0, p(np.ones(17 * 3)), 3, k, p(coef), p(fit)) == _hip.ERR_INVALID
    with pytest.raises(ValueError, match="k"):
        hip.column_regress(X, np.ones((20, 17)))
    assert regress() == 0 and fit.all() and np.max(np.abs(field)) < 1e-13


# ---- tensors -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["contiguous", "transposed", "column slice", "three dimensions", "spatial sub-box",
                                    "spatial sub-box on a side stream", "permuted spatial axes"])
def test_a_gpu_tensor_gives_a_gpu_tensor_with_the_bits_of_the_numpy_route(hip, layout, dtype):
    import torch
    case = (49, 65, 13)
    X = C.case_field(case, "random", dtype)[0]
    want = anomalies(X, period=12, trend=True, handle=hip)
    dev = torch.device("cuda", hip.device)
    if layout == "contiguous":
        t = torch.from_numpy(X.copy()).to(dev)
    elif layout == "transposed":
        t = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev).T
        assert t.stride() == (1, 49)
    elif layout == "column slice":
        wide = torch.full((49, 80), 7.0, dtype=getattr(torch, dtype), device=dev)
        wide[:, 10:75] = torch.from_numpy(X.copy()).to(dev)
        t = wide[:, 10:75]
        assert t.stride() == (80, 1)
    elif layout == "three dimensions":
        t = torch.from_numpy(X.copy()).to(dev).reshape(49, 5, 13)
    elif layout.startswith("spatial sub-box"):          # no two strides express (T, N): torch makes a contiguous copy first
        big = torch.full((49, 7, 15), 7.0, dtype=getattr(torch, dtype), device=dev)
        big[:, 1:6, 1:14] = torch.from_numpy(X.copy()).to(dev).reshape(49, 5, 13)
        t = big[:, 1:6, 1:14]
        assert not t.is_contiguous() and t.stride() == (105, 15, 1)
    else:
        t = torch.from_numpy(np.ascontiguousarray(X.reshape(49, 5, 13).transpose(0, 2, 1))).to(dev).permute(0, 2, 1)
        assert tuple(t.shape) == (49, 5, 13) and t.stride() == (65, 1, 5)
    before = t.clone()
    torch.cuda.synchronize(dev)
    if layout.endswith("side stream"):
        # the copy torch makes is queued on the caller's current stream, here one that does not wait for the null stream: the
        # library, which reads on a stream of its own, must see it finished.  A large fill ahead of the call keeps the stream busy.
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            busy = torch.zeros(64 * 1024 * 1024, dtype=torch.float64, device=dev)
            busy.add_(1.0)
            out = anomalies(t, period=12, trend=True, handle=hip)
            r_side = remove(t, out["basis"], out["coefficients"], handle=hip)
        side.synchronize()
        assert torch.equal(_tbits(r_side), _tbits(out["field"]))
    else:
        out = anomalies(t, period=12, trend=True, handle=hip)
    assert isinstance(out["field"], torch.Tensor) and out["field"].device == dev and out["field"].dtype == t.dtype
    assert tuple(out["field"].shape) == tuple(t.shape) and out["field"].is_contiguous()
    got = out["field"].cpu().numpy().reshape(X.shape)
    assert np.array_equal(_bits(got), _bits(want["field"]))
    assert isinstance(out["coefficients"], np.ndarray) and out["coefficients"].shape == (13,) + tuple(t.shape[1:])
    assert np.array_equal(_bits(out["coefficients"].reshape(13, -1)), _bits(want["coefficients"]))
    assert np.array_equal(out["fitted"].reshape(-1), want["fitted"])
    assert torch.equal(torch.nan_to_num(t, nan=-1.0), torch.nan_to_num(before, nan=-1.0))          # the input is unchanged
    r = remove(t, out["basis"], out["coefficients"], handle=hip)
    assert isinstance(r, torch.Tensor) and torch.equal(_tbits(r), _tbits(out["field"]))


def _tbits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def test_a_tensor_with_an_inf_is_refused(hip):
    import torch
    t = torch.ones(20, 4, dtype=torch.float64, device=torch.device("cuda", hip.device))
    t[3, 1] = float("inf")
    with pytest.raises(ValueError, match="Inf"):
        anomalies(t, period=4, handle=hip)


# ---- state and pipeline --------------------------------------------------------------------------------------------------------------
def test_a_solved_rotated_model_on_the_handle_keeps_its_result_to_the_bit(hip):
    rng = np.random.default_rng(11)
    F = rng.standard_normal((40, 6)) @ rng.standard_normal((6, 90)) + 0.1 * rng.standard_normal((40, 90))
    m = MCA(F, handle=hip)
    m.solve()
    m.rotate(3)
    before = (m.singular_values().copy(), m.eofs(3)['left'].copy(), m.pcs(3)['left'].copy())
    X = C.case_field((130, 257, 13), "random")[0]
    hip.reset_timings()
    out = anomalies(X, period=12, trend=True, handle=hip)
    assert {"reg_mask", "reg_moments", "reg_solve", "reg_residual"} <= set(hip.timings())
    remove(X, out["basis"], out["coefficients"], handle=hip)
    for a, b in zip(before, (m.singular_values(), m.eofs(3)['left'], m.pcs(3)['left'])):
        assert np.array_equal(_bits(a), _bits(b))


def test_the_pipeline_anomalies_then_fill_gaps(hip):
    X, expected = C.case_field(C.PIPELINE_CASE, "column")
    prep = anomalies(X, period=12, handle=hip)
    assert np.array_equal(prep["fitted"], expected) and np.isnan(prep["field"]).any()
    out = gaps.fill_gaps(prep["field"], n_modes=3, max_iter=5, tol=0, handle=hip)
    assert out["iterations"] == 5 and out["field"].shape == X.shape
    assert np.isfinite(out["field"][:, expected]).all() and np.isnan(out["field"][:, ~expected]).all()
    present = np.isfinite(prep["field"])
    assert np.array_equal(out["field"][present], prep["field"][present])
