"""GPU: `MCA.extended_rule_n` - the Monte-Carlo SSA test of extended EOFs: surrogates projected on the data's
patterns by one thin product and a shift sum (csrc/lag_project.h).  Truth and cases: tests/extended_rule_n_cases.py.

  * the projection kernels alone through `Handle.lag_project` against float64 numpy at shapes on the edges of their tile;
  * `Handle.extended_project` with R = the resident field and no scale: the eigenvalues of `extended_eofs`;
  * `extended_rule_n` against the truth formed from the device's own surrogates (`Handle.surrogate_ar1`) with the explicitly
    embedded matrices, per run; the column scale against numpy's std(ddof=1); phi = 0 against the white surrogates;
  * bits: a repeated call, a run range in two parts, a solved and rotated model left as it was, the facade;
  * a planted oscillatory pair in AR(1) noise stands out, the noise modes do not.

Errors are |Lambda - Lambda_truth| / lambda_1.  BOUND holds ten times the largest error measured on an MI355X over all cases of
a dtype (profiles/extended_rule_n_accuracy.json; written again to the file named by XMCA_EXTENDED_RULE_N_ACCURACY when set)."""
import json
import os
import sys

import numpy as np
import pytest

import ar1_cases as A
import extended_rule_n_cases as C
from xmca_amd import _hip
from xmca_amd.array import MCA

pytestmark = pytest.mark.gpu

BOUND = {np.float64: 6.5e-13, np.float32: 3.2e-7}       # 10 x 6.5e-14 (an eigenvalue, M = 12) and 10 x 3.2e-8 (the projected field)
EPS = np.finfo(np.float64).eps
WORST = {}


def _note(dtype, name, err):
    key = np.dtype(dtype).name
    print("%s %s: %.3g" % (name, key, err))
    WORST.setdefault(key, {})[name] = max(WORST.get(key, {}).get(name, 0.0), float(err))


# ---- the projection kernels alone ---------------------------------------------------------------------------------------
def _kernel_shapes():
    """(T', M, tau, k): T' around the row tile, over more than two tiles and the minimal T' = 1; tau below and above the tile;
    M = 1; k = 1; M k = 15 and 120; k past the column tile"""
    rows, cols = _hip.lag_project_tile()
    out = [(Tp, M, tau, k) for Tp in (1, rows - 1, rows, rows + 1, 2 * rows + 3) for M, k in ((1, 1), (1, 7), (3, 5), (12, 10))
           for tau in (1, rows - 1, rows + 5)]
    return out + [(rows + 9, 2, 3, cols + 6), (3 * rows + 1, 4, 2, 1), (2 * rows, 3, 2 * rows + 1, 2 * cols + 1)]


def test_projection_kernels_match_numpy_at_the_tile_edges(hip):
    """Device and numpy add the same M terms per entry of Q (the same order) and differ in the order of the column sums: means of
    T' terms, then T' squares.  With S_c = sum_t Q[t, c]^2 of the UNCENTRED Q - the size the roundings of the mean are relative
    to - both stay within 2 (T' + M + 4) eps S_c of the exact value, so within twice that of each other."""
    rng = np.random.default_rng(17)
    worst = 0.0
    hip.reset_timings()
    for Tp, M, tau, k in _kernel_shapes():
        T = Tp + (M - 1) * tau
        W = rng.standard_normal((T, M * k)) + rng.standard_normal(M * k)          # (columns with a mean: the centring matters)
        out = hip.lag_project(W, M, tau, k)
        ref = C.lag_project(W, M, tau, k)
        Q = sum(W[j * tau:j * tau + Tp, j * k:(j + 1) * k] for j in range(M))
        bound = 4 * (Tp + M + 4) * EPS * np.sum(Q * Q, axis=0)
        assert out.shape == (k,) and out.dtype == np.float64
        assert np.all(np.abs(out - ref) <= bound), (Tp, M, tau, k, np.max(np.abs(out - ref) / bound))
        worst = max(worst, float(np.max(np.abs(out - ref) / bound)))
        assert np.array_equal(out, hip.lag_project(W, M, tau, k)), (Tp, M, tau, k)
        if Tp == 1:
            assert np.all(out == 0.0)
    _note(np.float64, "lag_project_over_its_bound", worst)
    assert "mcssa_project" in hip.timings()


def test_lag_project_refuses_an_embedding_that_does_not_fit(hip):
    W = np.zeros((10, 6))
    with pytest.raises(ValueError):
        hip.lag_project(W, 3, 5, 2)
    rc = hip._lib.xmca_lag_project(hip._h, _hip._ptr(W), 10, 3, 5, 2, _hip._ptr(np.zeros(2)))
    assert rc == _hip.ERR_INVALID
    rc = hip._lib.xmca_lag_project(hip._h, _hip._ptr(W), 10, 3, 1, 0, _hip._ptr(np.zeros(2)))
    assert rc == _hip.ERR_INVALID


# ---- projecting the data ----------------------------------------------------------------------------------------------------
def _model(hip, case, dtype):
    """(model, handle with the field resident, the resident T x N field widened to float64, kept mask or None, M, tau, k)"""
    if len(case) == 8:
        name, T, shape, masked, M, tau, k, seed = case
        full, X, keep = C.masked_separated_field(T, shape, masked, seed)
        m = MCA(full.astype(dtype), handle=hip)
    else:
        name, T, N, M, tau, k, seed = case
        keep = None
        m = MCA(C.separated_field(T, N, seed).astype(dtype), handle=hip)
    dev = m._resident_device()
    n_kept = N if keep is None else int(keep.sum())
    X = dev.get_field(0, (T, n_kept), dtype).astype(np.float64)
    return m, dev, X, keep, M, tau, k


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", C.CASES + [C.MASKED_CASE], ids=lambda c: c[0])
def test_projecting_the_field_itself_returns_the_eigenvalues(hip, case, dtype):
    m, dev, X, keep, M, tau, k = _model(hip, case, dtype)
    T, N = X.shape
    Tp = T - (M - 1) * tau
    lam = m.extended_eofs(M, tau=tau, n_modes=k)['singular_values'] * (Tp - 1)
    out = dev.extended_project(T, N, M, tau, k, X, False)
    err = np.max(np.abs(out - lam)) / lam[0]
    _note(dtype, "project_field_" + case[0], err)
    assert err <= BOUND[dtype], (err, out, lam)
    # ... and they are those of the explicitly embedded matrix
    ref = C.patterns(X, M, tau, k)[0][:k]
    assert np.max(np.abs(out - ref)) / ref[0] <= BOUND[dtype]
    # with the scale folded in: the field with every column multiplied by its standard deviation
    d = X.std(axis=0, ddof=1)
    lam_ref, V = C.patterns(X, M, tau, k)
    scaled = dev.extended_project(T, N, M, tau, k, X, True)
    err = np.max(np.abs(scaled - C.truth(V, X * d, M, tau))) / lam_ref[0]
    _note(dtype, "project_scaled_field_" + case[0], err)
    assert err <= BOUND[dtype], err
    assert np.array_equal(out, dev.extended_project(T, N, M, tau, k, X, False))


# ---- the test against the truth ---------------------------------------------------------------------------------------------
def _check_runs(name, dtype, hip, out, X, keep, M, tau, k, seed, n_runs, white=False):
    T, N = X.shape
    Tp = T - (M - 1) * tau
    lam, V = C.patterns(X, M, tau, k)
    sel = slice(None) if keep is None else keep
    scale, phi = out['scale'].reshape(-1)[sel], out['phi'].reshape(-1)[sel]
    if keep is not None:
        assert np.isnan(out['scale'].reshape(-1)[~keep]).all() and np.isnan(out['phi'].reshape(-1)[~keep]).all()
    assert not np.isnan(scale).any() and not np.isnan(phi).any()
    for key in ('singular_values', 'surrogates', 'exceedance', 'phi', 'scale'):
        assert out[key].dtype == np.float64, key
    assert out['surrogates'].shape == (k, n_runs) and out['singular_values'].shape == (k,) and out['exceedance'].shape == (k,)
    # the column scale: a sum of T squared deviations in float64, in another order than numpy's
    assert np.max(np.abs(scale / X.std(axis=0, ddof=1) - 1)) <= 4 * (T + 4) * EPS
    err_lam = np.max(np.abs(out['singular_values'] * (Tp - 1) - lam[:k])) / lam[0]
    _note(dtype, "eigenvalues_" + name, err_lam)
    assert err_lam <= BOUND[dtype]
    worst = 0.0
    for run in range(n_runs):
        if white:
            R = hip.surrogate(T * N, seed, run, 0).reshape(T, N).astype(dtype).astype(np.float64)
        else:
            R = hip.surrogate_ar1(T, N, phi, seed, run, 0, dtype)
        ref = C.truth(V, R * scale, M, tau)
        worst = max(worst, np.max(np.abs(out['surrogates'][:, run] * (Tp - 1) - ref)) / lam[0])
    _note(dtype, ("white_" if white else "runs_") + name, worst)
    assert worst <= BOUND[dtype], worst
    assert np.array_equal(out['exceedance'], np.mean(out['surrogates'] >= out['singular_values'][:, None], axis=1))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", C.RULE_N_CASES + [C.MASKED_CASE], ids=lambda c: c[0])
def test_every_run_matches_the_explicitly_embedded_surrogate(hip, case, dtype):
    m, dev, X, keep, M, tau, k = _model(hip, case, dtype)
    T, N = X.shape
    hip.reset_timings()
    out = m.extended_rule_n(M, tau=tau, n_runs=C.N_RUNS, n_modes=k, seed=C.SEED)
    phi = out['phi'].reshape(-1)[slice(None) if keep is None else keep]
    assert np.max(np.abs(phi - A.lag1(X))) <= 4 * T * EPS                      # phi = None: the estimate of the field
    _check_runs(case[0], dtype, hip, out, X, keep, M, tau, k, C.SEED, C.N_RUNS)
    assert np.array_equal(out['singular_values'], m.extended_eofs(M, tau=tau, n_modes=k)['singular_values'])
    assert {"lag_gram", "eeof_eigh", "eeof_project", "mcssa_scale", "mcssa_surrogate", "mcssa_gemm", "mcssa_project"} <= set(hip.timings())


def test_one_of_the_shapes_has_a_filter_of_several_segments():
    assert any(len(_hip.ar1_segments(c[1], c[2])) > 1 for c in C.RULE_N_CASES)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_a_given_phi_is_used_and_phi_zero_gives_the_white_surrogates(hip, dtype):
    case = C.CASES[1]
    m, dev, X, keep, M, tau, k = _model(hip, case, dtype)
    T, N = X.shape
    white = m.extended_rule_n(M, tau=tau, n_runs=3, n_modes=k, seed=7, phi=0)
    assert np.all(white['phi'] == 0.0)
    _check_runs(case[0], dtype, hip, white, X, keep, M, tau, k, 7, 3, white=True)
    given = A.cycled_phi(N) * 0.9
    red = m.extended_rule_n(M, tau=tau, n_runs=3, n_modes=k, seed=7, phi=given)
    assert np.array_equal(red['phi'], given)
    _check_runs(case[0] + "_given_phi", dtype, hip, red, X, keep, M, tau, k, 7, 3)
    assert not np.array_equal(red['surrogates'], white['surrogates'])
    with pytest.raises(ValueError):                    # the library's own check, in front of every launch
        dev.extended_rule_n(T, N, M, tau, k, np.full(N, 1.0), 0, 2, 7)
    assert np.array_equal(m.extended_rule_n(M, tau=tau, n_runs=3, n_modes=k, seed=7, phi=0)['surrogates'], white['surrogates'])


# ---- bits -------------------------------------------------------------------------------------------------------------------
def test_a_repeated_call_and_a_split_run_range_give_the_same_bits(hip):
    case = C.CASES[2]
    m, dev, X, keep, M, tau, k = _model(hip, case, np.float64)
    T, N = X.shape
    first = m.extended_rule_n(M, tau=tau, n_runs=5, n_modes=k, seed=3)
    second = m.extended_rule_n(M, tau=tau, n_runs=5, n_modes=k, seed=3)
    for key in first:
        assert np.array_equal(first[key], second[key]), key
    phi = first['phi'].reshape(-1)
    lam, scale, whole = dev.extended_rule_n(T, N, M, tau, k, phi, 0, 5, 3)
    assert np.array_equal(whole.T / (T - (M - 1) * tau - 1), first['surrogates'])
    a = dev.extended_rule_n(T, N, M, tau, k, phi, 0, 2, 3)
    b = dev.extended_rule_n(T, N, M, tau, k, phi, 2, 5, 3)
    assert np.array_equal(np.concatenate([a[2], b[2]]), whole)
    assert np.array_equal(a[0], lam) and np.array_equal(b[1], scale)
    empty = dev.extended_rule_n(T, N, M, tau, k, phi, 4, 4, 3)
    assert empty[2].shape == (0, k) and np.array_equal(empty[0], lam)
    other = m.extended_rule_n(M, tau=tau, n_runs=5, n_modes=k, seed=4)
    assert not np.array_equal(other['surrogates'], first['surrogates'])
    np.random.seed(123)                                 # seed = None draws from numpy's global stream, as rule_n does
    drawn = m.extended_rule_n(M, tau=tau, n_runs=2, n_modes=k)
    np.random.seed(123)
    assert np.array_equal(drawn['surrogates'], m.extended_rule_n(M, tau=tau, n_runs=2, n_modes=k)['surrogates'])


def test_a_solved_and_rotated_model_keeps_its_result_to_the_bit(hip):
    name, T, N, M, tau, k, seed = C.CASES[3]
    m = MCA(C.separated_field(T, N, seed), handle=hip)
    m.solve()
    m.rotate(3)
    before = (m.singular_values().copy(), m.eofs(3)['left'].copy(), m.pcs(3)['left'].copy())
    first = m.extended_rule_n(M, tau=tau, n_runs=3, n_modes=k, seed=1)
    for a, b in zip(before, (m.singular_values(), m.eofs(3)['left'], m.pcs(3)['left'])):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):                    # a refused call leaves the handle usable
        hip.extended_rule_n(T, N, M, tau, T, np.zeros(N), 0, 2, 1)
    second = m.extended_rule_n(M, tau=tau, n_runs=3, n_modes=k, seed=1)
    assert np.array_equal(first['surrogates'], second['surrogates'])
    for a, b in zip(before, (m.singular_values(), m.eofs(3)['left'], m.pcs(3)['left'])):
        assert np.array_equal(a, b)


def test_the_facade_passes_the_dict_through(hip):
    try:
        import xarray as xr
    except Exception:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
        import xarray as xr
    from xmca_amd.xarray import xMCA
    name, T, shape, masked, M, tau, k, seed = C.MASKED_CASE
    full, X, keep = C.masked_separated_field(T, shape, masked, seed)
    time, lat, lon = np.arange(T) * 10, np.linspace(-20, 20, shape[0]), np.linspace(0, 50, shape[1])
    xm = xMCA(xr.DataArray(full, dims=['time', 'lat', 'lon'], coords={'time': time, 'lat': lat, 'lon': lon}))
    xm._handle_override = hip
    out = xm.extended_rule_n(M, tau=tau, n_runs=3, n_modes=k, seed=9)
    ref = MCA(full, handle=hip).extended_rule_n(M, tau=tau, n_runs=3, n_modes=k, seed=9)
    assert sorted(out) == sorted(ref) == ['exceedance', 'phi', 'scale', 'singular_values', 'surrogates']
    for key in ref:
        assert isinstance(out[key], np.ndarray) and np.array_equal(out[key], ref[key], equal_nan=True), key
    assert out['phi'].shape == tuple(shape) and np.array_equal(np.isnan(out['scale']).reshape(-1), ~keep)


# ---- a planted signal -------------------------------------------------------------------------------------------------------
def test_a_planted_oscillatory_pair_stands_out_of_red_noise(hip):
    """the field and seed of tests/test_extended_rule_n_host.py, where the truth alone decides the same with room to spare"""
    p = C.PLANTED
    out = MCA(C.planted_field(), handle=hip).extended_rule_n(p["M"], tau=p["tau"], n_runs=p["n_runs"], n_modes=p["k"], seed=p["seed"])
    assert np.all(out['exceedance'][:2] == 0.0), out['exceedance']
    assert np.any((out['exceedance'][2:] > 0.0) & (out['exceedance'][2:] < 1.0)), out['exceedance']
    lam, runs = C.planted_truth()              # (its normals come from the numpy twin of the generator, its phi from numpy)
    assert np.max(np.abs(out['exceedance'] - np.mean(runs >= lam, axis=0))) <= 1.0 / p["n_runs"]


def test_zz_write_accuracy_record():
    """(last in the file) the worst errors of the cases, for profiles/extended_rule_n_accuracy.json"""
    path = os.environ.get("XMCA_EXTENDED_RULE_N_ACCURACY")
    if path and WORST:
        largest = {key: max(v for name, v in errs.items() if not name.startswith("lag_project")) for key, errs in WORST.items()}
        with open(path, "w") as f:
            json.dump({"bounds": {np.dtype(t).name: b for t, b in BOUND.items()}, "largest_error": largest, "errors": WORST}, f, indent=1,
                      sort_keys=True)
