"""GPU: `MCA.extended_eofs` - EOFs of the lag-embedded field from a lag-summed, doubly centred Gram matrix
(csrc/lag_gram.h).  Truth and cases: tests/extended_eofs_cases.py.

  * the lag-sum kernel alone through `Handle.lag_gram` on integer-valued matrices, where every sum is exact: bit equality with
    numpy at shapes on the edges of its tile and of its two read paths, and the same bits on a second call;
  * lag sum and double centring on real-valued matrices against numpy's, to the bound of sums of T' + M terms;
  * end to end through `MCA.extended_eofs` against the SVD of the explicitly embedded, centred matrix at the project's model
    tolerances (tests/test_gpu_configs.py): 1e-5 / 1e-10 for float64 fields, 1e-3 / 2e-5 for float32 ones;
  * `extended_eofs(1)` against `solve()`, a solved and rotated model left bit-identical, refusals, the xarray facade.

The worst measured errors of the end-to-end cases go to the file named by XMCA_EXTENDED_EOFS_ACCURACY when that is set
(profiles/extended_eofs_accuracy.json holds the MI355X figures)."""
import json
import os
import sys

import numpy as np
import pytest

import extended_eofs_cases as C
from xmca_amd import _hip
from xmca_amd.array import MCA

pytestmark = pytest.mark.gpu

TOL = {np.float64: (1e-5, 1e-10), np.float32: (1e-3, 2e-5)}       # (patterns and PCs, singular values and explained variance)
WORST = {}


def _tile():
    return _hip.lag_gram_tile()


def _edge_shapes():
    """(T', M, tau) on the kernel's edges: T' around the tile and over more than two tiles, the minimal T' = 2; tau around the tile
    (below it the M windows of a tile overlap and may be staged as one band; from M = 5, tau = tile - 1 on the band no longer fits
    and plain reads take over); T' = 2 with tau = 3 and T' = tile + 1 with tau = tile + 8 are embeddings whose windows share no row"""
    t = _tile()
    out = [(Tp, M, tau) for Tp in (2, t - 1, t, t + 1, 2 * t + 3) for M in (1, 2, 5) for tau in (1, 3, t - 1, t, t + 1)]
    return out + [(t + 1, 3, t + 8)]


def _symmetric_integers(n, seed):
    a = np.random.default_rng(seed).integers(-2 ** 20 + 1, 2 ** 20, (n, n)).astype(np.float64)
    return np.triu(a) + np.triu(a, 1).T


@pytest.mark.parametrize("Tp_index", range(5))
def test_lag_sum_of_integer_matrices_is_numpy_to_the_bit(hip, Tp_index):
    """|g| < 2^20 and M <= 5: every partial sum is an integer below 2^23, exact in any order"""
    t = _tile()
    Tp_here = (2, t - 1, t, t + 1, 2 * t + 3)[Tp_index]
    for Tp, M, tau in [s for s in _edge_shapes() if s[0] == Tp_here]:
        n = Tp + (M - 1) * tau
        G = _symmetric_integers(n, [Tp, M, tau])
        K = hip.lag_gram(G, M, tau, False)
        assert K.shape == (Tp, Tp)
        assert np.array_equal(K, C.lag_sum(G, M, tau)), (Tp, M, tau)
        assert np.array_equal(K, hip.lag_gram(G, M, tau, False)), (Tp, M, tau)


def _real_gram(n, seed):
    X = C.case_field(n, 17, seed)
    G = X @ X.T
    return (G + G.T) / 2


@pytest.mark.parametrize("Tp_index", range(5))
def test_double_centring_matches_numpy_to_the_bound_of_its_sums(hip, Tp_index):
    """Device and numpy centre the same K (the lag sums of M terms, then means of T' terms): in any order of the sums they differ
    by at most (T' + M) 2^-52 max|K|, and rows and columns of the result sum to zero within the same bound"""
    t = _tile()
    Tp_here = (2, t - 1, t, t + 1, 2 * t + 3)[Tp_index]
    for Tp, M, tau in [s for s in _edge_shapes() if s[0] == Tp_here]:
        n = Tp + (M - 1) * tau
        G = _real_gram(n, 3)
        K = C.lag_sum(G, M, tau)
        bound = (Tp + M) * 2.0 ** -52 * np.abs(K).max()
        Kc = hip.lag_gram(G, M, tau, True)
        err = np.abs(Kc - C.double_center(K)).max()
        rows, cols = np.abs(Kc.sum(axis=1)).max(), np.abs(Kc.sum(axis=0)).max()
        print("T' = %d, M = %d, tau = %d: error %.3g, row sums %.3g, column sums %.3g, bound %.3g" % (Tp, M, tau, err, rows, cols, bound))
        assert err <= bound, (Tp, M, tau, err, bound)
        assert rows <= bound and cols <= bound, (Tp, M, tau, rows, cols, bound)
        assert np.array_equal(Kc, Kc.T)
        assert np.array_equal(Kc, hip.lag_gram(G, M, tau, True)), (Tp, M, tau)
        # ... and without the centring the same call returns the lag sum (real values: to the rounding of M terms)
        assert np.abs(hip.lag_gram(G, M, tau, False) - K).max() <= M * 2.0 ** -52 * np.abs(K).max()


def test_lag_gram_refuses_an_embedding_that_does_not_fit(hip):
    G = _symmetric_integers(10, 1)
    with pytest.raises(ValueError):
        hip.lag_gram(G, 4, 4, False)
    with pytest.raises(ValueError):
        hip.lag_gram(G, 0, 1, False)
    with pytest.raises(ValueError):
        hip.lag_gram(G[:, :9], 2, 1, False)
    assert np.array_equal(hip.lag_gram(G, 1, 1, False), G)


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _check_against_truth(name, out, ref, key, M, k, Tp, dtype, keep=None):
    tol_vec, tol_val = TOL[dtype]
    assert out['singular_values'].dtype == np.float64 and out['singular_values'].shape == (k,)
    assert out['explained_variance'].dtype == np.float64 and out['explained_variance'].shape == (k,)
    assert out['pcs'].dtype == np.float64 and out['pcs'].shape == (Tp, k)
    eofs = out['eofs'][key]
    assert eofs.dtype == np.float64 and eofs.shape[0] == M and eofs.shape[-1] == k
    flat = eofs.reshape(M, -1, k)
    if keep is None:
        assert not np.isnan(flat).any()
    else:                                   # masked points are NaN in every lag's slice and nowhere else
        assert np.isnan(flat[:, ~keep, :]).all() and not np.isnan(flat[:, keep, :]).any()
        flat = flat[:, keep, :]
    res = dict(out, eofs=flat)
    err = C.errors(res, ref)
    err["unit_norm"] = float(np.max(np.abs(np.sum(flat ** 2, axis=(0, 1)) - 1.0)))
    err["unit_variance"] = float(np.max(np.abs(out['pcs'].var(axis=0, ddof=1) - 1.0)))
    gram = out['pcs'].T @ out['pcs'] / (Tp - 1)
    err["pc_orthogonality"] = float(np.max(np.abs(gram - np.diag(np.diag(gram)))))
    WORST[name + "_" + np.dtype(dtype).name] = err
    print(name, np.dtype(dtype).name, err)
    assert err["eofs"] <= tol_vec and err["pcs"] <= tol_vec, err
    assert err["singular_values"] <= tol_val and err["explained_variance"] <= tol_val, err
    assert err["unit_norm"] <= tol_vec and err["unit_variance"] <= tol_vec, err
    if dtype == np.float64:
        assert err["pc_orthogonality"] <= 1e-10, err
    # the sign rule: the entry of largest magnitude of the lag-0 pattern is positive
    lag0 = flat[0]
    assert np.all(lag0[np.argmax(np.abs(lag0), axis=0), np.arange(k)] > 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", C.E2E_CASES, ids=lambda c: c[0])
def test_extended_eofs_match_the_svd_of_the_embedded_matrix(hip, case, dtype):
    name, T, N, M, tau, k, seed = case
    X = C.case_field(T, N, seed).astype(dtype)
    X64 = X.astype(np.float64)
    ref = C.svd_truth(X64 - X64.mean(axis=0), M, tau, k)
    m = MCA(X.copy(), handle=hip)
    out = m.extended_eofs(M, tau=tau, n_modes=k)                       # no solve() before it
    _check_against_truth(name, out, ref, 'left', M, k, T - (M - 1) * tau, dtype)
    again = m.extended_eofs(M, tau=tau, n_modes=k)
    for key in ('singular_values', 'explained_variance', 'pcs'):
        assert np.array_equal(out[key], again[key])
    assert np.array_equal(out['eofs']['left'], again['eofs']['left'])


def test_a_window_count_past_the_tridiagonal_threshold(hip):
    """T' = 799: the eigensolver reduces to tridiagonal form and forms the leading vectors only (solve(n_modes=k)'s route)"""
    name, T, N, M, tau, k, seed = C.LARGE_CASE
    X = C.case_field(T, N, seed)
    ref = C.svd_truth(X, M, tau, k)
    out = MCA(X.copy(), handle=hip).extended_eofs(M, tau=tau, n_modes=k)
    _check_against_truth(name, out, ref, 'left', M, k, T - (M - 1) * tau, np.float64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_masked_three_dimensional_field(hip, dtype):
    name, T, shape, masked, M, tau, k, seed = C.MASKED_CASE
    full, X, keep = C.masked_field(T, shape, masked, seed)
    X64 = X.astype(dtype).astype(np.float64)
    ref = C.svd_truth(X64 - X64.mean(axis=0), M, tau, k)
    out = MCA(full.astype(dtype), handle=hip).extended_eofs(M, tau=tau, n_modes=k)
    assert out['eofs']['left'].shape == (M,) + tuple(shape) + (k,)
    _check_against_truth(name, out, ref, 'left', M, k, T - (M - 1) * tau, dtype, keep=keep)


@pytest.mark.parametrize("preprocess", ["device", "host"])
def test_normalised_model_embeds_the_field_solve_sees(hip, preprocess):
    """normalize() before the call: the truth is that of the standardised field"""
    name, T, N, M, tau, k, seed = C.E2E_CASES[1]
    X = C.case_field(T, N, seed) * np.linspace(0.5, 3.0, N)
    m = MCA(X.copy(), handle=hip, preprocess=preprocess)
    m.normalize()
    ref = C.svd_truth(X / X.std(axis=0), M, tau, k)
    out = m.extended_eofs(M, tau=tau, n_modes=k)
    err = C.errors(dict(out, eofs=out['eofs']['left']), ref)
    assert err["eofs"] <= 1e-5 and err["pcs"] <= 1e-5 and err["singular_values"] <= 1e-10, err


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(40, 23), (30, 130)], ids=["40x23", "30x130"])
def test_an_embedding_of_one_is_solve(hip, shape, dtype):
    k = 3
    tol_vec, tol_val = TOL[dtype]
    m = MCA(C.case_field(shape[0], shape[1], 0).astype(dtype), handle=hip)
    m.solve()
    sv, eofs, pcs = m.singular_values(k), m.eofs(k)['left'], m.pcs(k)['left']
    out = m.extended_eofs(1, n_modes=k)
    assert np.max(np.abs(out['singular_values'] / sv - 1)) <= tol_val
    assert np.max(np.abs(out['explained_variance'] / m.explained_variance(k) - 1)) <= tol_val
    e = out['eofs']['left']
    assert e.shape == (1,) + eofs.shape
    sign = np.where(np.sum(e[0] * eofs, axis=0) < 0, -1.0, 1.0)
    assert np.max(np.abs(e[0] * sign - eofs)) <= tol_vec
    assert np.max(np.abs(out['pcs'] * sign - pcs)) <= tol_vec


def test_a_solved_and_rotated_model_keeps_its_result_to_the_bit(hip):
    name, T, N, M, tau, k, seed = C.E2E_CASES[2]
    m = MCA(C.case_field(T, N, seed), handle=hip)
    m.solve()
    m.rotate(3)
    before = (m.singular_values().copy(), m.eofs(3)['left'].copy(), m.pcs(3)['left'].copy())
    first = m.extended_eofs(M, tau=tau, n_modes=k)
    after = (m.singular_values(), m.eofs(3)['left'], m.pcs(3)['left'])
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    second = m.extended_eofs(M, tau=tau, n_modes=k)
    assert np.array_equal(first['pcs'], second['pcs']) and np.array_equal(first['eofs']['left'], second['eofs']['left'])
    assert np.array_equal(first['singular_values'], second['singular_values'])
    # a refused call leaves the handle usable
    with pytest.raises(ValueError):
        m.extended_eofs(M, tau=tau, n_modes=T)
    with pytest.raises(ValueError):
        hip.extended_eofs(T, N, M, tau, T)
    third = m.extended_eofs(M, tau=tau, n_modes=k)
    assert np.array_equal(first['pcs'], third['pcs'])
    for a, b in zip(before, (m.singular_values(), m.eofs(3)['left'], m.pcs(3)['left'])):
        assert np.array_equal(a, b)
    assert {"lag_gram", "eeof_eigh", "eeof_project", "eeof_assemble"} <= set(hip.timings())


def test_a_model_that_lost_the_handle_uploads_its_field_again(hip):
    name, T, N, M, tau, k, seed = C.E2E_CASES[0]
    a = MCA(C.case_field(T, N, seed), handle=hip)
    first = a.extended_eofs(M, tau=tau, n_modes=k)
    b = MCA(C.case_field(T + 3, N + 2, seed + 1), handle=hip)          # takes over the resident field
    b.solve()
    second = a.extended_eofs(M, tau=tau, n_modes=k)
    # (the field is centred again on the host before it goes up: the same field to rounding, not to the bit)
    assert np.max(np.abs(first['pcs'] - second['pcs'])) <= 1e-10
    assert np.max(np.abs(first['eofs']['left'] - second['eofs']['left'])) <= 1e-10
    assert np.max(np.abs(first['singular_values'] / second['singular_values'] - 1)) <= 1e-12


def test_facade_on_a_lat_lon_field(hip):
    try:
        import xarray as xr
    except Exception:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
        import xarray as xr
    from xmca_amd.xarray import xMCA
    name, T, shape, masked, M, tau, k, seed = C.MASKED_CASE
    full, X, keep = C.masked_field(T, shape, masked, seed)
    time, lat, lon = np.arange(T) * 10, np.linspace(-20, 20, shape[0]), np.linspace(0, 50, shape[1])
    da = xr.DataArray(full, dims=['time', 'lat', 'lon'], coords={'time': time, 'lat': lat, 'lon': lon})
    xm = xMCA(da)
    xm._handle_override = hip
    out = xm.extended_eofs(M, tau=tau, n_modes=k)
    Tp = T - (M - 1) * tau
    e, p = out['eofs']['left'], out['pcs']
    assert list(e.dims) == ['lag', 'lat', 'lon', 'mode'] and e.values.shape == (M,) + tuple(shape) + (k,)
    assert np.array_equal(np.asarray(e.coords['lag']), np.arange(M) * tau)
    assert list(p.dims) == ['time', 'mode'] and np.array_equal(np.asarray(p.coords['time']), time[:Tp])
    ref = C.svd_truth(X - X.mean(axis=0), M, tau, k)
    res = {'pcs': p.values, 'eofs': e.values.reshape(M, -1, k)[:, keep, :], 'singular_values': out['singular_values'],
           'explained_variance': out['explained_variance']}
    err = C.errors(res, ref)
    assert err["eofs"] <= 1e-5 and err["pcs"] <= 1e-5 and err["singular_values"] <= 1e-10, err


def test_zz_write_accuracy_record():
    """(last in the file) the worst errors of the end-to-end cases, for profiles/extended_eofs_accuracy.json"""
    path = os.environ.get("XMCA_EXTENDED_EOFS_ACCURACY")
    if path and WORST:
        with open(path, "w") as f:
            json.dump({"tolerances": {"float64": TOL[np.float64], "float32": TOL[np.float32]}, "worst_errors": WORST}, f, indent=1,
                      sort_keys=True)
