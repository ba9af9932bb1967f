"""GPU: `MCA.bootstrap_eofs` - bootstrap mean and standard error of the leading singular vectors, accumulated on
the device (csrc/boot_patterns.h).  Twin and cases: tests/bootstrap_patterns_cases.py.

  * the statistics alone through `Handle.pattern_stats` (given replicate vectors, no eigensolver) against the twin, to a
    rounding bound derived below, for every lane count, and the same bits on a second call;
  * end to end through `MCA.bootstrap_eofs(indices=...)` against the twin (numpy SVD per replicate) at the vector tolerances of
    tests/test_gpu_configs.py: 1e-5 for float64 models, 1e-3 for float32 ones; the replicates' singular values against
    `Handle.bootstrap_runs` fed the same indices;
  * the xarray facade, and the refused calls, after which the handle still solves as before.

The worst measured errors of the end-to-end cases go to the file named by XMCA_BOOTSTRAP_PATTERNS_ACCURACY when that is set
(profiles/bootstrap_patterns_accuracy.json holds the MI355X figures)."""
import json
import os
import sys

import numpy as np
import pytest

import bootstrap_patterns_cases as B
from xmca_amd import _hip
from xmca_amd.array import MCA, bootstrap_row_indices

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53            # unit roundoff of float64
R_STATS = 5
# Bounds of the kernel test, for R = 5 replicates; see test_statistics_match_the_twin_to_rounding
BOUND_G = 52 * EPS
BOUND_MEAN = 26 * R_STATS * EPS
BOUND_VAR = 250 * R_STATS * EPS

WORST = {}


def _tile_sizes():
    t = _hip.pattern_tile()
    return [1, 63, 64, 65, 257, t - 1, t, t + 1, 2 * t + 3]


def _round_planes(reps, dtype):
    """the replicate planes as the device holds them: re and im rounded to `dtype`, then float64 again"""
    if dtype == np.float64:
        return reps
    def rd(v):
        if np.iscomplexobj(v):
            return v.real.astype(np.float32).astype(np.float64) + 1j * v.imag.astype(np.float32).astype(np.float64)
        return v.astype(np.float32).astype(np.float64)
    return [[rd(v) for v in rep] for rep in reps]


@pytest.mark.parametrize("plane", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("n_index", range(9))
def test_statistics_match_the_twin_to_rounding(hip, n_index, two, cplx, plane):
    """Device and twin get the same numbers - v0, and replicate planes already rounded to the plane dtype - so they differ by the
    rounding of float64 sums alone.  e = 2^-53; unit vectors, so sum_n |v0| |v| <= 1 per side and |d| <= 2; R = 5 runs; every run
    but the exactly orthogonal one has |c| >= n_fields / 2 (asserted on the twin), where u is well conditioned.
      c:  a sum in any order errs by at most (roundings a term passes through) e sum|terms|.  Device: a tile is 4 columns per
          thread, two fused steps each for a complex product (8), 6 wave steps, 3 block steps, at most 6 tiles: 23.  numpy
          pairwise: blocks of 128 in 8 partial sums (16 + 3), 5 levels above, 2 for the product: 26.  |c_dev - c_twin| <=
          50 e n_fields, so g = |c| / n_fields differs by <= 50 e + 2 e (hypot, division) = 52 e.
      u = conj(c) / |c|:  <= 50 e n_fields / (n_fields / 2) + 4 e = 104 e (real vectors: u = +-1 exactly).
      d = u v - v0:  <= 104 e |v| + 4 e (|u v| + |v0|) <= 112 e.
      S = sum_r d:  <= R 112 e + (R - 1) e sum_r |d| <= R (112 + 2 R) e;  mean = v0 + S / R:  <= (112 + 2 R) e + 3 e = 125 e < 26 R e.
      Q = sum_r |d|^2:  per term 2 |d| 112 e + 3 e |d|^2 <= 460 e, the sum adds (R - 1) e 4 R:  <= R (460 + 4 R) e.
      (R - 1) var = Q - |S|^2 / R:  |S| <= 2 R, so |S|^2 / R errs by <= 2 (2 R) R (112 + 2 R) e / R + 3 e 4 R = R (460 + 8 R) e;
          together R (920 + 12 R) e, over R - 1 = 4:  var differs by <= 245 R e < 250 R e.
    The standard error is compared as its square: sqrt has no rounding bound where the variance is zero (N = 1)."""
    N = _tile_sizes()[n_index]
    widths = (N, N + 2) if two else (N,)
    for k in (1, 3):
        rng = np.random.default_rng([n_index, two, cplx, k])
        v0, reps = B.random_replicates(rng, widths, k, R_STATS, cplx)
        reps = _round_planes(reps, plane)
        mean_t, std_t, g_t = B.pattern_stats(v0, reps)
        assert g_t[:, :-1].min() >= 0.5 and g_t[:, -1].max() == 0.0
        left = np.array([rep[0] for rep in reps])
        right = np.array([rep[1] for rep in reps]) if two else None
        first = None
        for lanes in (1, 2, 4):
            mean, std, g = hip.pattern_stats(v0[0], left, v0[1] if two else None, right, plane_dtype=plane, n_lanes=lanes)
            assert g.shape == (R_STATS, k) and np.max(np.abs(g.T - g_t)) <= BOUND_G and np.all(g[-1] == 0.0)
            for s in range(len(widths)):
                assert mean[s].shape == (widths[s], k) and np.iscomplexobj(mean[s]) == cplx and np.isrealobj(std[s])
                assert np.max(np.abs(mean[s] - mean_t[s])) <= BOUND_MEAN, (N, k, lanes, s)
                assert np.max(np.abs(std[s] ** 2 - std_t[s] ** 2)) <= BOUND_VAR, (N, k, lanes, s)
            if first is None:
                first = (mean, std, g)
        again = hip.pattern_stats(v0[0], left, v0[1] if two else None, right, plane_dtype=plane, n_lanes=1)
        for a, b in zip(first[0] + first[1] + [first[2]], again[0] + again[1] + [again[2]]):
            assert np.array_equal(a, b)                                # no atomics: a call repeats its bits


def test_pattern_stats_refuses_what_it_cannot_run(hip):
    v0 = np.ones((4, 1)) / 2.0
    with pytest.raises(ValueError):
        hip.pattern_stats(v0, np.ones((1, 4, 1)) / 2.0)                # one run: no standard error
    with pytest.raises(ValueError):
        hip.pattern_stats(v0, np.ones((3, 4, 1)) / 2.0, n_lanes=0)
    with pytest.raises(ValueError):
        hip.pattern_stats(v0, np.ones((3, 5, 1)) / 2.0)                # replicate of another width


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _e2e_cases():
    cases = []
    for i, (T, N, k, block) in enumerate(B.E2E_SHAPES):
        for cplx in (False, True):
            cases.append((T, N, k, block, cplx, np.float64, False))
            if i < 2:
                cases.append((T, N, k, block, cplx, np.float32, False))
    cases.append(B.E2E_SHAPES[0] + (False, np.float64, True))          # masked grid points
    return cases


def _case_id(c):
    T, N, k, block, cplx, dtype, masked = c
    return "T%d-N%s-k%d-b%d-%s-%s%s" % (T, "x".join(str(n) for n in np.atleast_1d(N)), k, block, "complex" if cplx else "real",
                                        np.dtype(dtype).name, "-masked" if masked else "")


def _mode_err(mine, ref):
    return float(np.max(np.max(np.abs(mine - ref), axis=0) / np.max(np.abs(ref), axis=0)))


@pytest.fixture(scope="module", autouse=True)
def _record_accuracy():
    yield
    path = os.environ.get("XMCA_BOOTSTRAP_PATTERNS_ACCURACY")
    if path and WORST:
        with open(path, "w") as fh:
            json.dump(WORST, fh, indent=1, sort_keys=True)


@pytest.mark.parametrize("case", _e2e_cases(), ids=_case_id)
def test_bootstrap_eofs_matches_the_twin(hip, case):
    T, N, k, block, cplx, dtype, masked = case
    fields = [f.astype(dtype) for f in B.case_fields(T, N, k)]
    idx = bootstrap_row_indices(B.E2E_RUNS, T, block_size=block, seed=20240611)
    t = B.twin(fields, idx, k, cplx)
    assert t['min_relgap'] >= B.MIN_RELGAP, t['min_relgap']
    given, keep = list(fields), [np.ones(f.shape[1], dtype=bool) for f in fields]
    if masked:                                                         # 70 kept points on an 8 x 10 grid
        keep[0] = np.ones(80, dtype=bool)
        keep[0][[0, 7, 13, 14, 29, 41, 55, 56, 78, 79]] = False
        full = np.full((T, 80), np.nan, dtype=dtype)
        full[:, keep[0]] = fields[0]
        given[0] = full.reshape(T, 8, 10)
    m = MCA(*given)
    m.solve(complexify=cplx)
    out = m.bootstrap_eofs(B.E2E_RUNS, k, indices=idx)
    assert sorted(out) == ['congruence', 'mean', 'singular_values', 'std']
    tol = 1e-3 if dtype == np.float32 else 1e-5
    keys = m._keys
    v0_mine = [np.asarray(m._get_V(k, rotated=False)[key], dtype=np.complex128 if cplx else np.float64) for key in keys]
    phase = B.mode_phases(v0_mine, t['v0'])
    if not cplx:
        phase = phase.real
    errs = {}
    for s, key in enumerate(keys):
        mean, std = out['mean'][key], out['std'][key]
        assert mean.shape == given[s].shape[1:] + (k,) and std.shape == mean.shape
        assert np.iscomplexobj(mean) == cplx and std.dtype == np.float64
        mean, std = mean.reshape(-1, k), std.reshape(-1, k)
        assert np.all(np.isnan(mean[~keep[s]])) and np.all(np.isnan(std[~keep[s]]))
        errs['v0_' + key] = _mode_err(v0_mine[s], t['v0'][s] * phase)
        errs['mean_' + key] = _mode_err(mean[keep[s]], t['mean'][s] * phase)
        errs['std_' + key] = _mode_err(std[keep[s]], t['std'][s])
    assert out['congruence'].shape == (k, B.E2E_RUNS) and out['singular_values'].shape == (k, B.E2E_RUNS)
    errs['congruence'] = float(np.max(np.abs(out['congruence'] - t['congruence'])))
    # the replicates' singular values: those of `bootstrap_runs` on the working copies the call left, same rows on every side
    rank = min([T] + [f.shape[1] for f in fields])
    spectra, kept = hip.bootstrap_runs(T, cplx, idx, idx if len(fields) == 2 else None, B.E2E_RUNS, False, 0, 1, 1e-8, rank)
    assert np.all(kept)
    ref = spectra[:, :k].T
    errs['sigma_vs_bootstrap_runs'] = float(np.max(np.abs(out['singular_values'] - ref) / ref))
    errs['sigma_vs_twin'] = float(np.max(np.abs(out['singular_values'] - t['singular_values']) / t['singular_values']))
    errs['min_relgap'] = t['min_relgap']
    print(_case_id(case), json.dumps(errs))
    WORST[_case_id(case)] = errs
    for name, e in errs.items():
        if name.startswith(('v0_', 'mean_', 'std_')) or name == 'congruence':
            assert e < tol, (name, e)
    assert errs['sigma_vs_bootstrap_runs'] < (2e-5 if dtype == np.float32 else 1e-10)


def test_two_calls_give_the_same_bits_and_the_seed_draws_the_indices(hip):
    T, N, k, block = B.E2E_SHAPES[1]
    m = MCA(*B.case_fields(T, N, k))
    m.solve()
    a = m.bootstrap_eofs(6, k, block_size=block, seed=4)
    b = m.bootstrap_eofs(6, k, indices=bootstrap_row_indices(6, T, block, seed=4))
    for name in ('mean', 'std'):
        for key in m._keys:
            assert np.array_equal(a[name][key], b[name][key])
    assert np.array_equal(a['congruence'], b['congruence']) and np.array_equal(a['singular_values'], b['singular_values'])
    assert np.all(a['congruence'] > 0.5) and np.all(a['congruence'] <= 1.0 + 1e-12)
    # the model still answers afterwards (its fields go up again)
    assert m.pcs(k)['left'].shape == (T, k)


def test_facade_returns_data_arrays_over_the_coordinates_of_eofs(hip):
    try:
        import xarray as xr
    except Exception:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
        import xarray as xr
    from xmca_amd.xarray import xMCA
    T, nlat, nlon, k = 36, 7, 10, 3
    lat, lon = np.linspace(-30.0, 30.0, nlat), np.linspace(0.0, 90.0, nlon)
    field = B.case_fields(T, nlat * nlon, k)[0]
    da = xr.DataArray(field.reshape(T, nlat, nlon), dims=["time", "lat", "lon"], coords={"time": np.arange(T), "lat": lat, "lon": lon})
    m = xMCA(da)
    m.solve()
    idx = bootstrap_row_indices(4, T, 3, seed=1)
    out = m.bootstrap_eofs(4, k, indices=idx)
    eofs = m.eofs(k)['left']
    plain = MCA(field.reshape(T, nlat, nlon))
    plain.solve()
    ref = plain.bootstrap_eofs(4, k, indices=idx)
    for name in ('mean', 'std'):
        a = out[name]['left']
        assert tuple(a.dims) == tuple(eofs.dims) and a.shape == (nlat, nlon, k)
        for dim in eofs.dims:
            assert np.array_equal(np.asarray(a.coords[dim].values), np.asarray(eofs.coords[dim].values))
        assert np.allclose(np.asarray(a.values), ref[name]['left'], rtol=0, atol=1e-12)
    assert isinstance(out['congruence'], np.ndarray) and out['congruence'].shape == (k, 4)
    assert isinstance(out['singular_values'], np.ndarray) and out['singular_values'].shape == (k, 4)


def test_refused_calls_leave_the_handle_usable(hip):
    T, N, k = 30, 63, 2
    field = B.case_fields(T, N, k)[0]
    m = MCA(field)
    m.solve()
    before = m.singular_values().copy()
    V0 = m._get_V(k, rotated=False)['left']
    idx = bootstrap_row_indices(4, T, 2, seed=3)
    with pytest.raises(ValueError):
        m.bootstrap_eofs(1, k)
    with pytest.raises(ValueError):
        m.bootstrap_eofs(4, T + 1)
    bad = idx.copy()
    bad[2, 5] = T
    with pytest.raises(ValueError):
        m.bootstrap_eofs(4, k, indices=bad)
    # ... and the library's own checks, before anything is launched
    hip.set_field(0, np.ascontiguousarray(field - field.mean(axis=0)))
    hip.bootstrap_begin(1)
    with pytest.raises(ValueError, match="out of range"):
        hip.bootstrap_patterns(T, False, bad, 4, k, V0)
    too_many = np.linalg.qr(np.random.default_rng(0).standard_normal((N, T + 1)))[0]
    with pytest.raises(ValueError, match="rank"):
        hip.bootstrap_patterns(T, False, idx, 4, T + 1, too_many)
    with pytest.raises(ValueError):
        hip.bootstrap_patterns(T, False, idx[:1], 1, k, V0)
    again = MCA(field)
    again.solve()
    assert np.array_equal(again.singular_values(), before)
    out = again.bootstrap_eofs(4, k, indices=idx)
    assert np.all(np.isfinite(out['std']['left'])) and np.all(out['congruence'] > 0.5)
