"""GPU: the p-value kernel (xmca_pearson_pvalues) against an mpmath truth and scipy, xmca_correlation_maps against xmca_correlate,
and homogeneous_patterns / heterogeneous_patterns on the device route against the host route (`_patterns_on_host`).

Accuracy contract of the kernel: p = 2 exp(L) / cf with L a sum of terms of magnitude up to a |ln(x (1 - x))| (the log-normaliser has
the same magnitude and the opposite sign), each good to a few ulp, and the relative error of exp(L) is the absolute error of L:

    |p - truth| <= 64 * 2^-52 * (1 + a |ln(x (1 - x))|) * truth,        a = n_obs / 2 - 1, x = (1 - |r|) / 2

on every point of the main group of tests/golden/pvalue_truth.npz (truth >= 1e-290; scripts/make_pvalue_goldens.py).  Against
scipy (`_two_sided_p`) the same bound plus scipy's own measured error: 1e-12 relative where p_ref >= 1e-250, 1e-8 relative
between 1e-290 and 1e-250 (scipy is off by up to 2.1e-9 there against the truth), absolute 1e-289 below.
The worst error / bound per n_obs is printed by the tests; profiles/patterns_accuracy.json records the MI355X figures."""
import json
import os

import numpy as np
import pytest

from golden_inputs import GOLDEN_DIR, make_input
from xmca_amd.array import MCA, _two_sided_p

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def _bound(r, n_obs, p):
    a = n_obs / 2 - 1
    x = (1.0 - np.abs(r)) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return 64 * EPS * (1 + a * np.abs(np.log(x) + np.log1p(-x))) * p


def _check_against_scipy(p, r, n_obs, what):
    """p (device) against `_two_sided_p(r, n_obs)`; returns the worst error / allowance over the values above 1e-290"""
    ref = _two_sided_p(r, n_obs)
    assert np.array_equal(np.isnan(p), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    p, ref, r = p[ok], ref[ok], np.asarray(r, dtype=np.float64)[ok]
    assert np.all((p >= 0) & (p <= 1)), what
    low = ref < 1e-290
    assert np.all(np.abs(p[low] - ref[low]) <= 1e-289), what
    p, ref, r = p[~low], ref[~low], r[~low]
    allow = _bound(r, n_obs, ref) + np.where(ref >= 1e-250, 1e-12, 1e-8) * ref
    ratio = np.abs(p - ref) / allow
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, (what, worst, r[np.argmax(ratio)])
    return worst


def test_pvalue_kernel_against_truth(hip):
    g = np.load(os.path.join(GOLDEN_DIR, "pvalue_truth.npz"))
    report = {}
    for n_obs in np.unique(g["n_obs"]):
        sel = g["n_obs"] == n_obs
        r, truth = g["r"][sel], g["p"][sel]
        assert np.all(truth >= 1e-290)
        p = hip.pearson_pvalues(r, int(n_obs))
        ratio = np.abs(p - truth) / _bound(r, n_obs, truth)
        report[int(n_obs)] = {"points": int(sel.sum()), "worst_rel_error": float(np.max(np.abs(p - truth) / truth)),
                              "worst_error_over_bound": float(ratio.max())}
        print("n_obs %5d: %3d points, worst relative error %.3g, worst error / bound %.3g"
              % (n_obs, sel.sum(), report[int(n_obs)]["worst_rel_error"], ratio.max()))
    print("pvalue accuracy " + json.dumps(report))
    for n_obs, rep in report.items():                    # every point of the main group, no exception
        assert rep["worst_error_over_bound"] <= 1.0, (n_obs, rep)
    for n_obs in np.unique(g["tail_n_obs"]):
        sel = g["tail_n_obs"] == n_obs
        p = hip.pearson_pvalues(g["tail_r"][sel], int(n_obs))
        assert np.all(np.isfinite(p)) and np.all((p >= 0) & (p <= 1e-289)), n_obs


@pytest.mark.parametrize("n_obs", [3, 4, 10, 61, 1200, 2920])
def test_pvalue_kernel_against_scipy(hip, n_obs):
    rng = np.random.default_rng(1000 + n_obs)
    r = np.concatenate([rng.uniform(-1, 1, 150_000), rng.uniform(-1, 1, 25_000) * 10.0 ** -rng.uniform(0, 12, 25_000),
                        np.sign(rng.uniform(-1, 1, 25_000)) * (1 - 10.0 ** -rng.uniform(0, 15, 25_000))])
    assert r.size == 200_000
    p = hip.pearson_pvalues(r, n_obs)
    worst = _check_against_scipy(p, r, n_obs, n_obs)
    print("n_obs %5d: worst error / (bound + scipy's error) %.3g" % (n_obs, worst))


@pytest.mark.parametrize("n_obs", [3, 4, 50, 2920])
def test_pvalue_kernel_edge_values(hip, n_obs):
    r = np.array([1.0, -1.0, 1 + 2.0 ** -52, -1 - 2.0 ** -52, 0.0, -0.0, np.nan, 5e-324, 1 - 2.0 ** -53])
    p = hip.pearson_pvalues(r, n_obs)
    assert np.array_equal(p[:4], [0.0, 0.0, 0.0, 0.0])
    assert np.isnan(p[6]) and not np.any(np.isinf(p))
    for i in (4, 5, 7):                                   # p(0) = 1
        assert p[i] <= 1.0 and 1.0 - p[i] <= _bound(0.0, n_obs, 1.0), (i, p[i])
    assert 0.0 <= p[8] <= 1.0
    assert _check_against_scipy(p, r, n_obs, "edge") <= 1.0


def test_pvalue_kernel_grid_stride(hip):
    rng = np.random.default_rng(5)
    r = rng.uniform(-1, 1, 2_200_000)               # more values than one pass of the largest grid has lanes
    whole = hip.pearson_pvalues(r, 300)
    parts = np.concatenate([hip.pearson_pvalues(r[i:i + 1000], 300) for i in range(0, r.size, 1000)])
    assert np.array_equal(whole, parts)
    assert hip.pearson_pvalues(np.zeros(0), 300).shape == (0,)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", [3, 4, 61, 500])
@pytest.mark.parametrize("masked", [False, True])
def test_correlation_maps_entry_matches_correlate(hip, dtype, T, masked):
    rng = np.random.default_rng(T)
    N, m = 777, 5
    X = rng.standard_normal((T, N)).astype(dtype)
    X[:, 11] = 2.5                                   # a constant column: NaN in both maps
    X -= X.mean(axis=0)
    Y = X[:, :m].astype(np.float64) + 0.5 * rng.standard_normal((T, m))
    Y[:, 0] = X[:, 0]                                # a perfectly correlated pair
    N_full = N + 40 if masked else N
    keep_idx = np.sort(rng.choice(N_full, N, replace=False)) if masked else None
    hip.set_field(0, X)
    want = hip.correlate(0, Y, N)
    for r_dtype in (np.float32, np.float64):
        r, p = hip.correlation_maps(0, Y, keep_idx, N_full, r_dtype)
        assert r.shape == p.shape == (N_full, m) and r.dtype == r_dtype and p.dtype == np.float64
        rows = np.arange(N) if keep_idx is None else keep_idx
        assert np.array_equal(r[rows], want.astype(r_dtype), equal_nan=True)
        assert np.isnan(r[rows[11]]).all() and np.isnan(p[rows[11]]).all()
        gone = np.setdiff1d(np.arange(N_full), rows)
        assert np.isnan(r[gone]).all() and np.isnan(p[gone]).all()
        assert np.isfinite(np.delete(r[rows], 11, axis=0)).all()
        assert np.array_equal(p, hip.pearson_pvalues(r, T), equal_nan=True)
        assert abs(r[rows[0], 0] - 1) < 1e-5
    assert np.array_equal(hip.correlate(0, Y, N), want, equal_nan=True)            # xmca_correlate itself is as it was


_HANDLES = []


def _two_models(fields, cplx, rot):
    """the same model twice, device route and host route, each on a handle of its own (neither evicts the other's result)"""
    from xmca_amd import _hip
    while len(_HANDLES) < 2:
        _HANDLES.append(_hip.Handle(0))
    out = []
    for on_host, handle in zip((False, True), _HANDLES):
        m = MCA(*fields, handle=handle)
        m._patterns_on_host = on_host
        m.solve(complexify=cplx)
        if rot:
            m.rotate(*rot)
        out.append(m)
    return out


def _compare_routes(dev_maps, host_maps, n_obs, what):
    for d, h in zip(dev_maps, host_maps):
        assert set(d) == set(h), what
    (rd, pd), (rh, ph) = dev_maps, host_maps
    worst = 0.0
    for k in rd:
        assert rd[k].shape == rh[k].shape == pd[k].shape == ph[k].shape, (what, k)
        assert rd[k].dtype == rh[k].dtype and pd[k].dtype == ph[k].dtype == np.float64, (what, k)
        assert np.array_equal(rd[k], rh[k], equal_nan=True), (what, k)
        assert np.array_equal(np.isnan(pd[k]), np.isnan(ph[k])) and np.array_equal(np.isnan(pd[k]), np.isnan(rd[k])), (what, k)
        worst = max(worst, _check_against_scipy(pd[k].ravel(), rd[k].ravel(), n_obs, (what, k)))
        assert np.array_equal(_two_sided_p(rh[k], n_obs), ph[k], equal_nan=True), (what, k)
    return worst


@pytest.mark.parametrize("name", ["sst_prcp", "wide_both", "wide_both_f32", "wide_left"])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("rot", [None, (6, 1), (6, 4)])
def test_model_device_route_matches_host_route(name, cplx, rot):
    fields = make_input(name)
    dev, host = _two_models(fields, cplx, rot)
    n_obs = fields[0].shape[0]
    calls = [("homogeneous_patterns", dict(n=6))]
    if len(fields) == 2:
        calls.append(("heterogeneous_patterns", dict(n=6)))
    if cplx and name == "wide_both" and rot == (6, 4):
        calls += [("homogeneous_patterns", dict(n=None)), ("heterogeneous_patterns", dict(n=6, phase_shift=0.7))]
    for fn, kw in calls:
        worst = _compare_routes(getattr(dev, fn)(**kw), getattr(host, fn)(**kw), n_obs, (name, cplx, rot, fn, kw))
        print("%s %s: worst p error / allowance against the host route %.3g" % (fn, kw, worst))
    if len(fields) == 1:
        for m in (dev, host):
            with pytest.raises(KeyError, match="Two fields needed"):
                m.heterogeneous_patterns(6)


def test_patterns_do_not_call_the_host_beta_function(monkeypatch):
    import scipy.special
    dev, host = _two_models(make_input("wide_both"), False, (6, 1))

    def refuse(*args, **kwargs):
        raise AssertionError("scipy.special.betainc called")

    monkeypatch.setattr(scipy.special, "betainc", refuse)
    r, p = dev.homogeneous_patterns(6)
    assert np.isfinite(p["left"]).all() and np.isfinite(p["right"]).all()
    with pytest.raises(AssertionError, match="betainc called"):
        host.homogeneous_patterns(6)


def test_patterns_keep_the_resident_state():
    left, right = make_input("sst_prcp")
    m = MCA(left, right)
    m.solve()
    m.rotate(10, power=2)
    pcs6, eofs6, new = m.pcs(6), m.eofs(6), m.predict(left[:20], right[:20])
    dev = m._device()
    owner = dev.fields_owner
    m.homogeneous_patterns(6)
    m.heterogeneous_patterns()
    dev.pearson_pvalues(np.linspace(-1, 1, 1001), 40)
    assert m._V._pending == set(m._keys)
    assert dev.holds_result_of(m)
    assert dev.fields_owner == owner
    again = m.predict(left[:20], right[:20])
    for k in m._keys:
        assert np.array_equal(m.pcs(6)[k], pcs6[k])
        assert np.array_equal(m.eofs(6)[k], eofs6[k], equal_nan=True)
        assert np.array_equal(again[k], new[k])


def test_short_series_takes_the_host_route(hip):
    """two observations: a = n_obs / 2 - 1 = 0, no null distribution; the class keeps the host function (every p NaN)"""
    rng = np.random.default_rng(2)
    X = rng.standard_normal((2, 12))
    X[:, 5] = np.nan
    maps = []
    for on_host in (False, True):
        m = MCA(X, handle=hip)
        m._patterns_on_host = on_host
        m._get_pcs = lambda n=None, phase_shift=0: {"left": np.array([[1.0], [-1.0]])}      # (state injected: no solve of 2 rows)
        with np.errstate(invalid="ignore", divide="ignore"):
            maps.append(m.homogeneous_patterns(1))
    (rd, pd), (rh, ph) = maps
    assert rd["left"].shape == pd["left"].shape == (12, 1) and pd["left"].dtype == np.float64
    assert np.array_equal(rd["left"], rh["left"], equal_nan=True) and np.array_equal(pd["left"], ph["left"], equal_nan=True)
    assert np.isnan(pd["left"]).all() and np.isnan(rd["left"][5]).all()
    for n_obs in (2, 1, 0, -3):
        with pytest.raises(ValueError, match="n_obs >= 3"):
            hip.pearson_pvalues(np.array([0.5, -0.25]), n_obs)
    with pytest.raises(NotImplementedError):
        hip.pearson_pvalues(np.array([0.5]), 1_000_001)
