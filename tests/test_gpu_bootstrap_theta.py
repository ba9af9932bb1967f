"""`bootstrapping()` of a model solved with extend='theta' on the device (xmca_bootstrap_runs_theta,
xmca_bootstrap_runs_columns_theta; the Theta branch of the replicate runner): every replicate is gathered, centred,
fitted again by the kernels of csrc/theta.h and complexified as X_im = G0 X + B C on its lane.

1. against the restatement: the reference's loop on the same draws - cumulative `block_bootstrap`, re-centring, the numpy
   restatement of the extension (tests/theta_cases.py) and the numpy oracle solve (oracle/ref_numpy.py) - at the bound
   tests/test_gpu_extend_exp.py sets for device results against that oracle (its TOL, 1e-5 of the largest value).  Every
   restated replicate must meet the suite's condition on its columns (`first_round_gap >= MIN_GAP`): an input whose alpha hinges
   on rounding fails there instead of loosening the bound;
2. against the kept host loop (`_bootstrap_on_host`), at the bound of the row and column bootstrap tests for float64 replicates
   (tests/test_gpu_bootstrap_columns.py `_tol`: 1e-8 of the largest value);
3. the proof that the device route is taken;
4. the edges of the fit kernels' workgroups and of T against the season, through the C ABI with hand-made indices;
5. refusals before anything is launched;
6. independence from the number of lanes (a lane owns its fit buffers);
7. strategy='iterative'.

Resampling with replacement makes replicates rank deficient: every comparison is absolute, in units of the largest value."""
import os
import subprocess
import sys

import numpy as np
import pytest

import theta_cases as tc
from oracle import ref_numpy
from xmca_amd import _hip
from xmca_amd.array import MCA
from xmca_amd.tools.array import block_bootstrap

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5                 # device results against the numpy oracle (tests/test_gpu_extend_exp.py TOL)
TOL_HOST_LOOP = 1e-8       # float64 device replicates against the host loop (tests/test_gpu_bootstrap_columns.py _tol)
T_CLS = 25
N_RUNS, N_MODES = 5, 4


def _class_fields(two):
    """The fields of tests/test_gpu_theta_extension.py: 130 and 65 grid points, the constant ones left out."""
    left = tc.columns(T_CLS, 156, 4, seed=31)[:, np.arange(156) % 6 != 4] + 3.0
    right = tc.columns(T_CLS, 78, 4, seed=32)[:, np.arange(78) % 6 != 4] * 2.0 - 1.0
    assert left.shape == (T_CLS, 130) and right.shape == (T_CLS, 65)
    return (left, right) if two else (left,)


# tag, two fields, period, rotation, bootstrapping kwargs
CASES = [
    ("m1_b1", False, 1, None, dict(axis=0, on_left=True, block_size=1)),
    ("m4_b5", False, 4, None, dict(axis=0, on_left=True, block_size=5)),
    ("m12_b1", False, 12, None, dict(axis=0, on_left=True, block_size=1)),
    ("two_rot_b1", True, 4, (4, 1), dict(axis=0, on_left=True, on_right=True, block_size=1)),
    ("two_columns_b5", True, 4, None, dict(axis=1, on_left=True, on_right=True, block_size=5)),
]
IDS = [c[0] for c in CASES]


def _model(two, m, rot):
    model = MCA(*_class_fields(two))
    model.solve(complexify=True, extend='theta', period=m)
    if rot:
        model.rotate(*rot)
    return model


def _bootstrap(model, kw, host=False, n_runs=N_RUNS, n_modes=N_MODES):
    model._bootstrap_on_host = host
    np.random.seed(5)
    return model.bootstrapping(n_runs, n_modes=n_modes, **kw)


def _err(got, want):
    """largest difference in units of the largest value"""
    return float(np.max(np.abs(got - want)) / np.abs(want).max())


@pytest.fixture(scope="module")
def device_results():
    """bootstrapping(5, n_modes=4) of every case on the device route, computed once for the tests below"""
    return {tag: _bootstrap(_model(two, m, rot), kw) for tag, two, m, rot, kw in CASES}


def _restated_signals(fields, m):
    """Re-centred replicate fields -> their restated analytic signals and the smallest first-round gap of their fits"""
    signals, gap = [], np.inf
    for x in fields:
        xc = x - x.mean(axis=0)
        pair = tc.fits(xc, m)
        gap = min([gap] + [tc.first_round_gap(f["first_round"]) for f in pair])
        signals.append(tc.analytic_signal(xc, m, pair))
    return signals, gap


def _restated_spectrum(fields, m, rot, n):
    signals, gap = _restated_signals(fields, m)
    ref = ref_numpy.solve(signals)
    if rot is None:
        return ref["singular_values"][:n], gap
    r = ref_numpy.rotate(ref["V"], ref["singular_values"], *rot)
    return r["variance"][r["var_idx"]][:n], gap


def _reference_loop(two, m, rot, kw):
    """The reference's loop (xmca/array.py:1935-1947) on the draws of np.random.seed(5): (spectra n_modes x n_runs, smallest gap)"""
    X = [ref_numpy.flatten_and_center(f)[0] for f in _class_fields(two)]
    n_left = X[0].shape[1]
    draw = dict(axis=kw["axis"], block_size=kw["block_size"], replace=True)
    np.random.seed(5)
    want, gaps = np.zeros((N_MODES, N_RUNS)), []
    for run in range(N_RUNS):
        if two:
            both = block_bootstrap(np.concatenate(X, axis=1), **draw)
            X = [both[:, :n_left], both[:, n_left:]]
        else:
            X = [block_bootstrap(X[0], **draw)]
        want[:, run], gap = _restated_spectrum(X, m, rot, N_MODES)
        gaps.append(gap)
    return want, min(gaps)


# ----------------------------------------------------------------------------------------------
# 1. the restatement
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,two,m,rot,kw", CASES, ids=IDS)
def test_theta_replicates_match_the_restated_reference_loop(tag, two, m, rot, kw, device_results):
    want, gap = _reference_loop(two, m, rot, kw)
    got = device_results[tag]
    assert got.shape == want.shape == (N_MODES, N_RUNS)
    print(tag, "smallest first-round gap %.3g; max |device - restatement| / max = %.3e" % (gap, _err(got, want)))
    assert gap >= tc.MIN_GAP, "a replicate's alpha hinges on rounding: first-round gap %g" % gap
    assert np.all(want[0] > 0)
    assert _err(got, want) < TOL


# ----------------------------------------------------------------------------------------------
# 2. the kept host loop
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,two,m,rot,kw", CASES, ids=IDS)
def test_theta_replicates_equal_the_host_loop(tag, two, m, rot, kw, device_results):
    host = _bootstrap(_model(two, m, rot), kw, host=True)
    got = device_results[tag]
    assert got.shape == host.shape
    print(tag, "max |device - host loop| / max |host loop| = %.3e" % _err(got, host))
    assert _err(got, host) < TOL_HOST_LOOP


# ----------------------------------------------------------------------------------------------
# 3. the device route is taken
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
def test_theta_bootstrapping_builds_no_model_per_replicate(monkeypatch, axis):
    model = _model(True, 4, None)
    dev = model._device()
    made = []
    init = MCA.__init__

    def counting(self, *a, **k):
        made.append(1)
        return init(self, *a, **k)
    monkeypatch.setattr(MCA, "__init__", counting)
    dev.reset_timings()
    np.random.seed(1)
    out = model.bootstrapping(3, n_modes=4, axis=axis, on_left=True, on_right=True, block_size=5)
    assert out.shape == (4, 3) and np.all(out[0] > 0)
    stages = dev.timings()
    assert "resample" in stages and "theta_fit" in stages, sorted(stages)
    assert not made, "bootstrapping of a theta model built %d MCA models" % len(made)


# ----------------------------------------------------------------------------------------------
# 4. edges through the ABI: hand-made indices, no RNG
# ----------------------------------------------------------------------------------------------
def _row_patterns(T):
    t = np.arange(T)
    return np.stack([t, t[::-1].copy(), (3 * t + 1) % T, (2 * (t // 2)) % T])     # identity, reversed, scattered, duplicated rows


@pytest.mark.parametrize("N", [1, 63, 65, 130])
@pytest.mark.parametrize("T,m", [(8, 4), (9, 4), (9, 1), (24, 12)])
def test_fit_edges_through_the_abi(hip, T, m, N):
    """T = 2m, 2m + 1, no season and the longest season; N around the smoothing kernel's 64 columns and below the season
    kernel's 256."""
    X = np.ascontiguousarray(tc.columns(T, 130, m, seed=100 * m + T)[:, :N])
    idx = _row_patterns(T)
    rank = min(T, N)
    hip.set_field(0, X)
    hip.bootstrap_begin(1)
    spectra, kept = hip.bootstrap_runs(T, True, idx, None, len(idx), False, 0, 1, 1e-8, rank, theta_period=m)
    assert spectra.shape == (len(idx), rank) and kept.all() and np.isfinite(spectra).all()
    for run in range(len(idx)):
        want, gap = _restated_spectrum([X[idx[run]]], m, None, rank)
        err = np.max(np.abs(spectra[run] - want)) / want[0]
        print("T = %d m = %d N = %d pattern %d: gap %.3g, |device - restatement| = %.3e sigma_1" % (T, m, N, run, gap, err))
        assert err < TOL, (run, spectra[run], want)
    # the identity replicate is the model itself
    hip.complexify_theta(T, m)
    hip.solve(1)
    s = hip.singular_values(rank)
    assert np.max(np.abs(spectra[0] - s)) < TOL_HOST_LOOP * s[0]
    # reversal swaps forecast and backcast (a crossed blockIdx.y, or a B with its halves swapped, shows here)
    assert np.max(np.abs(spectra[1] - spectra[0])) < TOL_HOST_LOOP * spectra[0][0]


def test_column_indices_through_the_abi(hip):
    """Two fields of 65 and 1 columns, the left replicate entirely from the right field and the right one from the left"""
    T, m, n_l, n_r = 9, 4, 65, 1
    fields = [np.ascontiguousarray(tc.columns(T, 130, m, seed=100 * m + T)[:, :n_l]),
              np.ascontiguousarray(tc.columns(T, 6, m, seed=100 * m + T + 1)[:, 3:4])]
    ident = np.arange(n_l + n_r)
    swap = np.concatenate([n_l + np.arange(n_l) % n_r, np.arange(n_r) % n_l])
    pats = [ident, swap]
    cl, cr = np.stack([p[:n_l] for p in pats]), np.stack([p[n_l:] for p in pats])
    for side, f in enumerate(fields):
        hip.set_field(side, f)
    hip.bootstrap_begin(2)
    spectra, kept = hip.bootstrap_runs(T, True, cl, cr, len(pats), False, 0, 1, 1e-8, 1, theta_period=m, axis=1)
    assert spectra.shape == (len(pats), 1) and kept.all()
    concat = np.concatenate(fields, axis=1)
    for run in range(len(pats)):
        want, gap = _restated_spectrum([concat[:, cl[run]], concat[:, cr[run]]], m, None, 1)
        err = abs(spectra[run, 0] - want[0]) / want[0]
        print("columns pattern %d: gap %.3g, |device - restatement| = %.3e sigma_1" % (run, gap, err))
        assert err < TOL


# ----------------------------------------------------------------------------------------------
# 5. refusals, before anything is launched
# ----------------------------------------------------------------------------------------------
def _call_abi(hip, name, parts, period, idx, n_out):
    col3, hbar, B = parts
    out, kept = np.zeros((1, n_out)), np.zeros(1, dtype=np.int32)
    return getattr(hip._lib, name)(hip._h, _hip._ptr(col3), _hip._ptr(hbar), _hip._ptr(B), period, _hip._ptr(idx), None, 1, 0, 0, 1, 1e-8,
                                   _hip._ptr(out), _hip._ptr(kept), n_out)


def test_refusals_launch_nothing(hip):
    T, N, m = 9, 5, 4
    X = np.ascontiguousarray(tc.columns(T, N, m, seed=1))
    rows = np.arange(T, dtype=np.int64)[None].copy()
    cols = np.arange(N, dtype=np.int64)[None].copy()
    parts = _hip.theta_imag_parts(T, m)
    hip.set_field(0, X)
    hip.bootstrap_begin(1)
    hip.reset_timings()
    for period in (0, 5):                              # no season length; T < 2 period
        assert _call_abi(hip, "xmca_bootstrap_runs_theta", parts, period, rows, N) == _hip.ERR_INVALID
        assert _call_abi(hip, "xmca_bootstrap_runs_columns_theta", parts, period, cols, N) == _hip.ERR_INVALID
    bad = rows.copy()
    bad[0, -1] = T
    with pytest.raises(ValueError, match="row index out of range"):
        hip.bootstrap_runs(T, True, bad, None, 1, False, 0, 1, 1e-8, N, theta_period=m)
    with pytest.raises(ValueError):
        hip.bootstrap_runs(T, True, rows, None, 1, False, 0, 1, 1e-8, N, extend_period=3.0, theta_period=m)
    assert "resample" not in hip.timings()
    # float32 working copies
    hip.set_field(0, X.astype(np.float32))
    hip.bootstrap_begin(1)
    hip.reset_timings()
    for axis, idx in ((0, rows), (1, cols)):
        with pytest.raises(ValueError, match="needs float64 fields"):
            hip.bootstrap_runs(T, True, idx, None, 1, False, 0, 1, 1e-8, N, theta_period=m, axis=axis)
    assert "resample" not in hip.timings()
    # no xmca_bootstrap_begin
    fresh = _hip.Handle(0)
    try:
        fresh.set_field(0, X)
        with pytest.raises(_hip.HipError, match="xmca_bootstrap_begin") as info:
            fresh.bootstrap_runs(T, True, rows, None, 1, False, 0, 1, 1e-8, N, theta_period=m)
        assert info.value.code == _hip.ERR_STATE
        assert "resample" not in fresh.timings()
    finally:
        fresh.close()


# ----------------------------------------------------------------------------------------------
# 6. lanes
# ----------------------------------------------------------------------------------------------
def test_theta_replicates_do_not_depend_on_the_number_of_lanes(tmp_path):
    """A lane owns its operator, its B and its fit buffers (the season kernel accumulates in the fit buffer: two lanes writing one
    would race): one lane (XMCA_RULE_N_LANES=1, read once per process, hence the child) and the default give the same bits."""
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r);"
            "import theta_cases as tc; from xmca_amd.array import MCA;"
            "left = tc.columns(25, 156, 4, seed=31)[:, np.arange(156) %% 6 != 4] + 3.0;"
            "m = MCA(left); m.solve(complexify=True, extend='theta', period=4); m.rotate(4, 1); np.random.seed(5);"
            "np.save(sys.argv[1], m.bootstrapping(5, n_modes=4, on_left=True, block_size=5))"
            % (REPO, os.path.join(REPO, "tests")))
    outs = []
    for lanes in ("1", None):
        env = dict(os.environ)
        env.pop("XMCA_RULE_N_LANES", None)
        if lanes:
            env["XMCA_RULE_N_LANES"] = lanes
        dst = str(tmp_path / ("lanes_%s.npy" % lanes))
        r = subprocess.run([sys.executable, "-c", code, dst], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(dst))
    assert outs[0].shape == (4, 5) and np.all(outs[0] > 0)
    assert np.array_equal(outs[0], outs[1])


# ----------------------------------------------------------------------------------------------
# 7. strategy='iterative'
# ----------------------------------------------------------------------------------------------
def test_iterative_strategy_equals_the_host_loop():
    kw = dict(axis=0, on_left=True, block_size=1, strategy='iterative')
    got = _bootstrap(_model(False, 4, None), kw, n_runs=3, n_modes=2)
    host = _bootstrap(_model(False, 4, None), kw, host=True, n_runs=3, n_modes=2)
    assert got.shape == host.shape == (2, 3)
    print("iterative: max |device - host loop| / max |host loop| = %.3e" % _err(got, host))
    assert _err(got, host) < TOL_HOST_LOOP
