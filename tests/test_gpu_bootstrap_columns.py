"""`bootstrapping(axis=1)` - the column resampling - on the device (xmca_bootstrap_runs_columns*, csrc/kernels.h
gather_concat_columns_kernel): against the REAL reference's numbers under the same numpy seed
(scripts/make_bootstrap_columns_goldens.py -> tests/golden/bootstrap_columns_cases.npz), against the kept host loop, the proof that
the device path is taken, the kernel's edges through the C ABI with hand-made indices, and independence from the lanes.

Resampling columns with replacement duplicates columns, so replicates are rank deficient and the tail of a spectrum is zero up
to rounding (the reference returns about 1e-16 sigma_1 there): every comparison is absolute, in units of the largest value."""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_inputs import GOLDEN_DIR, make_input
from xmca_amd.array import MCA

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tag, input, single field, solve kwargs, rotation, bootstrapping kwargs  (scripts/make_bootstrap_columns_goldens.py holds the same list)
CASES = [
    ("small_b2", "small_both", False, dict(complexify=False), None, dict(on_left=True, on_right=True, block_size=2)),
    ("small_b3_seam", "small_both", False, dict(complexify=False), None, dict(on_left=True, on_right=True, block_size=3)),
    ("wide_rot_left", "wide_both", False, dict(complexify=False), (5, 2), dict(on_left=True, on_right=False, block_size=1)),
    ("wide_single_cplx", "wide_both", True, dict(complexify=True), None,
     dict(on_left=True, on_right=False, block_size=4, replace=False)),
    ("wide_cplx_rot_right", "wide_both", False, dict(complexify=True), (4, 1), dict(on_left=False, on_right=True, block_size=1)),
    ("mixed_b5", "mixed_both", False, dict(complexify=False), None, dict(on_left=True, on_right=True, block_size=5)),
    ("mixed_cplx_rot_both", "mixed_both", False, dict(complexify=True), (4, 1), dict(on_left=True, on_right=True, block_size=1)),
    ("wide_f32_both", "wide_both_f32", False, dict(complexify=False), None, dict(on_left=True, on_right=True, block_size=1)),
    ("wide_exp_left", "wide_both", False, dict(complexify=True, extend='exp', period=12), None,
     dict(on_left=True, on_right=False, block_size=1)),
    ("sst_iterative", "sst_prcp", False, dict(complexify=False), None,
     dict(on_left=True, on_right=True, block_size=1, strategy='iterative')),
]
IDS = [c[0] for c in CASES]


def _tol(dtype):
    """of the largest value: the row-bootstrap tests' bound (tests/test_gpu_mca.py, device replicates against the host loop)"""
    return 2e-5 if np.dtype(dtype) == np.float32 else 1e-8


def _model(inp, single, solve_kw, rot):
    fields = make_input(inp)
    if single:
        fields = fields[:1]
    m = MCA(*fields)
    m.solve(**solve_kw)
    if rot:
        m.rotate(*rot)
    return m, fields


def _bootstrap(m, n_modes, kw, host=False):
    m._bootstrap_on_host = host
    np.random.seed(5)
    return m.bootstrapping(3, n_modes=n_modes, axis=1, **kw)


@pytest.fixture(scope="module")
def device_results():
    """bootstrapping(3, n_modes=4, axis=1) of every case on the device path, computed once for the tests below"""
    out = {}
    for tag, inp, single, solve_kw, rot, kw in CASES:
        m, fields = _model(inp, single, solve_kw, rot)
        out[tag] = (_bootstrap(m, 4, kw), fields[0].dtype)
    return out


# ----------------------------------------------------------------------------------------------
# 1. the reference's numbers
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", IDS)
def test_column_bootstrapping_matches_the_reference(tag, device_results):
    """`xmca.array.MCA.bootstrapping(3, n_modes=4, axis=1, ...)` of the real reference under np.random.seed(5): the same draws from
    the same global stream, all 12 values of a case, absolutely in units of the largest."""
    ref = np.load(os.path.join(GOLDEN_DIR, "bootstrap_columns_cases.npz"))[tag]
    out, dtype = device_results[tag]
    assert out.shape == ref.shape == (4, 3)
    err = np.max(np.abs(out - ref)) / np.abs(ref).max()
    print(tag, "max |device - reference| / max |reference| = %.3e" % err)
    assert err < _tol(dtype)


# ----------------------------------------------------------------------------------------------
# 2. the kept host loop
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,inp,single,solve_kw,rot,kw", CASES, ids=IDS)
def test_device_replicates_equal_the_host_loop(tag, inp, single, solve_kw, rot, kw, device_results):
    m, fields = _model(inp, single, solve_kw, rot)
    host = _bootstrap(m, 4, kw, host=True)
    out, dtype = device_results[tag]
    assert out.shape == host.shape
    err = np.max(np.abs(out - host)) / np.abs(host).max()
    print(tag, "max |device - host loop| / max |host loop| = %.3e" % err)
    assert err < _tol(dtype)


def test_rank_deficient_tail_equals_the_host_loop():
    """small_both is 40 x 24 and 40 x 18: every replicate with a duplicated column has a singular side, rank and n_out stay 18 and
    the trailing values are zero up to rounding.  All 18 modes, absolutely against sigma_1.  (Measured on MI355X before the
    values-only two-field solve reported eigenvalues of K^H K below their rounding noise as zero: exact zeros came out as the square
    root of that noise, largest |device - host loop| = 1.205e-8 sigma_1 against the bound of 1e-8; the host loop, whose solve
    has vectors and refines its tail, returns 1e-16 ... 1e-24 there.)"""
    m, fields = _model("small_both", False, dict(complexify=False), None)
    kw = dict(on_left=True, on_right=True, block_size=2)
    rank = min(m._n_observations['left'], *m._n_variables.values())
    assert rank == 18
    dev = _bootstrap(m, rank, kw)
    host = _bootstrap(m, rank, kw, host=True)
    assert dev.shape == host.shape == (18, 3)
    sigma1 = host.max(axis=0)
    print("tail (device):", dev[-3:], "tail (host):", host[-3:])
    assert np.all(host[-1] < 1e-10 * sigma1)                   # the case is what it claims to be: rank deficient
    assert np.max(np.abs(dev - host) / sigma1) < 1e-8


# ----------------------------------------------------------------------------------------------
# 3. the device path is taken
# ----------------------------------------------------------------------------------------------
def test_axis_1_runs_on_the_device_without_a_model_per_replicate(monkeypatch):
    m, _ = _model("mixed_both", False, dict(complexify=False), None)
    dev = m._device()
    made = []
    init = MCA.__init__

    def counting(self, *a, **k):
        made.append(1)
        return init(self, *a, **k)
    monkeypatch.setattr(MCA, "__init__", counting)
    dev.reset_timings()
    np.random.seed(1)
    out = m.bootstrapping(3, n_modes=4, axis=1, on_left=True, on_right=True, block_size=5)
    assert out.shape == (4, 3) and np.all(out > 0)
    assert "resample" in dev.timings(), sorted(dev.timings())
    assert not made, "bootstrapping(axis=1) built %d MCA models" % len(made)


# ----------------------------------------------------------------------------------------------
# 4. the gather through the ABI: hand-made indices, no RNG
# ----------------------------------------------------------------------------------------------
T_EDGE = 8


def _expected(fields):
    """variance spectrum of the re-centered fields in float64, covariance normalisation of oracle/ref_numpy.py (kernel / (T - 1))"""
    X = [np.asarray(f, dtype=np.float64) for f in fields]
    X = [x - x.mean(axis=0) for x in X]
    kernel = X[0].T @ X[-1] / (X[0].shape[0] - 1)
    s = np.linalg.svd(kernel, compute_uv=False)
    return s[:min([X[0].shape[0]] + [x.shape[1] for x in X])]


def _patterns(n_l, n_r):
    """(cols_left, cols_right) per replicate, indices into [left | right]"""
    n = n_l + n_r
    ident = np.arange(n)
    last = np.full(n, n - 1)                                   # the last column of the right field (of the only field): rank 1
    if n_r:
        swap = np.concatenate([n_l + np.arange(n_l) % n_r, np.arange(n_r) % n_l])      # left entirely from right, right from left
    else:
        swap = (np.arange(n) * 7 + 3) % n                      # one field: any scattered pattern with repeats
    pats = [ident, ident[::-1].copy(), last, swap]
    return np.stack([p[:n_l] for p in pats]), (np.stack([p[n_l:] for p in pats]) if n_r else None)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n_l,n_r", [(1, 0), (63, 0), (64, 0), (65, 0), (257, 0), (65, 1), (3, 130)])
def test_column_gather_edges_through_the_abi(hip, n_l, n_r, dtype):
    rng = np.random.default_rng(100 * n_l + n_r)
    fields = [rng.standard_normal((T_EDGE, n)) * np.linspace(1.0, 3.0, n) for n in (n_l, n_r) if n]
    fields = [np.ascontiguousarray(f - f.mean(axis=0), dtype=dtype) for f in fields]
    rank = min([T_EDGE] + [f.shape[1] for f in fields])
    for side, f in enumerate(fields):
        hip.set_field(side, f)
    hip.bootstrap_begin(len(fields))
    cl, cr = _patterns(n_l, n_r)
    spectra, kept = hip.bootstrap_runs(T_EDGE, False, cl, cr, len(cl), False, 0, 1, 1e-8, rank, axis=1)
    assert spectra.shape == (len(cl), rank) and kept.all()
    concat = np.concatenate(fields, axis=1)
    tol = _tol(dtype)
    for run in range(len(cl)):
        want = _expected([concat[:, cl[run]]] + ([concat[:, cr[run]]] if n_r else []))
        err = np.max(np.abs(spectra[run] - want)) / want[0]
        print("N = (%d, %d) %s pattern %d: %.3e" % (n_l, n_r, np.dtype(dtype).name, run, err))
        assert err < tol, (run, spectra[run], want)
    # the identity replicate is the model itself
    hip.solve(len(fields))
    s = hip.singular_values(rank)
    assert np.max(np.abs(spectra[0] - s)) < tol * s[0]
    # the rank-1 replicate: nothing but sigma_1 (two fields: both are copies of one column)
    if rank > 1:
        assert np.all(np.abs(spectra[2][1:]) < tol * spectra[2][0])


@pytest.mark.parametrize("n_l,n_r", [(65, 0), (3, 130)])
def test_out_of_range_column_index_is_refused_before_anything_is_launched(hip, n_l, n_r):
    rng = np.random.default_rng(5)
    fields = [rng.standard_normal((T_EDGE, n)) for n in (n_l, n_r) if n]
    for side, f in enumerate(fields):
        hip.set_field(side, f)
    hip.bootstrap_begin(len(fields))
    rank = min([T_EDGE] + [f.shape[1] for f in fields])
    for bad in (n_l + n_r, -1):
        cl, cr = _patterns(n_l, n_r)
        cl = cl[:1].copy()
        cr = None if cr is None else cr[:1].copy()
        (cl if cr is None else cr)[0, -1] = bad
        hip.reset_timings()
        with pytest.raises(ValueError, match="column index out of range"):
            hip.bootstrap_runs(T_EDGE, False, cl, cr, 1, False, 0, 1, 1e-8, rank, axis=1)
        assert "resample" not in hip.timings()


# ----------------------------------------------------------------------------------------------
# 5. lanes
# ----------------------------------------------------------------------------------------------
def test_column_replicates_do_not_depend_on_the_number_of_lanes(tmp_path):
    """Replicates are independent once the indices are composed: one lane (XMCA_RULE_N_LANES=1, read once per process, hence the
    child) and the default number of lanes give the same bits."""
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r);"
            "from golden_inputs import make_input; from xmca_amd.array import MCA;"
            "m = MCA(*make_input('mixed_both')); m.solve(complexify=True); m.rotate(4, 1); np.random.seed(5);"
            "np.save(sys.argv[1], m.bootstrapping(5, n_modes=4, axis=1, on_left=True, on_right=True, block_size=5))"
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
