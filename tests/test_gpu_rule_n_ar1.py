"""Red-noise (AR(1)) surrogates of rule_n on the GPU:

* the filter kernels against the numpy twin (tests/ar1_cases.py) on the device's own normals, at the segment edges;
* the lag-1 estimator against the twin at the chunk edges of the column passes;
* `MCA.lag1_autocorrelation()`: masks, invariance under column scaling, nothing fetched;
* EXACT per-run parity of `xmca_rule_n_ar1` with the numpy oracle fed the device's red surrogates, lanes, later blocks;
* phi = 0 is the white test bit for bit; phi = 0.8 moves the null; facade, two ranks over gloo, the native communicator.
"""
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch                                  # before the library: one HIP runtime per process, the one torch brings

import ar1_cases as A
from oracle import ref_numpy as O
from xmca_amd import _hip
from xmca_amd.array import MCA

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL_CHUNKS = 32               # row chunks of the column passes (csrc/kernels.h)
EPS = np.finfo(np.float64).eps


def _normals(hip, T, N, seed, run, side):
    return hip.surrogate(T * N, seed, run, side).reshape(T, N)


# ----------------------------------------------------------------------------------------------
# 1. the filter against the twin
# ----------------------------------------------------------------------------------------------
def _filter_shapes():
    seg = _hip.ar1_segments(1000, 64)
    assert len(seg) > 1                                         # L comes from a shape that is split
    L = seg[0][1] - seg[0][0]
    shapes = [(T, N) for T in (1, 2, L - 1, L, L + 1, 2 * L + 3) for N in (1, 63, 64, 65, 257)]
    assert len(_hip.ar1_segments(L, 64)) == 1 and len(_hip.ar1_segments(L + 1, 64)) == 2 and len(_hip.ar1_segments(2 * L + 3, 257)) == 3
    assert any(T % 2 and N % 2 and T > 1 and N > 1 for T, N in shapes)       # a Philox pair straddles a row end
    return shapes + [(5000, 65)]                                # the most segments there are, longer than the shortest


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_filter_equals_the_twin_at_the_segment_edges(hip, dtype):
    for T, N in _filter_shapes():
        phi = A.cycled_phi(N)
        e = _normals(hip, T, N, 77, 3, 1)
        dev = hip.surrogate_ar1(T, N, phi, 77, 3, 1, dtype)
        assert dev.shape == (T, N)
        assert np.array_equal(dev.astype(dtype).astype(np.float64), dev)                # values of the run dtype
        ref = A.ar1_filter(e, phi, dtype)
        err = np.max(np.abs(dev - ref), axis=0)
        bound = A.filter_bound(ref, phi, T, dtype)
        assert np.all(err <= bound), (T, N, np.argmax(err / bound), np.max(err / bound))
        white = phi == 0.0
        assert np.array_equal(dev[:, white], e.astype(dtype).astype(np.float64)[:, white]), (T, N)       # bit for bit


def test_a_phi_outside_the_open_interval_is_refused_before_any_launch(hip):
    spectra, kept = np.zeros((2, 3)), np.zeros(2, dtype=np.int32)
    for bad in (1.0, -1.0, np.nan, np.inf):
        phi = np.array([0.5, bad, 0.0])
        with pytest.raises(ValueError):
            hip.surrogate_ar1(8, 3, phi, 1, 0, 0, np.float64)
        # the same check of the library in front of the lanes (the binding's own check is not in the way here)
        rc = hip._lib.xmca_rule_n_ar1(hip._h, 8, 3, 0, 1, None, 0, 0, 1, 1e-8, 0, 2, 1, _hip.XMCA_F64, _hip._ptr(spectra), _hip._ptr(kept), 3,
                                      _hip._ptr(phi), None)
        assert rc == _hip.ERR_INVALID
        with pytest.raises(ValueError):
            hip.rule_n(8, 3, 0, 1, False, False, 0, 1, 1e-8, 0, 2, 1, np.float64, 3, ar1=(phi, None))


# ----------------------------------------------------------------------------------------------
# 2. the estimator against the twin
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_estimator_equals_the_twin_at_the_chunk_edges(hip, dtype):
    from oracle.philox_numpy import surrogate
    for T in (2, 3, 31, 33, 2 * COL_CHUNKS + 1):                  # row chunks that are empty or hold a single row
        for N in (1, 65, 300):
            x = A.ar1_filter(surrogate(T * N, 11, T, 0).reshape(T, N), A.cycled_phi(N) * 0.9)
            x = x - x.mean(axis=0)                                # the estimate is taken from a centred field
            if N > 1:
                x[:, -1] = 2.5                                    # ... and one constant column
            x = np.ascontiguousarray(x.astype(dtype))
            hip.set_field(0, x)
            phi = hip.lag1_autocorrelation(0, N)
            ref = A.lag1(x)
            assert phi.dtype == np.float64 and np.all(np.isfinite(phi))
            assert np.max(np.abs(phi - ref)) <= 4 * T * EPS, (T, N, np.max(np.abs(phi - ref)) / (T * EPS))
            if N > 1:
                assert phi[-1] == 0.0
            assert np.array_equal(hip.lag1_autocorrelation(0, N), phi)


# ----------------------------------------------------------------------------------------------
# 3. through the class
# ----------------------------------------------------------------------------------------------
def _red_fields(T=50):
    from oracle.philox_numpy import surrogate
    a = A.ar1_filter(surrogate(T * 30, 5, 0, 0).reshape(T, 30), np.linspace(-0.3, 0.9, 30)).reshape(T, 6, 5)
    b = A.ar1_filter(surrogate(T * 8, 5, 0, 1).reshape(T, 8), 0.6)
    a[:, 0, 1] = a[:, 3, 3] = a[:, 5, 4] = np.nan
    return a, b


def test_class_estimate_has_the_masks_and_survives_column_scaling(hip):
    T = 50
    a, b = _red_fields(T)
    masked = np.isnan(a[0])
    m = MCA(a, b, handle=hip)
    m.solve()
    phi = m.lag1_autocorrelation()
    assert sorted(phi) == ['left', 'right'] and phi['left'].shape == (6, 5) and phi['right'].shape == (8,)
    assert phi['left'].dtype == np.float64 and np.array_equal(np.isnan(phi['left']), masked) and not np.isnan(phi['right']).any()
    X = m._get_X(real=True)
    assert np.max(np.abs(phi['left'][~masked] - A.lag1(X['left']))) <= 4 * T * EPS
    assert np.max(np.abs(phi['right'] - A.lag1(X['right']))) <= 4 * T * EPS

    def close(other):
        return all(np.allclose(other[k], phi[k], rtol=0, atol=1e-12, equal_nan=True) for k in phi)

    mn = MCA(a, b, handle=hip)
    mn.normalize()
    mn.solve()
    assert close(mn.lag1_autocorrelation())
    mw = MCA(a, b, handle=hip)
    mw.apply_weights(left=np.linspace(0.5, 2.0, 27)[None, :], right=np.linspace(3.0, 1.0, 8)[None, :])
    mw.solve()
    assert close(mw.lag1_autocorrelation())
    mc = MCA(a, b, handle=hip)
    mc.solve(complexify=True)
    assert close(mc.lag1_autocorrelation())                      # the real fields of the analytic signal
    mf = MCA(a.astype(np.float32), b.astype(np.float32), handle=hip)
    mf.solve()
    f32 = mf.lag1_autocorrelation()
    assert f32['left'].dtype == np.float64
    Xf = mf._get_X(real=True)
    assert np.max(np.abs(f32['right'] - A.lag1(Xf['right']))) <= 4 * T * EPS


def test_class_estimate_of_a_tensor_model_fetches_nothing_but_the_maps(hip):
    a, b = _red_fields()
    ref = MCA(a, b, handle=hip)
    ref.solve()
    want = ref.lag1_autocorrelation()
    dev = torch.device("cuda", 0)
    mt = MCA(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), handle=hip)
    mt.solve()
    resident = mt._vectors_resident()
    assert mt._store_is_raw
    got = mt.lag1_autocorrelation()
    assert mt._store_is_raw and mt._vectors_resident() == resident      # neither the fields nor the vectors came to the host
    for k in want:
        assert isinstance(got[k], np.ndarray) and np.allclose(got[k], want[k], rtol=0, atol=1e-12, equal_nan=True)


# ----------------------------------------------------------------------------------------------
# 4. run parity with the oracle on the device's red surrogates
# ----------------------------------------------------------------------------------------------
def _phi_of(widths, seed=8):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-0.3, 0.95, w) for w in widths]


def _ar1_pair(phis):
    return (phis[0], phis[1] if len(phis) == 2 else None)


@pytest.mark.parametrize("T,widths,cplx,rot", [
    (40, (24, 18), False, None),
    (60, (300, 200), True, None),
    (62, (300, 200), True, None),
    (60, (300,), False, (6, 1)),
    (60, (200, 150), True, (4, 2)),
    (500, (1200, 900), True, None),          # the tridiagonal values-only route
])
def test_red_runs_equal_the_oracle_on_the_same_surrogates(hip, T, widths, cplx, rot):
    seed, n_runs = 20240607, (5 if T < 200 else 2)
    n_fields = len(widths)
    p, power = rot if rot else (0, 0)
    n_out = p if rot else min((T,) + widths)
    phis = _phi_of(widths)
    args = (T, widths[0], widths[1] if n_fields == 2 else 0, n_fields, cplx, bool(rot), p, max(power, 1), 1e-8)
    trd_before = hip.timings().get("trd_reduce_calls", 0)
    spectra, kept = hip.rule_n(*args, 0, n_runs, seed, np.float64, n_out, ar1=_ar1_pair(phis))
    assert spectra.shape == (n_runs, n_out)
    white, white_kept = hip.rule_n(*args, 0, 1, seed, np.float64, n_out)
    assert not (kept[0] and white_kept[0]) or not np.array_equal(white[0], spectra[0])        # the option is not a no-op
    for r in range(n_runs):
        data = [hip.surrogate_ar1(T, w, phis[side], seed, r, side, np.float64) for side, w in enumerate(widths)]
        om = O.OracleModel(*data)
        om.solve(complexify=cplx)
        try:
            if rot:
                om.rotate(*rot)
        except RuntimeError:                                     # the reference drops the run
            assert kept[r] == 0
            continue
        ref = om.variance()
        assert kept[r] == 1 and ref.shape == (n_out,)
        keep = ref > 1e-7 * ref[0]
        assert np.max(np.abs(spectra[r][keep] - ref[keep]) / ref[keep]) < 1e-5, (r, widths, cplx, rot)
        assert np.all(np.abs(spectra[r][~keep]) < 1e-5 * ref[0])
    if T >= 200:
        assert hip.timings().get("trd_reduce_calls", 0) >= trd_before + n_runs
    again, _ = hip.rule_n(*args, n_runs - 2, n_runs, seed, np.float64, n_out, ar1=_ar1_pair(phis))
    assert np.array_equal(again, spectra[n_runs - 2:n_runs])     # a later block is keyed by the run index only


def test_red_spectra_do_not_depend_on_the_number_of_lanes():
    code = ("import sys, numpy as np; sys.path.insert(0, %r); from xmca_amd import _hip; h = _hip.Handle(0);"
            "rng = np.random.default_rng(8); pl, pr = rng.uniform(-0.3, 0.95, 300), rng.uniform(-0.3, 0.95, 200);"
            "a, ka = h.rule_n(60, 300, 200, 2, True, False, 0, 1, 1e-8, 0, 7, 5, np.float64, 60, ar1=(pl, pr));"
            "c, kc = h.rule_n(48, 300, 0, 1, False, True, 4, 1, 1e-8, 2, 9, 3, np.float32, 4, ar1=(pl, None));"
            "np.savez(sys.argv[1], a=a, ka=ka, c=c, kc=kc)" % REPO)
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        for lanes in ("1", "4"):
            dst = os.path.join(tmp, "l%s.npz" % lanes)
            r = subprocess.run([sys.executable, "-c", code, dst], env=dict(os.environ, XMCA_RULE_N_LANES=lanes), capture_output=True,
                               text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            outs.append(dict(np.load(dst)))
    assert outs[0]["ka"].sum() == 7
    for k in outs[0]:
        assert np.array_equal(outs[1][k], outs[0][k]), k


# ----------------------------------------------------------------------------------------------
# 5. phi = 0 is the white test
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx,rot", [(False, None), (True, None), (False, (4, 1))], ids=["real", "complex", "rotated"])
def test_phi_zero_is_the_white_test_bit_for_bit(hip, cplx, rot):
    a, b = _red_fields()
    m = MCA(a, b, handle=hip)
    m.solve(complexify=cplx)
    if rot:
        m.rotate(*rot)
    white = m.rule_n(5, seed=9)
    assert np.array_equal(m.rule_n(5, seed=9, noise='ar1', phi=0.0), white)
    assert not np.array_equal(m.rule_n(5, seed=9, noise='ar1', phi=0.5), white)


# ----------------------------------------------------------------------------------------------
# 6. the null changes
# ----------------------------------------------------------------------------------------------
def test_red_null_lies_above_the_white_null(hip):
    """Field: twin AR(1), phi = 0.8, T = 120, N = 40, Philox seed 20240607.  The numpy check with the twin and the oracle (runs of
    seed 1): share of mode 1 in the normalised spectrum 0.0533 ... 0.0636 for white surrogates, 0.1126 ... 0.1662 for phi = 0.8 and
    0.1050 ... 0.1528 for the estimated phi, whose mean is 0.770 (expected 0.8 - (1 + 3 phi) / T = 0.772)."""
    from oracle.philox_numpy import surrogate
    T, N = 120, 40
    field = A.ar1_filter(surrogate(T * N, 20240607, 0, 0).reshape(T, N), 0.8)
    m = MCA(field, handle=hip)
    m.solve()
    est = m.lag1_autocorrelation()['left']
    assert 0.65 <= est.mean() <= 0.85

    def share(sp):
        assert sp.shape[1] == 40
        return sp[0] / sp.sum(axis=0)

    white = share(m.rule_n(40, seed=1))
    red = share(m.rule_n(40, seed=1, noise='ar1', phi=0.8))
    red_est = share(m.rule_n(40, seed=1, noise='ar1'))
    print("share of mode 1: white %.4f..%.4f, phi=0.8 %.4f..%.4f, estimated %.4f..%.4f, mean phi %.4f"
          % (white.min(), white.max(), red.min(), red.max(), red_est.min(), red_est.max(), est.mean()))
    assert red.min() > white.max()
    assert red_est.min() > white.max()


# ----------------------------------------------------------------------------------------------
# 7. facade and sharding
# ----------------------------------------------------------------------------------------------
def test_facade_forwards_the_noise_model():
    from test_gpu_xarray_facade import _fields
    from xmca_amd.xarray import xMCA
    left, right = _fields()
    xm = xMCA(left, right)
    xm.solve()
    m = MCA(left.values, right.values)
    m.solve()
    runs = xm.rule_n(5, seed=3, noise='ar1')
    assert runs.dims == ('mode', 'run')
    assert np.array_equal(runs.values, m.rule_n(5, seed=3, noise='ar1'))
    assert not np.array_equal(runs.values, m.rule_n(5, seed=3))
    phi = xm.lag1_autocorrelation()
    assert phi['left'].shape == left.shape[1:] and np.isnan(phi['left'][2, 3]) and np.isnan(phi['left']).sum() == 1


def _worker(rank, world, port, n_runs, q):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch.distributed as td
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    from golden_inputs import make_input as mk
    from xmca_amd import _hip as hp
    from xmca_amd.array import MCA as M
    m = M(*mk("wide_both"), handle=hp.Handle(0))
    m.solve(complexify=True)
    out = m.rule_n(n_runs, seed=1000 + rank, noise='ar1')        # every rank estimates the same phi; rank 0's seed is broadcast
    out_phi = m.rule_n(n_runs, seed=77, noise='ar1', phi=0.4)
    q.put((rank, out, out_phi))
    td.destroy_process_group()


def test_two_ranks_on_one_device_equal_a_single_rank():
    import torch.multiprocessing as mp
    from golden_inputs import make_input
    n_runs, world = 5, 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_runs, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    m = MCA(*make_input("wide_both"), handle=_hip.Handle(0))
    m.solve(complexify=True)
    single = m.rule_n(n_runs, seed=1000, noise='ar1')
    single_phi = m.rule_n(n_runs, seed=77, noise='ar1', phi=0.4)
    for _, out, out_phi in results:
        assert np.array_equal(out, single) and np.array_equal(out_phi, single_phi)


def test_native_communicator_of_one_rank_gives_the_plain_call():
    code = ("import sys, os, numpy as np; sys.path.insert(0, %r);"
            "from xmca_amd import _hip, dist;"
            "h = _hip.Handle(0); c = dist.init_native(h, rank=0, world=1, id_file=sys.argv[1] + '.id');"
            "rng = np.random.default_rng(8); ar1 = (rng.uniform(-0.3, 0.95, 400), rng.uniform(-0.3, 0.95, 300));"
            "args = (150, 400, 300, 2, True, True, 6, 2, 1e-8);"
            "a, ka = h.rule_n(*args, 0, 5, 2 ** 40 + 77, np.float64, 6, ar1=ar1);"
            "w, kw = h.rule_n(*args, 0, 5, 2 ** 40 + 77, np.float64, 6);"
            "s, ks = dist.sharded_rule_n(h, 5, T=150, Nx=400, Ny=300, n_fields=2, complexify=True, rotated=True, p=6, power=2,"
            " tol=1e-8, seed=2 ** 40 + 77, dtype=np.float64, n_out=6, comm=c, ar1=ar1);"
            "c.close();"
            "np.savez(sys.argv[1], a=a, ka=ka, s=s, ks=ks, w=w)" % REPO)
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "o.npz")
        r = subprocess.run([sys.executable, "-c", code, dst], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        o = dict(np.load(dst))
    assert np.array_equal(o["a"], o["s"]) and np.array_equal(o["ka"], o["ks"]) and o["ka"].sum() >= 1
    assert not np.array_equal(o["a"], o["w"])
