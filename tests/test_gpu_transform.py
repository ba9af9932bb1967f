"""predict() and reconstructed_fields() on the device (xmca_predict / xmca_reconstruct / xmca_project without V).

a. handle level against float64 numpy at edge shapes (T' in {1, 5, 130}, N' in {1, 257, 300}, m in {0, 1, 7, rank}), for real
   float64, complex and float32-resident vectors, resident and host vectors;
b. model level, the device route against the host route (`_transform_on_host`);
c. nothing fetched, nothing evicted;
d. invariants without a reference: predict(training data) = pcs(), full reconstruction = the input."""
import zlib

import numpy as np
import pytest

from golden_inputs import make_input
from xmca_amd import _hip
from xmca_amd.array import MCA

pytestmark = pytest.mark.gpu

T_TRAIN = 64


@pytest.fixture(scope="module")
def h():
    handle = _hip.Handle(0)
    yield handle
    handle.close()


def _solve(h, kind, N, rng):
    """one-field solve on the handle; returns (V: N x rank host copy, field dtype)"""
    dtype = np.float32 if kind == "f32" else np.float64
    X = rng.standard_normal((T_TRAIN, N)).astype(dtype)
    X -= X.mean(axis=0)
    h.set_field(0, X)
    if kind == "cplx":
        h.complexify(T_TRAIN)
    rank = h.solve(1)
    V = h.vectors(0, rank, N, np.float64).T
    if kind == "f32" and N > T_TRAIN:
        assert h.vectors_are_f32(0)
    return V, dtype


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _scale(a):
    return max(float(np.nanmax(np.abs(a))), 1e-300)


def _tol(dtype):
    return 2e-5 if dtype == np.float32 else 1e-10          # the repository's float32 bar, float64 relative


CASES = [(kind, T, N) for kind in ("f64", "cplx", "f32") for T, N in ((1, 257), (5, 300), (130, 1), (130, 257), (5, 1))]


@pytest.mark.parametrize("kind,T,N", CASES)
@pytest.mark.parametrize("resident", [True, False])
def test_predict_handle_matches_numpy(h, kind, T, N, resident):
    rng = np.random.default_rng(_seed(kind, T, N))
    V, dtype = _solve(h, kind, N, rng)
    rank = V.shape[1]
    keep = np.sort(rng.choice(N + 3, N, replace=False))
    X = (3.0 + rng.standard_normal((T, N + 3))).astype(dtype)
    X[:, np.setdiff1d(np.arange(N + 3), keep)] = np.nan        # masked columns may hold anything
    mean = rng.standard_normal(N).astype(dtype)
    std = rng.uniform(0.5, 2.0, N).astype(dtype)
    for m in sorted({1, min(7, rank), rank}):
        for cw in (False, True):
            W = rng.standard_normal((m, 3)) + (1j * rng.standard_normal((m, 3)) if cw else 0)
            xs = (X[:, keep] - mean) / std
            ref = (xs.astype(np.float64) @ V[:, :m]) @ W
            got = h.predict(0, X, keep, mean, std, None if resident else V[:, :m], W)
            assert got.shape == ref.shape and np.iscomplexobj(got) == np.iscomplexobj(ref)
            assert np.max(np.abs(got - ref)) <= _tol(dtype) * _scale(ref) * max(1.0, np.sqrt(N) / 4), (m, cw)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_predict_nan_row_and_bitwise_ingest(h, dtype):
    rng = np.random.default_rng(5)
    N = 257
    X0 = rng.standard_normal((T_TRAIN, 300))
    h.set_field(0, X0 - X0.mean(axis=0))
    h.solve(1)
    keep = np.sort(rng.choice(260, N, replace=False))
    X = (5.0 + 3.0 * rng.standard_normal((130, 260))).astype(dtype)
    mean = rng.standard_normal(N).astype(dtype)
    std = rng.uniform(0.3, 3.0, N).astype(dtype)
    # identity vectors and mix: the output is the ingested block itself (products by 1 and sums with 0 are exact)
    I = np.eye(N)
    got = h.predict(0, X, keep, mean, std, I, I)
    x = X[:, keep].copy()
    x -= mean
    x /= std
    assert np.array_equal(got, x.astype(np.float64))
    got = h.predict(0, np.ascontiguousarray(X[:, keep]), None, mean, None, I, I)     # contiguous case, no division
    x = X[:, keep] - mean
    assert np.array_equal(got, x.astype(np.float64))
    # a NaN in a kept column makes exactly its row NaN, as numpy's matmul does
    X[7, keep[100]] = np.nan
    got = h.predict(0, X, keep, mean, std, rng.standard_normal((N, 10)), rng.standard_normal((10, 4)))
    assert np.isnan(got[7]).all() and not np.isnan(np.delete(got, 7, axis=0)).any()


@pytest.mark.parametrize("kind,T,N", CASES)
@pytest.mark.parametrize("resident", [True, False])
def test_reconstruct_handle_matches_numpy(h, kind, T, N, resident):
    rng = np.random.default_rng(_seed(kind, T, N, 1))
    V, dtype = _solve(h, kind, N, rng)
    rank = V.shape[1]
    n_full = N + 3
    keep = np.sort(rng.choice(n_full, N, replace=False))
    masked = np.setdiff1d(np.arange(n_full), keep)
    mean = rng.standard_normal(N)
    std = rng.uniform(0.5, 2.0, N)
    for m in sorted({0, 1, min(7, rank), rank}):
        for cb in (False, True):
            B = rng.standard_normal((T, m)) + (1j * rng.standard_normal((T, m)) if cb else 0)
            core = (B @ V[:, :m].conj().T).real
            Vh = None if resident else V[:, :m]
            got = h.reconstruct(0, B, Vh, N, keep_idx=keep, N_full=n_full, mean=mean, std=std)
            ref = core * std + mean
            assert got.shape == (T, n_full) and got.dtype == np.float64
            assert np.isnan(got[:, masked]).all() and not np.isnan(got[:, keep]).any()
            assert np.max(np.abs(got[:, keep] - ref)) <= _tol(dtype) * _scale(ref), (m, cb)
            got = h.reconstruct(0, B, Vh, N)                       # compact, no scaling
            assert got.shape == (T, N)
            if m == 0:
                assert np.array_equal(got, np.zeros((T, N)))
            else:
                assert np.max(np.abs(got - core)) <= _tol(dtype) * _scale(core)


def test_project_resident_equals_host_vectors(h):
    rng = np.random.default_rng(9)
    for kind in ("f64", "cplx", "f32"):
        V, dtype = _solve(h, kind, 300, rng)
        for m in (1, 7, V.shape[1]):
            a = h.project(0, None, T_TRAIN, m, 300)
            b = h.project(0, V[:, :m].astype(np.result_type(V.dtype, dtype)), T_TRAIN)
            assert np.array_equal(a, b), (kind, m)


# ----------------------------------------------------------------------------------------------
# b. model level: device route against `_transform_on_host`
# ----------------------------------------------------------------------------------------------
def _model(name):
    if name == "device_pre":
        left, right = make_input("wide_both")
        m = MCA(left, right, preprocess='device')
        m.normalize()
        m.apply_weights(left=np.linspace(0.5, 1.5, left.shape[1]))
        m.solve()
        m.rotate(4, power=2)
        return m, (left, right)
    fields = make_input("sst_prcp" if name.startswith("sst") else name.split(":")[0])
    m = MCA(*fields)
    if name == "sst_varimax":
        m.solve()
        m.rotate(10)
    elif name == "sst_promax":
        m.solve()
        m.rotate(10, power=2)
    elif name == "wide_both:cplx_rot":
        m.solve(complexify=True)
        m.rotate(6, power=4)
    else:
        m.solve()
    return m, fields


def _calls(fields):
    new = [f[:37] * 1.1 for f in fields]
    calls = [("predict", dict(n=None)), ("predict", dict(n=3, scaling='eigen', phase_shift=0.4)),
             ("predict", dict(n=5, scaling='max')), ("predict", dict(n=4, scaling='std'))]
    calls += [("rec", dict(mode=mode, original_scale=o)) for mode in (None, 3, slice(2, 6)) for o in (True, False)]
    calls += [("recX", dict(mode=slice(2, 6), original_scale=True)), ("recX", dict(mode=0, original_scale=False))]
    return new, calls


def _run(m, new, calls):
    out = []
    for what, kw in calls:
        if what == "predict":
            out.append(m.predict(*new, **kw))
        elif what == "rec":
            out.append(m.reconstructed_fields(**kw))
        else:
            out.append(m._reconstructed_X(**kw))
    return out


@pytest.mark.parametrize("name", ["sst_prcp", "sst_varimax", "sst_promax", "wide_both:cplx_rot", "wide_both_f32", "device_pre"])
def test_model_device_route_matches_host_route(name):
    m, fields = _model(name)
    new, calls = _calls(fields)
    dev = _run(m, new, calls)
    assert m._V._pending == set(m._keys)            # the device route fetched nothing
    m._transform_on_host = True
    host = _run(m, new, calls)
    tol = 2e-5 if fields[0].dtype == np.float32 else 1e-10
    for (what, kw), d, r in zip(calls, dev, host):
        for k in m._keys:
            a, b = d[k], r[k]
            assert a.shape == b.shape and a.dtype == b.dtype, (what, kw, k, a.dtype, b.dtype)
            assert np.array_equal(np.isnan(a), np.isnan(b)), (what, kw, k)
            if np.isfinite(b).any():          # (a float32 model whose null mode has sigma = 0: 0 / 0 makes both routes all NaN)
                assert np.nanmax(np.abs(a - b)) <= tol * _scale(b), (what, kw, k, np.nanmax(np.abs(a - b)) / _scale(b))


# ----------------------------------------------------------------------------------------------
# c. nothing fetched, nothing evicted
# ----------------------------------------------------------------------------------------------
def test_transforms_keep_the_resident_state():
    left, right = make_input("sst_prcp")
    m = MCA(left, right)
    m.solve()
    m.rotate(10, power=2)
    pcs6, eofs6 = m.pcs(6), m.eofs(6)
    dev = m._device()
    owner = dev.fields_owner
    m.predict(left[:20], right[:20])
    m.reconstructed_fields()
    m.reconstructed_fields(3)
    m.pcs(m._analysis['rank'], rotated=False)
    assert m._V._pending == set(m._keys)
    assert dev.holds_result_of(m)
    assert dev.fields_owner == owner
    for k in m._keys:
        assert np.array_equal(m.pcs(6)[k], pcs6[k])
        assert np.array_equal(m.eofs(6)[k], eofs6[k], equal_nan=True)


# ----------------------------------------------------------------------------------------------
# d. invariants
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [None, (10, 1), (10, 2)])
def test_predict_of_training_data_is_pcs(rot):
    left, right = (f.astype(np.float64) for f in make_input("sst_prcp"))
    m = MCA(left, right)
    m.solve()
    if rot:
        m.rotate(*rot)
    pcs = m.pcs()
    new = m.predict(left, right)
    for k in m._keys:
        assert np.max(np.abs(new[k] - pcs[k])) <= 1e-10 * _scale(pcs[k])


@pytest.mark.parametrize("normalize", [False, True])
def test_full_reconstruction_returns_the_input(normalize):
    (X,) = make_input("unit_left")
    m = MCA(X)
    if normalize:
        m.normalize()
    m.solve()
    rec = m.reconstructed_fields()['left']
    assert rec.shape == X.shape
    assert np.max(np.abs(rec - X)) <= 1e-10 * np.max(np.abs(X))
