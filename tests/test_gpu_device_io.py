"""GPU: fields that come in as tensors on the device and results that stay there.

  * the strided ingest (`xmca_set_field_strided`) in its three regimes, float32 and float64, at the edges of the 64 x 64 transpose
    tile and of the 16-byte accesses of the row copy: the resident field is BIT-equal to the numpy array of the same view, the
    parent tensor is unchanged, and nothing next to the view (the parents are filled with random values around it) leaks in;
  * ownership (the model keeps nothing of the tensor) and ordering (work queued on the caller's stream is waited for);
  * `MCA(tensor)` against `MCA(tensor.cpu().numpy(), preprocess='device')`, and every getter of `output='torch'` against the
    numpy result of the same model in the same handle state;
  * `predict` with new data on the GPU in a contiguous, a padded-row and a time-fast layout;
  * the errors of the constructor.

Tolerance of the class parity: none was needed.  Every torch result - unrotated, Varimax- and Promax-rotated, real and complex,
the plain `eofs()` that takes `xmca_get_maps` instead of `xmca_get_eofs` included - is `array_equal` (NaN positions included) to
the numpy result; the bound tests/test_gpu_maps.py holds between its two routes was not called upon."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from xmca_amd import _hip                                       # noqa: E402
from xmca_amd.array import MCA, _device_view, _numpy_result      # noqa: E402

pytestmark = pytest.mark.gpu

B = 64                                                           # edge of the transpose tile (csrc/kernels.h INGEST_TILE)
SHAPES = [(2, 1), (B - 1, B + 1), (B, B), (B + 1, 2 * B - 1), (67, 131)]
DTYPES = [torch.float32, torch.float64]
DEV = "cuda:0"

_HANDLES = []


def _handle(i=0):
    while len(_HANDLES) <= i:
        _HANDLES.append(_hip.Handle(0))
    return _HANDLES[i]


def _random(shape, dtype, seed):
    """random values with a few specials (NaN, inf, -0.0) scattered in, on the GPU"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float64).to(dtype)
    flat = x.reshape(-1)
    n = flat.numel()
    for i, v in enumerate((float("nan"), float("inf"), -0.0)):
        flat[(7 * i + 3) % n] = v
    return x.to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# (name, parent shape and view for a T x N field, regime the strides select)
def _contiguous(T, N):
    return (T, N), lambda p: p, _hip.INGEST_ROWS


def _transposed(T, N):
    return (N, T), lambda p: p.T, _hip.INGEST_TRANSPOSE if N > 1 else _hip.INGEST_ROWS


def _transposed_slice(T, N):
    """.T of a slice of a wider space-major parent: time is the fast axis, the base is aligned to the element only"""
    return (N + 1, T + 3), lambda p: p[:N, 2:2 + T].T, _hip.INGEST_TRANSPOSE if N > 1 else _hip.INGEST_ROWS


def _column_slice(T, N):
    """big[1:1+T, 3:3+N] of a parent with an odd row pitch: misaligned base, the alignment drifts from row to row"""
    pitch = N + 7 + (N % 2)
    assert pitch % 2 == 1
    return (T + 2, pitch), lambda p: p[1:1 + T, 3:3 + N], _hip.INGEST_ROWS


def _steps(T, N):
    return (2 * T + 1, 3 * N + 2), lambda p: p[0:2 * T:2, 0:3 * N:3], _hip.INGEST_GATHER if N > 1 else _hip.INGEST_ROWS


LAYOUTS = {"contiguous": _contiguous, "transposed": _transposed, "transposed_slice": _transposed_slice,
           "column_slice": _column_slice, "steps": _steps}


def _check_ingest(h, parent, view, regime):
    before = parent.clone()
    want = view.cpu().numpy()                                    # the numpy array of the same view
    dv = _device_view(view)
    T, N = dv.shape
    assert (T, N) == (view.shape[0], int(np.prod(view.shape[1:])))
    assert _hip.ingest_regime(T, N, dv.stride_t, dv.stride_n) == regime
    torch.cuda.synchronize()
    h.set_field_strided(0, dv)
    got = h.get_field(0, (T, N), want.dtype)
    assert got.dtype == want.dtype
    assert np.array_equal(_bits(got), _bits(want.reshape(T, N)))
    assert torch.equal(parent.view(torch.int32 if parent.dtype == torch.float32 else torch.int64),
                       before.view(torch.int32 if parent.dtype == torch.float32 else torch.int64))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_strided_ingest_is_bit_equal(layout, shape, dtype):
    T, N = shape
    pshape, take, regime = LAYOUTS[layout](T, N)
    parent = _random(pshape, dtype, seed=1000 * T + N)
    _check_ingest(_handle(), parent, take(parent), regime)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("T", [2, B - 1, B, B + 1, 67])
def test_strided_ingest_of_a_permuted_3d_tensor(T, dtype):
    """(T, 5, 7) permuted from (5, 7, T): the two spatial dimensions collapse to one stride, time is the fast axis"""
    parent = _random((5, 7, T), dtype, seed=T)
    view = parent.permute(2, 0, 1)
    assert tuple(view.shape) == (T, 5, 7)
    _check_ingest(_handle(), parent, view, _hip.INGEST_TRANSPOSE)


def test_a_view_two_strides_cannot_express_is_made_contiguous_on_the_device():
    parent = _random((9, 6, 8), torch.float64, seed=5)
    view = parent[:, ::2, 1:7]                                   # spatial strides (16, 1) with 6 columns: they do not collapse
    dv = _device_view(view)
    assert dv.ptr != view.data_ptr() and (dv.stride_t, dv.stride_n) == (18, 1)
    h = _handle()
    torch.cuda.synchronize()                                     # (the copy is torch's work on torch's stream)
    h.set_field_strided(0, dv)
    assert np.array_equal(_bits(h.get_field(0, (9, 18), np.float64)), _bits(view.cpu().numpy().reshape(9, 18)))


def test_strided_entry_keeps_the_checks_of_set_field():
    h = _handle()
    a = _random((6, 5), torch.float64, seed=1)
    b = _random((7, 5), torch.float64, seed=2)
    c = _random((6, 5), torch.float32, seed=3)
    h.set_field_strided(0, _device_view(a))
    with pytest.raises(ValueError, match="time dimensions"):
        h.set_field_strided(1, _device_view(b))
    with pytest.raises(ValueError, match="same dtype"):
        h.set_field_strided(1, _device_view(c))
    host = np.zeros((6, 5))
    with pytest.raises(ValueError, match="device"):             # a host address is refused, not read
        h.set_field_strided(0, _hip.DeviceView(host.ctypes.data, 6, 5, 5, 1, np.float64, owner=host))


# ----------------------------------------------------------------------------------------------
# ownership and ordering
# ----------------------------------------------------------------------------------------------
def test_the_model_owns_its_copy_of_the_tensor():
    x0 = np.random.default_rng(3).standard_normal((40, 6, 9))
    x = torch.from_numpy(x0).to(DEV)
    m = MCA(x, handle=_handle(0))
    x.fill_(float("nan"))
    torch.cuda.synchronize()
    m.solve()
    twin = MCA(x0, handle=_handle(1), preprocess="device")
    twin.solve()
    assert np.array_equal(m.singular_values(), twin.singular_values())


def test_the_constructor_waits_for_the_tensors_producer():
    """`x` is filled by an asynchronous copy from pinned memory on a side stream that is current when the model is built"""
    x0 = np.random.default_rng(4).standard_normal((1500, 2000)).astype(np.float32)
    host = torch.from_numpy(x0).pin_memory()
    side = torch.cuda.Stream(device=DEV)
    h = _handle(0)
    with torch.cuda.stream(side):
        x = torch.zeros(x0.shape, dtype=torch.float32, device=DEV)
        x.copy_(host, non_blocking=True)
        m = MCA(x, handle=h)
    got = h.get_field(0, x0.shape, np.float32)
    twin = MCA(x0, handle=_handle(1), preprocess="device")
    want = _handle(1).get_field(0, x0.shape, np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(m._field_means["left"], twin._field_means["left"])


# ----------------------------------------------------------------------------------------------
# the class
# ----------------------------------------------------------------------------------------------
def _fields(kind, n_fields):
    rng = np.random.default_rng(11 if kind == "f64" else 12)
    if kind == "f64":                                            # 40 x (6, 9) with three all-NaN grid points
        T, shapes, dt = 40, [(6, 9), (4, 5)], np.float64
    else:
        T, shapes, dt = 33, [(50,), (21,)], np.float32
    k = 5
    pcs = rng.standard_normal((T, k)) * (6.0 * 0.7 ** np.arange(k))
    out = []
    for s in shapes[:n_fields]:
        n = int(np.prod(s))
        f = (pcs @ rng.standard_normal((k, n)) + 0.5 * rng.standard_normal((T, n)) + 3.0).astype(dt).reshape((T,) + s)
        out.append(f)
    if kind == "f64":
        out[0][:, 0, 0] = np.nan
        out[0][:, 3, 4] = np.nan
        out[0][:, 5, 8] = np.nan
    return out


def _same(t, a, what):
    """a torch result against the numpy one: a tensor on the GPU with the same dtype, shape and values (NaN positions included)"""
    assert isinstance(t, torch.Tensor) and t.device.type == "cuda", what
    g = t.cpu().numpy()
    assert g.dtype == a.dtype and g.shape == a.shape, (what, g.dtype, a.dtype, g.shape, a.shape)
    assert np.array_equal(g, a, equal_nan=True), (what, float(np.nanmax(np.abs(g - a))))


def _compare(m, name, *args, **kwargs):
    """getter `name` of the torch model against its own numpy result in the same handle state"""
    assert m._output == "torch"
    got = getattr(m, name)(*args, **kwargs)
    want = _numpy_result(m, name, *args, **kwargs)
    assert m._output == "torch"
    if not isinstance(got, tuple):
        got, want = (got,), (want,)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w)
        for k in w:
            _same(g[k], w[k], (name, args, kwargs, k))


def _all_getters(m, n_fields, cplx, new):
    """every getter that returns a dict of arrays, but `fields()` (which fetches the fields of a device-preprocessed model)"""
    for name, args, kwargs in [
            ("eofs", (4,), {}), ("eofs", (3,), {"scaling": "eigen"}), ("eofs", (4,), {"scaling": "max"}), ("eofs", (4,), {"scaling": "std"}),
            ("eofs", (slice(2, 3),), {"rotated": False}), ("spatial_amplitude", (4,), {}), ("spatial_amplitude", (4,), {"scaling": "max"}),
            ("spatial_phase", (4,), {}), ("reconstructed_fields", (4,), {}), ("reconstructed_fields", (2,), {"original_scale": False}),
            ("homogeneous_patterns", (3,), {}), ("pcs", (4,), {}), ("temporal_amplitude", (4,), {}), ("temporal_phase", (4,), {}),
            ("predict", (), {"left": new})]:
        _compare(m, name, *args, **kwargs)
    if cplx:
        _compare(m, "eofs", 4, phase_shift=0.7)
        _compare(m, "spatial_phase", 4, phase_shift=0.7)
    if n_fields == 2:
        _compare(m, "heterogeneous_patterns", 3)


@pytest.mark.parametrize("rot", [(4, 1), (4, 2)], ids=["varimax", "promax"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("n_fields", [1, 2])
@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_class_parity(kind, n_fields, cplx, rot):
    h = _handle(0)
    arrays = _fields(kind, n_fields)
    tensors = [torch.from_numpy(a).to(DEV) for a in arrays]
    keys = ["left", "right"][:n_fields]

    # the numpy model that preprocesses on the device, then the tensor model, one after the other on one handle
    mn = MCA(*arrays, handle=h, preprocess="device")
    assert mn._output == "numpy"
    fields_n = [h.get_field(s, mn._fields_store[k].shape, arrays[s].dtype) for s, k in enumerate(keys)]
    mn.solve(complexify=cplx)
    sv_n = mn.singular_values()
    mt = MCA(*tensors, handle=h)
    assert mt._output == "torch" and mt._store_is_raw
    for s, k in enumerate(keys):
        assert np.array_equal(mt._no_nan_index[k], mn._no_nan_index[k])
        assert mt._field_means[k].dtype == mn._field_means[k].dtype
        assert np.array_equal(_bits(mt._field_means[k]), _bits(mn._field_means[k]))
        assert np.array_equal(_bits(mt._field_stds[k]), _bits(mn._field_stds[k]))
        assert np.array_equal(_bits(h.get_field(s, mt._fields_store[k].shape, arrays[s].dtype)), _bits(fields_n[s]))
        assert mt._shape[k] == mn._shape[k] and mt._fields_spatial_shape[k] == mn._fields_spatial_shape[k]
    mt.solve(complexify=cplx)
    sv_t = mt.singular_values()
    assert isinstance(sv_t, np.ndarray) and sv_t.dtype == sv_n.dtype          # spectra stay numpy
    assert np.array_equal(sv_t, sv_n)

    new = tensors[0][:7] * 1.5 + 0.25
    _compare(mt, "eofs", 3)                                       # unrotated, the plain case: xmca_get_maps without options
    _compare(mt, "reconstructed_fields", 3)
    mt.rotate(*rot)
    # (float32 models other than one real field rotate loadings built on the host, as the reference does in float32: their
    # vectors are on the host from here on, and their getters are host results that are uploaded)
    resident = mt._vectors_resident()
    assert resident or kind == "f32"
    _all_getters(mt, n_fields, cplx, new)
    assert mt._vectors_resident() == resident and mt._store_is_raw            # nothing was fetched to answer them
    _compare(mt, "fields")
    assert isinstance(mt.variance(), np.ndarray) and isinstance(mt.norm()["left"], np.ndarray)

    mt._maps_on_host = True                                       # the forced host routes: computed as before, then uploaded
    for name in ("eofs", "spatial_amplitude", "spatial_phase"):
        _compare(mt, name, 4)
    mt._maps_on_host = False
    mt.truncate(6)                                                # the vectors are on the host from here on
    assert not mt._vectors_resident()
    _all_getters(mt, n_fields, cplx, new)
    _compare(mt, "fields", original_scale=True)


def test_cpu_tensor_and_explicit_numpy_output():
    h = _handle(0)
    a = _fields("f32", 1)[0]
    m = MCA(torch.from_numpy(a), handle=h)                        # a CPU tensor is its numpy array
    assert m._output == "numpy"
    m.solve()
    ref = MCA(a, handle=_handle(1))
    ref.solve()
    assert np.array_equal(m.singular_values(), ref.singular_values())
    assert isinstance(m.eofs(3)["left"], np.ndarray)
    mg = MCA(torch.from_numpy(a).to(DEV), handle=h, output="numpy")
    mg.solve()
    assert isinstance(mg.eofs(3)["left"], np.ndarray)
    assert np.array_equal(mg.eofs(3)["left"], ref.eofs(3)["left"])
    mh = MCA(a, handle=h, output="torch")                         # numpy in, tensors out
    mh.solve()
    _same(mh.eofs(3)["left"], ref.eofs(3)["left"], "numpy in, torch out")


# ----------------------------------------------------------------------------------------------
# predict
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_predict_from_gpu_tensors(kind):
    h = _handle(0)
    arrays = _fields(kind, 2)
    m = MCA(*[torch.from_numpy(a).to(DEV) for a in arrays], handle=h)
    m.solve()
    m.rotate(4, 2)
    resident = m._vectors_resident()
    assert resident or kind == "f32"
    tdt = torch.float64 if kind == "f64" else torch.float32
    for key, a in zip(("left", "right"), arrays):
        n = int(np.prod(a.shape[1:]))
        Tn = 7
        def parent(shape, seed):                  # (finite new data)
            return torch.nan_to_num(_random(shape, tdt, seed), nan=0.5, posinf=1.0, neginf=-1.0)
        layouts = {
            "contiguous": (parent((Tn, n), n), (n, 1)),
            "padded rows": (parent((Tn, n + 7), n + 1)[:, 3:3 + n], (n + 7, 1)),
            "time fast": (parent((n, Tn), n + 2).T, (1, Tn)),
            "field shaped": (parent((Tn,) + a.shape[1:], n + 3), None),
        }
        for what, (x, strides) in layouts.items():
            assert strides is None or x.stride() == strides
            xn = x.cpu().numpy()
            before = x.clone()
            for mode in ("torch", "numpy"):
                m._output = mode
                got = m.predict(**{key: x}, n=3)[key]
                want = m.predict(**{key: xn}, n=3)[key]
                if mode == "torch":
                    assert isinstance(got, torch.Tensor) and got.device.type == "cuda" and isinstance(want, torch.Tensor)
                    got, want = got.cpu().numpy(), want.cpu().numpy()
                assert isinstance(got, np.ndarray) and got.shape == (Tn, 3)
                assert np.array_equal(got, want), (kind, key, what, mode)
            m._output = "torch"
            assert torch.equal(x, before)
    assert m._vectors_resident() == resident
    with pytest.raises(ValueError, match="Did you forget the time dimension"):
        m.predict(left=_random((int(np.prod(arrays[0].shape[1:])),), tdt, seed=1))


# ----------------------------------------------------------------------------------------------
# errors
# ----------------------------------------------------------------------------------------------
def test_constructor_errors():
    h = _handle(0)
    x = torch.zeros((8, 5), device=DEV)
    with pytest.raises(TypeError, match="int64"):
        MCA(torch.zeros((8, 5), dtype=torch.int64, device=DEV), handle=h)
    with pytest.raises(TypeError, match="different dtypes"):
        MCA(x, x.double(), handle=h)
    with pytest.raises(ValueError, match="1 dimension"):
        MCA(torch.zeros(8, device=DEV), handle=h)
    with pytest.raises(TypeError, match="mixed"):
        MCA(x, np.zeros((8, 5), dtype=np.float32), handle=h)
    with pytest.raises(TypeError, match="numpy.ndarray"):
        MCA(list(range(4)), handle=h)
    with pytest.raises(ValueError, match="output"):
        MCA(x, handle=h, output="cupy")
