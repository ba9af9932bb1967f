"""No GPU: the host side of tensor input and tensor output - which views of a tensor two strides express and which copy kernel
those strides select, the `output=` keyword, CPU tensors as numpy input, and the C ABI (same number, new symbols)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from abi_cases import check_entry, header_abi_version, header_define   # noqa: E402
from xmca_amd import _hip                                       # noqa: E402
from xmca_amd.array import MCA, _flat_strides, _tensor_np_dtype  # noqa: E402

NEW_SYMBOLS = ["xmca_set_field_strided", "xmca_ingest_regime", "xmca_get_maps_to", "xmca_reconstruct_to", "xmca_correlation_maps_to",
               "xmca_predict_strided"]
ROWS, TRANSPOSE, GATHER = _hip.INGEST_ROWS, _hip.INGEST_TRANSPOSE, _hip.INGEST_GATHER


def _strides(t):
    return _flat_strides(tuple(t.shape), tuple(t.stride()))


def _regime(t):
    st, sn = _strides(t)
    n = 1
    for d in t.shape[1:]:
        n *= d
    return _hip.ingest_regime(t.shape[0], n, st, sn)


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_views_two_strides_express(device):
    big = torch.empty((40, 137), device=device)
    cube = torch.empty((5, 7, 30), device=device)                # (lat, lon, time)
    cases = [
        (big, (137, 1), ROWS),
        (big[:, 3:134], (137, 1), ROWS),                         # padded rows
        (big[::2], (274, 1), ROWS),
        (big.T, (1, 137), TRANSPOSE),                            # a (space, time) array handed over transposed
        (big[5:, 2:9].T, (1, 137), TRANSPOSE),
        (big[::2, ::3], (274, 3), GATHER),
        (big.T[:, ::2], (1, 274), TRANSPOSE),
        (cube.permute(2, 0, 1), (1, 30), TRANSPOSE),             # both spatial strides collapse: 7 * 30 = 210
        (cube.permute(2, 0, 1)[::3], (3, 30), GATHER),
        (torch.empty((30, 5, 7), device=device), (35, 1), ROWS),
        (torch.empty((30, 5, 8), device=device)[:, :1, :7], (40, 1), ROWS),
        (torch.empty((30, 1, 7), device=device).expand(30, 1, 7), (7, 1), ROWS),      # dimensions of one element do not count
        (torch.empty((30, 7, 1), device=device), (7, 1), ROWS),
        (torch.empty((30, 1), device=device), (1, 1), ROWS),
    ]
    for t, want, regime in cases:
        assert _strides(t) == want, (tuple(t.shape), t.stride())
        assert _regime(t) == regime, (tuple(t.shape), t.stride())


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_views_that_need_contiguous(device):
    cube = torch.empty((30, 6, 8), device=device)
    for t in (cube[:, :, 1:7],                                   # rows of 6 in a pitch of 8: the spatial strides do not collapse
              cube[:, ::2],
              cube.permute(0, 2, 1),
              torch.empty((6, 30, 8), device=device).permute(1, 0, 2)):
        assert _strides(t) is None, (tuple(t.shape), t.stride())
        assert _strides(t.contiguous()) == (t[0].numel(), 1)
    assert _flat_strides((30,), (1,)) is None                    # no spatial dimension
    assert _flat_strides((4, 5), (5, -1)) is None                # (numpy can hand these over, torch cannot)


def test_regime_of_degenerate_views():
    assert _hip.ingest_regime(8, 1, 3, 99) == ROWS               # one column: its stride means nothing
    assert _hip.ingest_regime(1, 8, 99, 4) == TRANSPOSE          # one row
    assert _hip.ingest_regime(8, 8, 0, 1) == ROWS                # an expanded row
    assert _hip.ingest_regime(8, 8, 1, 1) == ROWS
    assert _hip.ingest_regime(8, 8, 16, 2) == GATHER
    for bad in [(0, 4, 4, 1), (4, 0, 1, 1), (4, 4, -4, 1), (4, 4, 4, -1)]:
        with pytest.raises(ValueError):
            _hip.ingest_regime(*bad)


def test_device_view_validates():
    v = _hip.DeviceView(4096, 3, 4, 4, 1, np.float32)
    assert v.shape == (3, 4) and v.dtype == np.float32
    with pytest.raises(TypeError):
        _hip.DeviceView(4096, 3, 4, 4, 1, np.int32)
    with pytest.raises(ValueError):
        _hip.DeviceView(4096, 3, 4, -4, 1, np.float32)
    assert _tensor_np_dtype(torch.empty(1, dtype=torch.float64)) == np.float64
    assert _tensor_np_dtype(torch.empty(1, dtype=torch.bfloat16)) is None


def test_output_keyword_and_cpu_tensors():
    a = np.random.default_rng(0).standard_normal((12, 3, 4)).astype(np.float32)
    a[:, 1, 2] = np.nan
    ref = MCA(a, preprocess="host")
    assert ref._output == "numpy"
    m = MCA(torch.from_numpy(a), preprocess="host")              # a CPU tensor is its numpy array
    assert m._output == "numpy"
    for k in ("_field_means", "_field_stds", "_no_nan_index", "_fields_store"):
        assert np.array_equal(getattr(m, k)["left"], getattr(ref, k)["left"], equal_nan=True), k
    assert m._shape == ref._shape and m._fields_spatial_shape == ref._fields_spatial_shape
    assert isinstance(m.fields()["left"], np.ndarray)
    two = MCA(torch.from_numpy(a), a[:, 0], preprocess="host")   # tensors and arrays on the host mix freely
    assert two._keys == ["left", "right"]
    for bad in ("cupy", "Torch", 1):
        with pytest.raises(ValueError, match="output"):
            MCA(a, preprocess="host", output=bad)
    assert MCA(a, preprocess="host", output="numpy")._output == "numpy"
    assert MCA(a, preprocess="host", output="torch")._output == "torch"
    with pytest.raises(TypeError, match="numpy.ndarray"):
        MCA(list(range(4)), preprocess="host")
    with pytest.raises(ValueError, match="Time dimensions"):
        MCA(torch.from_numpy(a), torch.from_numpy(a[:5]), preprocess="host")


def test_abi_number_and_new_symbols():
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version()
    for name in NEW_SYMBOLS:
        check_entry(name)
    # the wrappers kept their signatures: the new entry points add one trailing memory-space argument (predict: strides + space)
    sig = _hip.SIGNATURES
    assert sig["xmca_get_maps_to"][1][:-1] == sig["xmca_get_maps"][1]
    assert sig["xmca_reconstruct_to"][1][:-1] == sig["xmca_reconstruct_weighted"][1]
    assert sig["xmca_correlation_maps_to"][1][:-1] == sig["xmca_correlation_maps"][1]
    assert len(sig["xmca_predict_strided"][1]) == len(sig["xmca_predict_weighted"][1]) + 3
    for name, value in (("XMCA_INGEST_ROWS", ROWS), ("XMCA_INGEST_TRANSPOSE", TRANSPOSE), ("XMCA_INGEST_GATHER", GATHER)):
        assert header_define(name) == value
