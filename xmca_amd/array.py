"""`xmca_amd.array.MCA` - drop-in for `xmca.array.MCA` with solve()/rotate()/rule_n() on the MI355X.

Host side (this file, numpy): validation, flattening, NaN masking, centering, weights, getters, IO - the same
public methods, argument meanings, state attributes and exceptions as xmca/array.py (v1.4.2), so the
reference's tests read the same against this class.
Device side (libxmca_hip.so through `_hip.Handle`): the numerical core of
  * `solve`   xmca/array.py:549-584   (per-field SVD, kernel, kernel SVD, back-projection)
  * `rotate`  xmca/array.py:821-823 + xmca/tools/rotation.py (Varimax/Promax loop)
  * `rule_n`  xmca/array.py:1753-1765 (surrogate loop; run-sharded over ranks when torch.distributed is up)
  * `predict` xmca/array.py:1299-1428 and `reconstructed_fields` :1263-1292 (products over the resident vectors; the host route
    remains for other dtypes and models without device vectors)
There is no numpy fallback for these three: without the library or a GPU they raise.
"""
import cmath
import os
import sys
import warnings
from datetime import datetime

import numpy as np

from . import __version__, _hip
from .tools.array import (block_bootstrap, get_nan_cols, has_nan_time_steps, pearsonr, remove_mean, remove_nan_cols)

_SCALINGS_MSG = ('The scaling option {:} is not valid. Please choose one of the following: None, eigen, std, max')
# `scaling` of the spatial getters -> the divisor `xmca_get_maps` computes ('eigen' is a per-column factor, not a divisor)
_MAP_SCALINGS = {'None': _hip.SCALE_NONE, 'eigen': _hip.SCALE_NONE, 'max': _hip.SCALE_MAX, 'std': _hip.SCALE_STD}


def _two_sided_p(r, n_obs):
    """Two-sided p-value of a Pearson correlation under the exact null distribution, as tools/array.py:86-88:
    `2 * scipy.stats.beta(n/2 - 1, n/2 - 1, loc=-1, scale=2).cdf(-abs(r))` = 2 I_{(1-|r|)/2}(n/2 - 1, n/2 - 1): the same regularised
    incomplete beta function (bit for bit) without the frozen distribution's argument handling.  The function itself is what
    `homogeneous_patterns` costs on the host (18 of 21.7 ms at C2 for 10^5 values; it holds the GIL, so threads do not help)."""
    import scipy.special
    a = n_obs / 2 - 1
    # |r| an ulp above 1 (correlations summed in another order than the variances) is |r| = 1, p = 0; NaN stays NaN
    x = np.clip((1.0 - np.abs(np.asarray(r, dtype=np.float64))) / 2, 0.0, 1.0)
    return 2 * scipy.special.betainc(a, a, x)


def _predict_mix(svals, R_inv_t, var_idx, n_rot, n):
    """m x q mix of MCA.predict: pcs = x V[:, :m] W reproduces the reference's `(x @ V[:, :n_rot] / sqrt(s[:n_rot])) @ R` followed
    by `[:, var_idx][:, :n]` (array.py:1299-1428) with W = diag(1 / sqrt(s[:n_rot])) R^-H[:, var_idx][:, :n], R^-H the
    `rotation_matrix(inverse_transpose=True)`.  Trailing rows of W that are zero (modes no selected column mixes in, e.g. an
    unrotated model asked for n < rank modes) are dropped, so m <= n_rot vectors enter the product."""
    W = (R_inv_t / np.sqrt(svals[:n_rot])[:, None])[:, var_idx][:, :n]
    used = np.flatnonzero(np.any(W != 0, axis=1))           # (a NaN row is used: it propagates as the reference's does)
    return W[:used[-1] + 1] if used.size else W[:1]


def _rotated_mix(svals, R, norm, var_idx, keep):
    """m x q mix A of the rotated vectors: V_rot = V[:, :m] A with A = (diag(sqrt(s)) R / norm)[:, var_idx][:, keep], m = len(s)
    (`_get_V`, array.py:615-646).  Used by the device EOFs and the reconstruction."""
    return ((np.sqrt(svals)[:, None] * R) / norm)[:, var_idx][:, keep]


def _reconstruct_coefficients(P, A):
    """T x m coefficients B = P A^H of the reconstruction: (P @ V_rot^H).real = Re(B V[:, :m]^H) for V_rot = V[:, :m] A, with P the
    PCs in 'eigen' scaling (array.py:1263-1292)."""
    return P @ A.conj().T


def _is_int(x):
    """A python or numpy integer that is not a bool."""
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def _torch():
    """torch when the process has imported it, else None: a tensor can only be handed over by code that has."""
    return sys.modules.get('torch')


def _is_tensor(x):
    torch = _torch()
    return torch is not None and isinstance(x, torch.Tensor)


def _tensor_np_dtype(t):
    """numpy dtype of a tensor's elements, or None when numpy has no such dtype (bfloat16)."""
    try:
        return np.dtype(str(t.dtype).replace('torch.', ''))
    except TypeError:
        return None


def _flat_strides(shape, strides):
    """Element strides (stride_t, stride_n) of the (T, N) view of an array of `shape` / `strides` (time first, the spatial
    dimensions flattened in C order), or None when no two strides express it - the caller then makes the array contiguous.  The
    spatial dimensions collapse when each one's stride is the next one's stride times its length; dimensions of one element do
    not count, and neither does a negative stride."""
    if len(shape) < 2 or any(st < 0 for st in strides):
        return None
    dims = [(n, st) for n, st in zip(shape[1:], strides[1:]) if n != 1]
    for (_, st), (n_next, st_next) in zip(dims, dims[1:]):
        if st != st_next * n_next:
            return None
    return int(strides[0]), int(dims[-1][1]) if dims else 1


def _numpy_result(model, name, *args, **kwargs):
    """Public getter `name` of `model` - as `model` resolves it: a subclass's override, or the base class's for the numpy view a
    facade passes as `self` - with numpy results whatever the model's `output` says: what the numpy code of another getter
    builds on."""
    output = getattr(model, '_output', 'numpy')
    model._output = 'numpy'
    try:
        return getattr(model, name)(*args, **kwargs)
    finally:
        model._output = output


def _device_view(t, owner=None):
    """`_hip.DeviceView` of a real float32 / float64 GPU tensor flattened to (T, N): as it lies in memory when two strides
    express that view, else of a copy torch makes contiguous on the device."""
    if t.dim() == 1:
        t = t.unsqueeze(1)
    flat = _flat_strides(tuple(t.shape), tuple(t.stride()))
    if flat is None:
        t = t.contiguous()
        flat = _flat_strides(tuple(t.shape), tuple(t.stride()))
    n = 1
    for d in t.shape[1:]:
        n *= int(d)
    return _hip.DeviceView(t.data_ptr(), t.shape[0], n, flat[0], flat[1], _tensor_np_dtype(t), owner=t if owner is None else owner)


class _LazyVectors(dict):
    """`MCA._V` after solve(): (N', rank) singular vectors per field, fetched from the device when first read.  `head`
    fetches only the leading modes while the full array has not been asked for.  After `solve(n_modes=k)` `rank` is k: the
    device holds no further vectors."""

    def __init__(self, dev, where, rank, dtype):
        super().__init__({k: None for k in where})
        self._dev, self._where, self._rank, self._dtype = dev, dict(where), rank, dtype
        self._pending = set(where)

    def _load(self, k):
        if k in self._pending:
            side, n_k = self._where[k]
            dict.__setitem__(self, k, self._dev.vectors(side, self._rank, n_k, self._dtype).T)   # view of the mode-major result
            self._pending.discard(k)

    def materialize(self):
        for k in list(self._pending):
            self._load(k)

    def head(self, k, m):
        if k in self._pending:
            side, n_k = self._where[k]
            m = self._rank if m is None else min(m, self._rank)
            if m < self._rank:
                return self._dev.vectors(side, m, n_k, self._dtype).T
            self._load(k)
        return dict.__getitem__(self, k)[:, :m]

    def __getitem__(self, k):
        self._load(k)
        return dict.__getitem__(self, k)

    def __setitem__(self, k, v):
        self._pending.discard(k)
        dict.__setitem__(self, k, v)

    def get(self, k, default=None):
        return self[k] if k in self else default

    def items(self):
        self.materialize()
        return dict.items(self)

    def values(self):
        self.materialize()
        return dict.values(self)


class _RawField:
    """Stand-in for a field that was preprocessed on the device (MCA(..., preprocess='device')): the raw input, the
    mask of its NaN-free columns, and the shape / dtype the centered field has."""

    def __init__(self, raw, keep, tensor=None):
        self._raw = raw
        self.tensor = tensor     # a field handed over as a GPU tensor: kept for the recompute fallback only (`raw`)
        self.keep = keep
        self.shape = ((raw if tensor is None else tensor).shape[0], int(np.count_nonzero(keep)))
        self.dtype = raw.dtype if tensor is None else _tensor_np_dtype(tensor)
        self.ops = []            # (divide, per-column factors) applied on the device after centering, in order

    @property
    def raw(self):
        if self._raw is None:    # (the tensor as it is NOW: the model only owns the centered copy on the device)
            self._raw = self.tensor.detach().reshape(self.tensor.shape[0], -1).cpu().numpy()
        return self._raw

    @property
    def real(self):
        return self

    def kept_columns(self):
        return self.raw if self.shape[1] == self.raw.shape[1] else self.raw[:, self.keep]

    def centered(self):
        """What the device holds, recomputed on the host."""
        f = np.ascontiguousarray(remove_mean(self.kept_columns()))
        for divide, w in self.ops:
            f = f / w if divide else f * w
        return f


class MCA:
    """Maximum Covariance Analysis of one (EOF/PCA) or two fields - `numpy.ndarray`s or `torch.Tensor`s; time is axis 0."""

    def __init__(self, *fields, handle=None, preprocess=None, output=None):
        """fields: one or two numpy arrays or `torch.Tensor`s, time first.  `handle`: a `_hip.Handle` (default: one per device).
        `preprocess` (extension): where the constructor's NaN-column / mean / std / centering passes (array.py:191-215)
        run.  `'device'`: on the GPU over the uploaded raw field - column means in float64 - and the centered field stays
        resident for solve(); the host copy `_fields` is fetched on first use.  `'host'`: the reference's numpy path
        (bit-identical means for float32 input).  Default (None): `'device'` when a GPU is visible and the fields are
        plain real float32 / float64 arrays of one dtype, `'host'` otherwise (XMCA_PREPROCESS=host|device overrides).
        Tensors (extension): a CPU tensor is taken as its numpy array.  Real float32 / float64 tensors on the handle's GPU, of one
        dtype and with a spatial dimension, never visit the host: the library copies them, in whatever strided layout they have,
        into its own buffer (`xmca_set_field_strided`) and preprocesses them there; the tensor is neither written nor needed
        afterwards.  `output`: `'numpy'` or `'torch'` - what the getters that return dicts of arrays return; with `'torch'` they
        are tensors on the handle's GPU, and the field-sized ones (eofs, spatial_amplitude, spatial_phase, reconstructed_fields,
        homogeneous / heterogeneous_patterns) are written there by the device.  Spectra stay numpy.  Default: `'torch'` when a
        field is a GPU tensor, else `'numpy'`."""
        if preprocess is None:
            preprocess = os.environ.get('XMCA_PREPROCESS') or 'auto'
        if preprocess not in ('host', 'device', 'auto'):
            raise ValueError("preprocess must be 'host' or 'device'")
        if preprocess == 'auto':
            preprocess = 'device' if (handle is not None or _gpu_visible()) else 'host'
        if len(fields) > 2:
            raise ValueError("Too many fields. Pass 1 or 2 fields.")
        if len(fields) == 2 and fields[0].shape[0] != fields[1].shape[0]:
            raise ValueError('''Time dimensions of given fields are different.
                Time series should have same time lengths.''')
        if output not in (None, 'numpy', 'torch'):
            raise ValueError("output must be 'numpy' or 'torch'")
        fields = tuple(f.detach().numpy() if _is_tensor(f) and f.device.type == 'cpu' else f for f in fields)
        if not all(isinstance(f, np.ndarray) or _is_tensor(f) for f in fields):
            raise TypeError('''One or more fields are not `numpy.ndarray`.
            Please provide `numpy.ndarray` only.''')
        self._handle_override = handle
        on_gpu = any(_is_tensor(f) for f in fields)
        if on_gpu:
            self._check_gpu_tensors(fields)
            if preprocess != 'device':                       # an explicit 'host': the reference's numpy path on a host copy
                fields = tuple(f.detach().cpu().numpy() for f in fields)
        self._output = output or ('torch' if on_gpu else 'numpy')
        if self._output == 'torch':
            try:
                import torch      # noqa: F401
            except ImportError as err:
                raise ValueError("output='torch' needs PyTorch") from err
        self._preprocess = preprocess
        self._store_is_raw = False
        self._keys = ['left', 'right']
        if len(fields) == 1:
            self._keys.pop()
        self._fields_store = {}
        self._pending_hilbert = False
        self._device_hilbert = False
        self._device_extend = None          # period of extend='exp' when the device applies the extended operator
        self._device_theta = None           # season length of extend='theta' when the device fits and applies the extension
        self._upload_serial = 0
        self._token = object()              # identity of this model as owner of a handle's resident fields (never reused, unlike id())
        self._shape = {}
        self._field_names = {}
        self._field_means = {}
        self._field_stds = {}
        self._fields_spatial_shape = {}
        self._n_variables = {}
        self._no_nan_index = {}
        self._n_observations = {}

        data = {k: f for k, f in zip(self._keys, fields)}
        if not (preprocess == 'device' and self._ingest_on_device(data)):
            if any(_is_tensor(f) for f in fields):           # no NaN-free column: the host path raises the reference's errors
                fields = tuple(f.detach().cpu().numpy() for f in fields)
                data = {k: f for k, f in zip(self._keys, fields)}
            if any(has_nan_time_steps(f) for f in fields):
                raise ValueError('''One or more fields contain NaN time steps.
            Please remove these prior to analysis.''')
            self._ingest(data)

        self._analysis = {
            'version': __version__,
            'is_bivariate': len(self._fields_store) > 1,
            'is_normalized': False,
            'is_coslat_corrected': False,
            'method': 'pca',
            'is_complex': False,
            'extend': False,
            'theta_period': 365,
            'is_rotated': False,
            'n_rot': 0,
            'power': 0,
            'is_truncated': False,
            'is_truncated_at': 0,
            'rank': 0,
            'total_covariance': 0.0,
            'total_squared_covariance': 0.0,
        }
        self._analysis['method'] = self._get_method_id()

    # ------------------------------------------------------------------------------------------
    # `_fields`: the reference replaces it by the analytic signal inside solve(complexify=True)
    # (array.py:546-547).  The device only needs the real field, so the host copy of the analytic signal is
    # materialised lazily, the first time anything reads `_fields`.
    # ------------------------------------------------------------------------------------------
    @property
    def _fields(self):
        if self._store_is_raw:
            self._materialize_fields()
        if self._pending_hilbert:
            if getattr(self, '_device_theta', None) is not None:
                self._fields_store = self._fetch_analytic_fields()            # the signal the device solved: its planes
            elif getattr(self, '_device_extend', None) is not None:
                self._fields_store = self._complexify(self._fields_store)     # the reference's own extension (array.py:429-472)
            else:
                from scipy.signal import hilbert
                self._fields_store = {k: hilbert(f.real, axis=0) for k, f in self._fields_store.items()}
            self._pending_hilbert = False
        return self._fields_store

    def _device_extension(self):
        """True when the last solve complexified with a fore/back-cast extension applied on the device ('exp' or 'theta')."""
        return getattr(self, '_device_extend', None) is not None or getattr(self, '_device_theta', None) is not None

    def _fetch_analytic_fields(self):
        """extend='theta': the analytic signal as the device formed it - the real fields in float64 and the imaginary planes
        G0 X + B C fetched from the handle.  When something else has used the handle since the solve, the fields go up and are
        extended there again first (the fits of a column are the same bits on every call)."""
        dev = self._resident_device()
        store = self._fields_store
        return {k: np.asarray(store[k].real, dtype=np.float64) + 1j * dev.get_field_imag(side, store[k].shape)
                for side, k in enumerate(self._keys)}

    def _real_fields(self):
        """Real parts of `_fields` without materialising a pending analytic signal on the host.  extend='exp' / 'theta': float64, as
        the reference's real part of its complex128 signal (the imaginary part never enters the replicates of `bootstrapping`)."""
        if not (self._pending_hilbert and self._device_extension()):
            return {k: x.real for k, x in self._get_X(original_scale=False).items()}
        if self._store_is_raw:
            self._materialize_fields()
        return {k: np.array(f.real, dtype=np.float64) for k, f in self._fields_store.items()}

    @_fields.setter
    def _fields(self, value):
        self._fields_store = value
        self._pending_hilbert = False
        self._store_is_raw = False
        self._upload_serial = getattr(self, '_upload_serial', 0) + 1    # whatever the device still holds is stale now

    def _owner_key(self):
        if not hasattr(self, '_token'):          # models built without __init__ (bench / load flows)
            self._token = object()
        return (self._token, self._upload_serial)

    def _owns_device_fields(self, dev):
        return getattr(dev, 'fields_owner', None) == self._owner_key()

    def _resident_device(self):
        """The handle, with the fields `solve()` works on resident: they go up again when another model, `rule_n` or a bootstrap
        has used the handle in between."""
        dev = self._device()
        if not self._owns_device_fields(dev):
            self._upload_serial += 1
            self._upload_fields(dev)
        return dev

    def _kept_columns(self, k):
        """(indices of the kept columns of field k, or None when none is masked; its full width)."""
        mask = self._no_nan_index[k]
        return (None if mask.all() else np.flatnonzero(mask)), mask.size

    def _ingest_on_device(self, data):
        """preprocess='device': upload the raw fields, drop their NaN columns and center them there, keep them resident.
        False (nothing changed) when the fields are not plain real float32/float64 arrays of one dtype, or when a
        field has no NaN-free column (the host path then raises the reference's errors)."""
        if len(data) == 0:
            return False
        tensors = any(_is_tensor(f) for f in data.values())          # (all of them then: `_check_gpu_tensors`)
        dtypes = {_tensor_np_dtype(f) if tensors else np.dtype(f.dtype) for f in data.values()}
        if len(dtypes) != 1 or next(iter(dtypes)) not in (np.dtype(np.float32), np.dtype(np.float64)):
            return False
        dev = self._device()
        if tensors:
            # GPU tensors: flattened to (T, N) as strided views of their own memory (or of a contiguous copy torch makes) and
            # copied by the device; first wait for whatever produces them on the caller's stream - the library works on its own
            flat = {k: _device_view(f.detach()) for k, f in data.items()}
            _torch().cuda.current_stream(dev.device).synchronize()
        else:
            flat = {k: np.ascontiguousarray(f.reshape(f.shape[0], int(np.prod(f.shape[1:])))) for k, f in data.items()}
        stats, keep = {}, {}
        for side, k in enumerate(self._keys):
            if tensors:
                dev.set_field_strided(side, flat[k])
            else:
                dev.set_field(side, flat[k])
            keep[k], n_keep = dev.compact_field(side, flat[k].shape[1])      # array.py:191-197 on the device
            if n_keep == 0:
                dev.fields_owner = None
                return False
            stats[k] = dev.center_field(side, n_keep)
        self._set_field_meta(data)
        store = {}
        for k, f in flat.items():
            self._no_nan_index[k] = keep[k]
            self._field_means[k] = stats[k][0].astype(f.dtype, copy=False)
            self._field_stds[k] = stats[k][1].astype(f.dtype, copy=False)
            store[k] = _RawField(None, keep[k], tensor=data[k].detach()) if tensors else _RawField(f, keep[k])
        self._fields_store = store              # stand-ins: only shape / dtype are read while `_store_is_raw`
        self._store_is_raw = True
        dev.fields_owner = self._owner_key()
        return True

    def _materialize_fields(self):
        """Host copy of the centered fields of a device-preprocessed model: downloaded while the device still holds them,
        otherwise recomputed from the raw input."""
        dev = self._device()
        if self._owns_device_fields(dev):
            store = {k: dev.get_field(side, self._fields_store[k].shape, self._fields_store[k].dtype)
                     for side, k in enumerate(self._keys)}
        else:
            store = {k: f.centered() for k, f in self._fields_store.items()}
        self._fields_store = store
        self._store_is_raw = False

    def _device(self):
        return self._handle_override or _hip.default_handle()

    def _check_gpu_tensors(self, fields):
        """The fields that may take the device route: all of them real float32 / float64 tensors of one dtype on the handle's GPU,
        each with a spatial dimension.  Anything else says what is wrong."""
        dev = self._device()
        for f in fields:
            if not _is_tensor(f):
                raise TypeError('Fields on the GPU and on the host cannot be mixed: pass tensors of one device, or arrays.')
            if f.device.type != 'cuda' or f.device.index != dev.device:
                raise ValueError('A field is on {:}, the handle works on GPU {:}. Move the tensor, or pass a handle of its '
                                 'device.'.format(f.device, dev.device))
            if _tensor_np_dtype(f) not in (np.dtype(np.float32), np.dtype(np.float64)):
                raise TypeError('A GPU tensor field has dtype {:}: only real float32 and float64 tensors are '
                                'supported.'.format(f.dtype))
            if f.dim() < 2:
                raise ValueError('A GPU tensor field has {:} dimension(s): time and at least one spatial dimension are '
                                 'needed.'.format(f.dim()))
        if len({f.dtype for f in fields}) != 1:
            raise TypeError('The GPU tensor fields have different dtypes ({:}): both must be float32 or both '
                            'float64.'.format(', '.join(str(f.dtype) for f in fields)))

    # ------------------------------------------------------------------------------------------
    # output='torch': results as tensors on the handle's GPU
    # ------------------------------------------------------------------------------------------
    def _alloc(self):
        """None for numpy results; for torch results the allocator the device routes write through (`_hip.Handle.maps`): a new
        tensor on the handle's GPU and its address.  torch's allocator may hand out memory that work queued on the caller's stream
        still uses, so that stream is drained first; the library's call synchronises its own stream before it returns."""
        if getattr(self, '_output', 'numpy') != 'torch':
            return None
        import torch
        device = torch.device('cuda', self._device().device)
        torch.cuda.current_stream(device).synchronize()

        def alloc(shape, dtype):
            t = torch.empty(tuple(int(n) for n in shape), dtype=getattr(torch, np.dtype(dtype).name), device=device)
            return t, t.data_ptr()
        return alloc

    def _deliver(self, result):
        """A getter's dict (or tuple of dicts) in the model's output type: numpy arrays become tensors on the handle's GPU when
        it is 'torch' (the results that were computed on the host); tensors pass."""
        if getattr(self, '_output', 'numpy') != 'torch':
            return result
        if isinstance(result, tuple):
            return tuple(self._deliver(r) for r in result)
        import torch
        device = torch.device('cuda', self._device().device)
        return {k: v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)).to(device)
                for k, v in result.items()}

    # ------------------------------------------------------------------------------------------
    # constructor helpers (array.py:191-240)
    # ------------------------------------------------------------------------------------------
    def _ingest(self, data):
        """meta, reshape to 2-D, NaN mask, mean/std, centering - in the reference's order (array.py:110-117)."""
        self._set_field_meta(data)
        data = self._reshape_to_2d(data)
        self._set_no_nan_idx(data)
        data = self._remove_nan_cols(data)
        self._set_field_means(data)
        self._set_field_stds(data)
        self._fields = self._center(data)

    def _set_field_meta(self, data):
        for k, field in data.items():
            shape = tuple(int(n) for n in field.shape)      # (a tensor's torch.Size as the tuple numpy has)
            self._shape[k] = shape
            self._n_observations[k] = shape[0]
            self._fields_spatial_shape[k] = shape[1:]
            self._n_variables[k] = int(np.prod(shape[1:]))
            self._field_names[k] = k

    def _reshape_to_2d(self, data):
        return {k: f.reshape(f.shape[0], int(np.prod(f.shape[1:]))) for k, f in data.items()}

    def _set_no_nan_idx(self, data):
        for k, f in data.items():
            self._no_nan_index[k] = ~get_nan_cols(f)

    def _remove_nan_cols(self, data):
        return {k: remove_nan_cols(f) for k, f in data.items()}

    def _set_field_means(self, data):
        for k, f in data.items():
            self._field_means[k] = f.mean(axis=0)

    def _set_field_stds(self, data):
        for k, f in data.items():
            self._field_stds[k] = f.std(axis=0)

    def _center(self, data):
        # time-major contiguous rows for the device upload (boolean column selection leaves a column-major layout; the
        # means above were taken on it, exactly like the reference, so the values are bit-identical)
        return {k: np.ascontiguousarray(remove_mean(f)) for k, f in data.items()}

    def _get_method_id(self):
        return 'mca' if self._analysis['is_bivariate'] else 'pca'

    def _get_slice(self, input):
        """int n -> slice(0, n); slice (1-based, inclusive stop) -> 0-based slice.  array.py:145-173"""
        if input is None or np.issubdtype(type(input), np.integer):
            return slice(0, self._analysis['rank'] if input is None else input)
        if isinstance(input, slice):
            start = 0 if input.start is None else max(0, input.start - 1)
            stop = self._analysis['rank'] if input.stop is None else min(input.stop, self._analysis['rank'])
            return slice(start, stop, input.step)
        raise ValueError('Invalid type {:}. Must be either int or slice.'.format(type(input)))

    def set_field_names(self, left='left', right='right'):
        """Names used in plots and saved files."""
        self._field_names['left'] = left
        self._field_names['right'] = right

    # ------------------------------------------------------------------------------------------
    # scaling helpers (array.py:264-315)
    # ------------------------------------------------------------------------------------------
    def _scale_X(self, data_dict):
        scaled = data_dict.copy()
        field = None
        k = None
        for k, field in scaled.items():
            field -= self._field_means[k]
        # as in the reference the normalisation sits outside the loop: only the LAST field is divided (array.py:269-272)
        if self._analysis['is_normalized'] and field is not None:
            field /= self._field_stds[k]
        return scaled

    def _scale_X_inverse(self, data_dict):
        for k, field in data_dict.items():
            if self._analysis['is_normalized']:
                field *= self._field_stds[k]
            field += self._field_means[k]
        return data_dict

    def _get_X(self, original_scale=False, real=False):
        X = {k: f.copy() for k, f in self._fields.items()}
        if real:
            X = {k: x.real for k, x in X.items()}
        if original_scale:
            X = self._scale_X_inverse(X)
        return X

    def _with_nan_columns(self, key, values, lead_shape):
        """re-insert the masked grid points: values (..., N') -> (..., N) filled with NaN."""
        out = np.zeros(lead_shape + (self._n_variables[key],), dtype=values.dtype) * np.nan
        out[..., self._no_nan_index[key]] = values
        return out

    def _get_fields(self, original_scale=False):
        n_obs = self._n_observations['left']
        fields = {}
        for k, X in self._get_X(original_scale=original_scale).items():
            full = self._with_nan_columns(k, X, (n_obs,))
            fields[k] = full.reshape((n_obs,) + self._fields_spatial_shape[k])
        return fields

    # ------------------------------------------------------------------------------------------
    # pre-processing
    # ------------------------------------------------------------------------------------------
    def apply_weights(self, left=None, right=None):
        """Multiply the (centered) fields by weights broadcastable to (T, N').  array.py:317-349"""
        weights = {'left': 1 if left is None else left, 'right': 1 if right is None else right}
        if self._scale_on_device({k: weights[k] for k in self._keys}, divide=False):
            return
        self._fields = {k: f * weights[k] for k, f in self._fields.items()}

    def normalize(self):
        """Divide every grid point's series by its standard deviation.  array.py:351-365"""
        if not self._scale_on_device({k: self._field_stds[k] for k in self._keys}, divide=True):
            fields = self._fields
            self._fields = {k: fields[k] / self._field_stds[k] for k in self._keys}
        self._analysis['is_normalized'] = True
        self._analysis['is_coslat_corrected'] = False
        self._analysis['method'] = self._get_method_id()

    def _scale_on_device(self, factors, divide):
        """Device-preprocessed model whose fields are still resident: per-column factors (scalars, (N',) or (1, N')
        arrays that do not change the dtype) are applied there.  False when the host path has to do it."""
        if not self._store_is_raw:
            return False
        dev = self._device()
        if not self._owns_device_fields(dev):
            return False
        cols = {}
        for k, w in factors.items():
            f = self._fields_store[k]
            if getattr(dev, 'field_dtype', None) not in (None, np.dtype(f.dtype)):
                return False                  # float32 fields promoted by an extend='exp' solve: the host path scales them
            w = np.asarray(w)
            if w.ndim > 2 or (w.ndim == 2 and w.shape[0] != 1) or np.iscomplexobj(w):
                return False
            orig = factors[k]
            weak = isinstance(orig, (int, float)) and not isinstance(orig, np.generic)     # python scalars do not promote
            if np.result_type(f.dtype, orig if weak else w.dtype) != f.dtype:
                return False
            try:
                cols[k] = np.ascontiguousarray(np.broadcast_to(w.reshape(-1) if w.ndim else w, (f.shape[1],)), dtype=f.dtype)
            except ValueError:
                return False
        # a complexified solve on the general path leaves an imaginary plane next to the resident real one; the real
        # plane is untouched and the next solve re-complexifies (the reference simply rescales `_fields`)
        dev.decomplexify()
        for side, k in enumerate(self._keys):
            dev.scale_field(side, cols[k], divide)
            self._fields_store[k].ops.append((divide, cols[k]))
        return True

    # ------------------------------------------------------------------------------------------
    # complexification on the host (only needed for extend != False, and lazily for the getters)
    # ------------------------------------------------------------------------------------------
    def _theta_forecast(self, series):
        try:
            from statsmodels.tsa.forecasting.theta import ThetaModel
        except Exception as err:          # statsmodels is an optional dependency
            raise ImportError("extend='theta' needs statsmodels") from err
        steps = len(series)
        model = ThetaModel(series, period=self._analysis['theta_period'], deseasonalize=True, use_test=False).fit()
        return model.forecast(steps=steps, theta=20)

    def _get_reg_coefs(self, x, y):
        assert x.shape[0] == y.shape[0]
        n = x.shape[0]
        xmean, ymean = np.mean(x, axis=0), np.mean(y, axis=0)
        xstd = np.mean(x, axis=0)      # sic: the reference uses the mean here (array.py:384); kept for parity
        cov = np.sum((x - xmean) * (y - ymean), axis=0) / n
        slope = cov / (xstd ** 2)
        return ymean - xmean * slope, slope

    def _exp_forecast(self, field):
        n = field.shape[0]
        x = np.repeat(np.arange(n)[:, np.newaxis], field.shape[1], axis=1)
        intercept, slope = self._get_reg_coefs(x, field)
        linear_end = slope * x[-1, :] + intercept
        offset = field[-1, :] - linear_end
        theta = self._analysis['theta_period']
        return offset * np.exp(-(x + 1) / theta) + (slope * x) + linear_end

    def _extend(self, field):
        extend = self._analysis['extend']
        if extend == 'theta':
            return np.array([self._theta_forecast(col) for col in field.T]).T
        if extend == 'exp':
            return self._exp_forecast(field)
        raise ValueError('''{:} is not a valid extension. Choose either
            `exp` or `theta`.'''.format(extend))

    def _complexify(self, fields):
        """Analytic signal along time (array.py:429-472), with optional fore/back-cast extension."""
        from scipy.signal import hilbert
        n_obs = self._n_observations['left']
        out = {}
        for k in self._keys:
            f = fields[k].real
            if self._analysis['extend']:
                post = self._extend(f)
                pre = self._extend(f[::-1])[::-1]
                f = np.concatenate([pre, f, post])
            f = hilbert(f, axis=0)
            if self._analysis['extend']:
                f = remove_mean(f[n_obs:(2 * n_obs)])
            out[k] = f
        return out

    # ------------------------------------------------------------------------------------------
    # solve (array.py:509-603) - numerical core on the device
    # ------------------------------------------------------------------------------------------
    def solve(self, complexify=False, extend=False, period=1, n_modes=None):
        """EOF analysis / MCA: singular value decomposition of the (cross-)covariance matrix.

        complexify : Hilbert-transform the fields first (complex EOF/MCA).
        extend     : False, 'exp' or 'theta' - fore/back-cast before the Hilbert transform.  Both run on the device in float64
                     (float32 fields are promoted; the result is complex128): 'exp' is one linear operator along time, 'theta'
                     fits every grid point there - additive seasonal means of season length `period`, drift, simple exponential
                     smoothing with alpha from a fixed grid zoom - and forecasts with theta = 20 as the reference does
                     (the Theta method restated from the published algorithm, not compared with statsmodels).
        period     : season length (theta: an integer >= 1, at most half the number of time steps) / e-folding time (exp).
        n_modes    : None - all modes - or an integer k >= 1 (extension): the model is left as `solve()` followed by
                     `truncate(k)` leaves it - k singular values and the vectors of k modes, the totals of the full spectrum - but
                     the device forms, back-projects and keeps the vectors of those k modes only, and nothing is fetched to the
                     host.  k at or above the rank is the same as None.  The values are the bits of `solve()` wherever
                     both take the same eigensolver; a field of numerical rank far below its length sends the full
                     `solve()` to Jacobi sweeps that the k leading vectors do not need, and the two then agree to
                     n eps sigma_1.
        """
        if n_modes is not None:
            if not _is_int(n_modes):
                raise ValueError('`n_modes` must be None or an integer >= 1, not {!r}'.format(n_modes))
            if n_modes < 1:
                raise ValueError('`n_modes` must be >= 1, not {!r}'.format(n_modes))
            n_modes = int(n_modes)
        if complexify and extend == 'theta':
            n_obs = self._n_observations.get('left', 0)
            if not _is_int(period) or period < 1:
                raise ValueError("`period` must be an integer >= 1 for extend='theta', not {!r}".format(period))
            if n_obs < 2 * period:
                raise ValueError("`period` = {:} needs at least 2 * period = {:} time steps for extend='theta'; the fields have "
                                 "{:}".format(period, 2 * period, n_obs))
            period = int(period)
        store = self._fields_store
        if len(store) == 0 or (not self._store_is_raw and any(np.isnan(f).all() for f in store.values())):
            raise RuntimeError('''
            Fields are empty. Did you forget to load data?
            ''')
        self._analysis['is_complex'] = complexify
        self._analysis['extend'] = extend
        self._analysis['theta_period'] = period
        if isinstance(getattr(self, '_V', None), _LazyVectors):
            del self._V                                              # vectors of an earlier solve still on the device: not wanted

        dev = self._device()
        # extend='exp' is a fixed linear operator along time (`_hip.extended_imag_parts`): X_im = G X on the device, in float64
        # like the reference; extend='theta' is fitted per column on the device and its forecast is linear in the fitted coefficients
        # (`_hip.theta_imag_parts`): X_im = G0 X + B C.  `_extend_on_host` (private) keeps the reference's host procedure for comparison
        on_host = getattr(self, '_extend_on_host', False)
        extend_exp = bool(complexify) and extend == 'exp' and not on_host
        extend_theta = bool(complexify) and extend == 'theta' and not on_host
        self._device_extend = period if extend_exp else None
        self._device_theta = period if extend_theta else None
        if complexify and extend and not (extend_exp or extend_theta):
            self._fields = self._complexify(self._fields)           # host path (`_extend_on_host`, or an unknown extension's error)
            self._device_hilbert = False
        elif self._store_is_raw:
            self._device_hilbert = bool(complexify)                  # centered real fields are resident already
            self._pending_hilbert = bool(complexify)
        else:
            real = {k: self._fields[k].real if np.iscomplexobj(self._fields_store[k]) else self._fields_store[k]
                    for k in self._keys}
            self._device_hilbert = bool(complexify)                  # X_im = Ht X (or G X) on the device
            if complexify:
                self._fields_store = real
                self._pending_hilbert = True                         # host copy of the analytic signal: on first use
            else:
                self._fields = real
        self._upload_fields(dev)

        # n_modes: the device is asked for that many modes' vectors only (all singular values come back in any case)
        full_rank = min(min(f.shape) for f in self._fields_store.values())
        n_vec = -1 if n_modes is None or n_modes >= full_rank else n_modes
        try:
            rank = dev.solve(len(self._keys), n_vec)
        except np.linalg.LinAlgError as err:                       # array.py:575-578 (the device message is the cause)
            raise np.linalg.LinAlgError('''SVD failed. NaN entries may be the problem.''') from err

        real_dtype = _real_dtype(next(iter(self._fields_store.values())).dtype)
        if extend_exp or extend_theta:
            real_dtype = np.float64                                  # float32 input is extended in float64 (complex128 result)
        singular_values = dev.singular_values(rank).astype(real_dtype, copy=False)
        # the vectors stay on the device until something reads them (233 MB at C2; pcs / eofs / rotate of a few modes
        # fetch just those modes); anything that would invalidate them on the handle makes this model fetch them first
        n_kept = rank if n_vec < 0 else min(n_vec, rank)
        self._V = _LazyVectors(dev, {k: (side, self._fields_store[k].shape[1]) for side, k in enumerate(self._keys)}, n_kept, real_dtype)
        dev.hold_result(self)

        self._singular_values = singular_values
        self._variance = singular_values
        self._var_idx = np.argsort(singular_values)[::-1]
        self._norm = {k: np.sqrt(singular_values) for k in self._keys}
        self._analysis['total_covariance'] = singular_values.sum()
        self._analysis['total_squared_covariance'] = (singular_values ** 2).sum()
        self._analysis['rank'] = len(singular_values)
        self._analysis['is_rotated'] = False
        self._analysis['n_rot'] = len(singular_values)
        self._analysis['power'] = 0
        # unrotated: both are the unit matrix (array.py:594-595) - built by rotation_matrix() / correlation_matrix() when
        # somebody asks (two rank x rank arrays are 400 MB at rank 5000, and rotate() would pay for freeing them)
        for name in ('_rotation_matrix', '_correlation_matrix'):
            if hasattr(self, name):
                delattr(self, name)
        self._analysis['is_truncated_at'] = len(singular_values)
        if n_kept < len(singular_values):
            # what truncate(n_kept) does to this state - without its fetch of every vector (there are no others to drop)
            self._singular_values = self._singular_values[:n_kept]
            self._analysis['is_truncated'] = True
            self._analysis['is_truncated_at'] = n_kept

    # ------------------------------------------------------------------------------------------
    # state accessors used by the getters (array.py:605-779)
    # ------------------------------------------------------------------------------------------
    def _get_svals(self, n=None):
        try:
            return self._singular_values[self._get_slice(n)]
        except AttributeError:
            raise RuntimeError('Cannot retrieve singular values. Please call the method `solve` first.')

    def _get_min_mode(self, n=None, rotated=False):
        cand = [self._analysis['rank']]
        if n is not None:
            cand.append(n)
        if rotated:
            cand.append(self._analysis['n_rot'])
        return np.min(cand)

    def _get_max_mode(self, n=None, rotated=False):
        cand = [self._analysis['rank'] if n is None else n]
        if rotated:
            cand.append(self._analysis['n_rot'])
        return np.max(cand)

    def _max_mode(self, n, rotated):
        if rotated:
            return self._analysis['n_rot']
        return n.stop if isinstance(n, slice) else n

    def _materialize_vectors(self):
        """Called by the handle before the device result this model still reads from is overwritten."""
        V = getattr(self, '_V', None)
        if isinstance(V, _LazyVectors):
            V.materialize()

    def _get_V(self, n=None, rotated=True):
        # an unrotated model: the reference multiplies all `rank` modes by sqrt(s) I / sqrt(s) and reorders them by the
        # (already descending) singular values - the identity; only the requested modes are touched here
        rotated = rotated and self._analysis['is_rotated']
        max_mode = self._max_mode(n, rotated)
        keep = self._get_slice(n)
        try:
            V = {k: (self._V.head(k, max_mode) if isinstance(self._V, _LazyVectors) else self._V[k][:, :max_mode]) for k in self._V}
        except AttributeError:
            raise RuntimeError('Cannot retrieve singular vectors. Please call the method `solve` first.')
        for k in self._keys:
            if rotated:
                sqrt_svals = np.sqrt(self._get_svals(max_mode))
                norm = self._get_norm(max_mode, sorted=False)
                V[k] = (V[k] * sqrt_svals @ self.rotation_matrix() / norm[k])[:, self._var_idx]
            V[k] = V[k][:, keep]
        return V

    def _upload_fields(self, dev):
        """Makes the fields solve() works on resident on the device and records this model as their owner."""
        T = self._n_observations['left']
        extend = getattr(self, '_device_extend', None)
        theta = getattr(self, '_device_theta', None)
        extended = self._device_extension()
        if self._store_is_raw:
            # (float32 fields promoted by an earlier extend='exp' / 'theta' solve are resident as float64: a plain solve uploads them again)
            same_dtype = getattr(dev, 'field_dtype', None) in (None, np.dtype(self._fields_store[self._keys[0]].dtype))
            if self._owns_device_fields(dev) and (extended or same_dtype):   # still resident: nothing to send
                if theta is not None:
                    dev.complexify_theta(T, theta)
                elif extend is not None:
                    dev.complexify_extended(T, extend)
                elif self._device_hilbert:
                    dev.complexify(T)
                else:
                    dev.decomplexify()
                return
            self._materialize_fields()                          # the handle was used elsewhere: recompute, then upload
        store = self._fields_store
        for side, k in enumerate(self._keys):
            dev.set_field(side, _device_ready(store[k]))
        if self._device_hilbert and not any(np.iscomplexobj(f) for f in store.values()):
            # (a materialised host analytic signal goes up as it is); the extended operator, never the plain Hilbert one, for
            # a model solved with extend='exp' / 'theta'
            if theta is not None:
                dev.complexify_theta(T, theta)
            elif extend is not None:
                dev.complexify_extended(T, extend)
            else:
                dev.complexify(T)
        dev.fields_owner = self._owner_key()

    def _project_on_device(self, V):
        """fields[k] @ V[k] of `_get_U` (array.py:391) as a device GEMM over the resident fields."""
        dev = self._resident_device()
        T = self._n_observations['left']
        if next(iter(V.values())).shape[1] == 0:          # pcs(0): nothing to project (bootstrapping's first iterative step)
            return {k: np.zeros((T, 0), dtype=V[k].dtype) for k in self._keys}
        return {k: dev.project(side, V[k], T) for side, k in enumerate(self._keys)}

    def _vectors_resident(self):
        """True while every vector of this model's last solve is still on the device only (nothing fetched, result held)."""
        V = getattr(self, '_V', None)
        return isinstance(V, _LazyVectors) and V._pending == set(self._keys) and self._device().holds_result_of(self)

    def _resident_dtype(self):
        """dtype the resident vectors have on the host (`_LazyVectors`): complex for a complex solve."""
        dt = self._V._dtype
        return np.result_type(dt, np.complex64) if self._analysis['is_complex'] else np.dtype(dt)

    def _project_resident(self, max_mode):
        """fields[k] @ V[k][:, :max_mode] of `_get_U` with the vectors still resident (xmca_project without V): nothing is fetched
        or uploaded again.  (None, None) when they are not resident - the caller then takes `_get_V`."""
        if not self._vectors_resident():
            return None, None
        dev = self._resident_device()
        if not self._vectors_resident():          # (an upload may have released the result)
            return None, None
        m = self._analysis['rank'] if max_mode is None else min(int(max_mode), self._analysis['rank'])
        m = min(m, self._V._rank)                 # (solve(n_modes=k): k modes are resident, as `_get_V` finds k after truncate(k))
        T = self._n_observations['left']
        vdt = {k: self._resident_dtype() for k in self._keys}
        if m < 1:
            return {k: np.zeros((T, 0), dtype=vdt[k]) for k in self._keys}, vdt
        return {k: dev.project(side, None, T, m, self._V._where[k][1]) for side, k in enumerate(self._keys)}, vdt

    def _get_U(self, n=None, rotated=True):
        keep = self._get_slice(n)
        mix = rotated and self._analysis['is_rotated']
        if mix:
            max_mode = self._max_mode(n, rotated)
        else:
            # the reference multiplies by the identity rotation matrix over all `rank` modes here (array.py:393); only
            # the kept modes are projected instead - same numbers, no T x N x rank product for pcs(10), and the
            # null modes (sigma = 0 exactly on the device) cannot leak 0 * inf into the kept columns
            max_mode = keep.stop if keep.stop is not None else self._analysis['rank']
        sqrt_svals = np.sqrt(self._get_svals(max_mode))
        XV, vdt = self._project_resident(max_mode)
        if XV is None:
            V = self._get_V(max_mode, rotated=False)
            XV = self._project_on_device(V)
            vdt = {k: V[k].dtype for k in self._keys}
        U = {}
        for k in self._keys:
            U[k] = XV[k].astype(np.result_type(vdt[k], self._fields_store[k].dtype), copy=False) / sqrt_svals
            if mix:
                R = self.rotation_matrix(inverse_transpose=True)
                U[k] = (U[k] @ R)[:, self._var_idx]
            U[k] = U[k][:, keep]
        return U

    def _get_norm(self, n=None, sorted=True):
        try:
            norm = self._norm
        except AttributeError:
            raise RuntimeError('Cannot retrieve field norms. Please call the method `solve` first.')
        if sorted:
            norm = {k: v[self._var_idx] for k, v in norm.items()}
        modes = self._get_slice(n)
        return {k: v[modes] for k, v in norm.items()}

    def _get_variance(self, n=None, sorted=True):
        norm = self._get_norm(n=n, sorted=sorted)
        if self._analysis['is_bivariate']:
            return norm['left'] * norm['right']
        return norm['left'] ** 2

    def _eofs_from_device(self, n, rotated):
        """(N' x q) array per field in its final memory layout, mixed on the device from the vectors still resident there
        (`xmca_get_eofs`), or None when they are not (then `_get_V`'s host path is taken).  Same numbers as `_get_V`:
        `(V sqrt(s)) @ R / norm`, columns ordered by explained variance, then the requested slice (array.py:615-646)."""
        mix = self._eof_mix(n, rotated)
        if mix is None:
            return None                                   # (vectors already on the host - or injected by a test: no device needed)
        dev = self._device()
        return {k: dev.eofs(side, n_k, m, W, dtype) for k, (side, n_k, m, W, dtype) in mix.items()}

    def _eof_mix(self, n, rotated):
        """Arguments of `xmca_get_eofs` / `xmca_get_maps` per field - (side, N', m, W, component dtype): the resident vectors
        V[:, :m], the m x q mix W (None: the first q = m vectors as they are) - or None when the vectors are not resident or the
        selection is empty."""
        if not self._vectors_resident():
            return None
        Vl = self._V
        rotated = rotated and self._analysis['is_rotated']
        max_mode = self._max_mode(n, rotated)
        max_mode = self._analysis['rank'] if max_mode is None else min(max_mode, self._analysis['rank'])
        max_mode = min(max_mode, Vl._rank)
        keep = self._get_slice(n)
        if max_mode < 1 or len(range(max_mode)[keep]) < 1:
            return None
        out = {}
        for side, k in enumerate(self._keys):
            n_k = Vl._where[k][1]
            if rotated:
                norm = self._get_norm(max_mode, sorted=False)
                W = _rotated_mix(self._get_svals(max_mode), self.rotation_matrix(), norm[k], self._var_idx, keep)
                out[k] = (side, n_k, max_mode, W, np.float64)
            else:
                cols = range(max_mode)[keep]
                if cols.start == 0 and cols.step == 1:
                    out[k] = (side, n_k, len(cols), None, Vl._dtype)
                else:
                    out[k] = (side, n_k, max_mode, np.eye(max_mode)[:, keep], Vl._dtype)
        return out

    def _maps_from_device(self, n, rotated, kind, scaling='None', phase_shift=0, alloc=None):
        """eofs() / spatial_amplitude() / spatial_phase() of every field in their final (space..., modes) arrays from the device
        (`xmca_get_maps`): phase shift and 'eigen' norms as per-column factors, 'max' / 'std' divisors, amplitude or phase and the
        NaN rows of the masked grid points, without a pass over N x q on the host.  The dtype of each result is worked out here with
        the promotions the numpy code below performs, and passed down.  None when the vectors are not resident, the selection is
        empty, `_maps_on_host` is set or a float32 / complex64 result is to be scaled by 'std': the caller then runs the numpy code.
        alloc (`_alloc`): the maps are written into tensors on the GPU and those returned."""
        if getattr(self, '_maps_on_host', False) or scaling not in _MAP_SCALINGS:
            return None
        mix = self._eof_mix(n, rotated)
        if mix is None:
            return None
        dev = self._device()
        cplx = self._analysis['is_complex']
        shift = cmath.rect(1, phase_shift) if cplx and phase_shift != 0 else None
        plan = {}
        for k, (side, n_k, m, W, dtype) in mix.items():
            q = m if W is None else W.shape[1]
            dt = np.result_type(dtype, np.complex64) if cplx or np.iscomplexobj(W) else np.dtype(dtype)
            factor = None
            if shift is not None:
                dt = (np.zeros(0, dtype=dt) * shift).dtype
                factor = np.full(q, shift)
            if scaling == 'eigen':
                norm = self._get_norm(q, sorted=True)[k]
                if norm.shape != (q,):
                    return None                           # (the numpy code raises numpy's own broadcasting error)
                dt = np.result_type(dt, norm.dtype)
                factor = norm if factor is None else factor * norm
            if scaling == 'std' and dt in (np.float32, np.complex64):
                # the reference's divisor of a float32 result is `np.nanstd` in float32: it adds the N' squares one after the other
                # in float32 and is off by 3e-5 at N' = 4e4, fifteen times the 2e-6 this class holds float32 results to against the
                # reference's arithmetic - the device's float64 sums would not be that number, so the numpy code keeps this case
                return None
            if kind != _hip.MAP_EOF:
                dt = np.zeros(0, dtype=dt).real.dtype
            plain = kind == _hip.MAP_EOF and factor is None and scaling == 'None' and self._n_variables[k] == n_k
            plan[k] = (side, n_k, m, W, dtype, factor, dt, plain)
        out = {}
        for k, (side, n_k, m, W, dtype, factor, dt, plain) in plan.items():
            if plain and alloc is None:
                full = dev.eofs(side, n_k, m, W, dtype)   # no mask, no scaling, no phase shift: `xmca_get_eofs` as it is
            else:                                         # (on the GPU the plain case is a map without options: the same bits)
                keep_idx, n_full = self._kept_columns(k)
                full = dev.maps(side, n_k, m, W, factor, keep_idx, n_full, kind, _MAP_SCALINGS[scaling], dt, alloc=alloc)
            out[k] = full.reshape(self._fields_spatial_shape[k] + (full.shape[1],))
        return out

    def _get_eofs(self, n=None, scaling='None', phase_shift=0, rotated=True, alloc=None):
        eofs = self._maps_from_device(n, rotated, _hip.MAP_EOF, scaling, phase_shift, alloc=alloc)
        if eofs is not None:
            return eofs
        V = self._eofs_from_device(n, rotated)
        fresh = V is not None                 # arrays of the device path are the caller's; `_get_V` may return views of `_V`
        if V is None:
            V = self._get_V(n, rotated=rotated)
        eofs = {}
        for k in self._keys:
            n_modes = V[k].shape[1]
            if self._n_variables[k] == V[k].shape[0] and fresh and V[k].flags['C_CONTIGUOUS']:
                full = V[k]                                                   # no masked points: the array is final as it is
            elif self._n_variables[k] == V[k].shape[0]:
                full = np.array(V[k], order='C')                              # (a copy: never the model's own vectors)
            else:
                full = np.full((self._n_variables[k], n_modes), np.nan, dtype=V[k].dtype)
                full[self._no_nan_index[k]] = V[k]                            # (N, n_modes), NaN at masked points
            eofs[k] = full.reshape(self._fields_spatial_shape[k] + (n_modes,))
            if self._analysis['is_complex'] and phase_shift != 0:
                eofs[k] = eofs[k] * cmath.rect(1, phase_shift)
            space_axes = tuple(range(eofs[k].ndim - 1))
            if scaling == 'None':
                pass
            elif scaling == 'eigen':
                eofs[k] = eofs[k] * self._get_norm(V[self._keys[0]].shape[1], sorted=True)[k]
            elif scaling == 'max':
                eofs[k] = eofs[k] / np.nanmax(abs(eofs[k].real), axis=space_axes)
            elif scaling == 'std':
                eofs[k] = eofs[k] / np.nanstd(eofs[k].real, axis=space_axes)
            else:
                raise ValueError(_SCALINGS_MSG.format(scaling))
        return eofs

    def _get_pcs(self, n=None, scaling='None', phase_shift=0, rotated=True):
        U = self._get_U(n, rotated=rotated)
        for k in self._keys:
            if self._analysis['is_complex']:
                U[k] = U[k] * cmath.rect(1, phase_shift)
            if scaling == 'None':
                pass
            elif scaling == 'eigen':
                U[k] = U[k] * self._get_norm(n, sorted=True)[k]
            elif scaling == 'max':
                U[k] = U[k] / np.nanmax(abs(U[k].real), axis=0)
            elif scaling == 'std':
                U[k] = U[k] / np.nanstd(U[k].real, axis=0)
            else:
                raise ValueError(_SCALINGS_MSG.format(scaling))
        return U

    # ------------------------------------------------------------------------------------------
    # rotate (array.py:781-844) - Varimax/Promax loop on the device
    # ------------------------------------------------------------------------------------------
    def rotate(self, n_rot, power=1, tol=1e-8):
        """Promax rotation of the first `n_rot` modes (`power=1`: Varimax).

        Raises ValueError for `n_rot < 2` / `power < 1`, RuntimeError when Varimax does not converge
        within 1000 iterations.
        """
        if n_rot < 2:
            raise ValueError('`n_rot` must be > 1')
        if power < 1:
            raise ValueError('`power` must be >=1')
        dev = self._device()
        V = getattr(self, '_V', None)
        if (isinstance(V, _LazyVectors) and V._pending == set(self._keys) and dev.holds_result_of(self)
                and n_rot <= self._analysis['rank'] and n_rot <= V._rank and (V._dtype == np.float64 or dev.vectors_are_f32(0))):
            # the vectors of solve() are still resident: the stacked loadings V sqrt(s) are built on the device.  float32
            # models: the reference rotates float32 loadings (float32 vectors x float32 sqrt(s)) - the device does the same
            # product when the vectors are resident in float32 (one real field, dual side); any other float32 model
            # takes the host path below
            out = dev.rotate_solved(n_rot, power=power, tol=tol, max_iter=1000)
        else:
            sqrt_svals = np.sqrt(self._get_svals(n_rot))
            V = self._get_V(n_rot, rotated=False)
            n_vars_left = V['left'].shape[0]
            # loadings of both fields stacked (Cheng and Dunkerton 1995)
            L = np.concatenate(list(V.values())) * sqrt_svals
            out = dev.rotate_loadings(L, n_left=n_vars_left, power=power, tol=tol, max_iter=1000)
        self._varimax_iterations = out['n_iter']

        norm = {'left': out['norm_left'], 'right': out['norm_right']}
        if not self._analysis['is_bivariate']:
            norm['right'] = norm['left']
        variance = norm['left'] * norm['right']
        self._norm = norm
        self._variance = variance
        self._var_idx = np.argsort(variance)[::-1]
        self._rotation_matrix = out['R']
        self._correlation_matrix = out['Phi']
        self._analysis['is_rotated'] = True
        self._analysis['n_rot'] = n_rot
        self._analysis['power'] = power

    def rotation_matrix(self, inverse_transpose=False):
        """Rotation matrix (unit matrix when not rotated); `inverse_transpose` matters for Promax only."""
        try:
            R = self._rotation_matrix
        except AttributeError:
            R = np.eye(len(self._get_svals()))         # (not the public getter: the facade's returns a DataArray)
        if inverse_transpose and self._analysis['power'] > 1:
            R = np.linalg.pinv(R).conjugate().T
        return R

    def correlation_matrix(self):
        """Correlation matrix of the (rotated) PCs, ordered by variance."""
        try:
            idx = self._var_idx
            return self._correlation_matrix[idx, :][:, idx]
        except AttributeError:
            return np.eye(len(self._get_svals()))

    # ------------------------------------------------------------------------------------------
    # public getters (array.py:898-1297)
    # ------------------------------------------------------------------------------------------
    def fields(self, original_scale=False):
        """The (centered / normalised / complexified) input fields, optionally back in original units."""
        return self._deliver(self._get_fields(original_scale))

    def singular_values(self, n=None):
        return self._get_svals(n)

    def norm(self, n=None, sorted=True):
        return self._get_norm(n=n, sorted=sorted)

    def variance(self, n=None, sorted=True):
        return self._get_variance(n=n, sorted=sorted)

    def scf(self, n=None):
        """Squared covariance fraction in percent."""
        variance = self._variance[self._var_idx][:n]
        return variance ** 2 / self._analysis['total_squared_covariance'] * 100

    def explained_variance(self, n=None):
        """Covariance fraction in percent."""
        return self._get_variance(n=n, sorted=True) / self._analysis['total_covariance'] * 100

    def pcs(self, n=None, scaling='None', phase_shift=0, rotated=True):
        return self._deliver(self._get_pcs(n, scaling, phase_shift, rotated))

    def eofs(self, n=None, scaling='None', phase_shift=0, rotated=True):
        return self._deliver(self._get_eofs(n, scaling, phase_shift, rotated, alloc=self._alloc()))

    def spatial_amplitude(self, n=None, scaling='None', rotated=True):
        out = self._maps_from_device(n, rotated, _hip.MAP_AMPLITUDE, 'max' if scaling == 'max' else 'None', alloc=self._alloc())
        if out is not None:
            return out
        out = {}
        for k, eof in _numpy_result(self, 'eofs', n, scaling='None', rotated=rotated).items():
            out[k] = np.sqrt(eof * eof.conjugate()).real
            if scaling == 'max':
                out[k] /= np.nanmax(out[k], axis=tuple(range(out[k].ndim - 1)))
        return self._deliver(out)

    def spatial_phase(self, n=None, phase_shift=0, rotated=True):
        out = self._maps_from_device(n, rotated, _hip.MAP_PHASE, 'None', phase_shift, alloc=self._alloc())
        if out is not None:
            return out
        return self._deliver({k: np.arctan2(e.imag, e.real).real
                              for k, e in _numpy_result(self, 'eofs', n, phase_shift=phase_shift, rotated=rotated).items()})

    def temporal_amplitude(self, n=None, scaling='None', rotated=True):
        out = {}
        for k, pc in _numpy_result(self, 'pcs', n, scaling='None', rotated=rotated).items():
            out[k] = np.sqrt(pc * pc.conjugate()).real
            if scaling == 'max':
                out[k] /= np.nanmax(out[k], axis=0)
        return self._deliver(out)

    def temporal_phase(self, n=None, phase_shift=0, rotated=True):
        return self._deliver({k: np.arctan2(p.imag, p.real).real
                              for k, p in _numpy_result(self, 'pcs', n, phase_shift=phase_shift, rotated=rotated).items()})

    def _correlation_maps(self, n, phase_shift, pair):
        """Pearson correlation of every grid point (real part of the field) with the PCs and its p-value
        (array.py:1188-1261, tools/array.py:76-88).  The correlations are one tall GEMM over the field resident on the
        device instead of the reference's (N + m)^2 `np.corrcoef` matrix; the p-values and the final layout (masked grid
        points as NaN, modes last) come from the device as well (`xmca_correlation_maps`).  Fewer than 3 observations (the null
        distribution does not exist: every p is NaN) and `_patterns_on_host` take the host route: `xmca_correlate`, then
        `_two_sided_p` and the re-layout in numpy."""
        pcs = self._get_pcs(n=n, phase_shift=phase_shift)
        dev = self._resident_device()
        n_obs = self._n_observations['left']
        on_host = n_obs < 3 or n_obs > _hip.PVALUE_MAX_OBS or getattr(self, '_patterns_on_host', False)
        alloc = None if on_host else self._alloc()
        rvals, pvals = {}, {}
        for side, k in enumerate(self._keys):
            try:
                y = pcs[pair[k]].real
            except KeyError:
                raise KeyError('Key not found. Two fields needed for heterogenous maps.')
            r_dtype = np.result_type(self._fields_store[k].real.dtype, y.dtype)
            if on_host:
                r = dev.correlate(side, y, self._fields_store[k].shape[1]).astype(r_dtype, copy=False)
                p = _two_sided_p(r, n_obs)
                r, p = (self._with_nan_columns(k, src.T, (src.shape[1],)).T for src in (r, p))
            else:
                r, p = dev.correlation_maps(side, y, *self._kept_columns(k), r_dtype, alloc=alloc)
            rvals[k] = r.reshape(self._fields_spatial_shape[k] + (r.shape[1],))
            pvals[k] = p.reshape(self._fields_spatial_shape[k] + (p.shape[1],))
        return self._deliver((rvals, pvals))

    def homogeneous_patterns(self, n=None, phase_shift=0):
        return self._correlation_maps(n, phase_shift, {k: k for k in self._keys})

    def heterogeneous_patterns(self, n=None, phase_shift=0):
        other = dict(zip(['left', 'right'], ['right', 'left']))
        return self._correlation_maps(n, phase_shift, other)

    def _transform_vectors(self, k):
        """(handle, vectors) for the device transforms of field k (xmca_predict / xmca_reconstruct): vectors None while they are
        still resident from this model's solve, the host array once they were fetched (or truncated).  None - the host path - for
        a model that was not solved by this package (`load_analysis`, injected vectors), a subclass with its own scaling that does
        not state it through `_device_column_weights`, and under `_transform_on_host`."""
        V = getattr(self, '_V', None)
        if getattr(self, '_transform_on_host', False) or not isinstance(V, _LazyVectors):
            return None
        if not self._scaling_known_to_device():
            return None                   # a subclass scales differently and does not say how: its own host path
        dev = self._device()
        if k in V._pending:
            return (dev, None) if dev.holds_result_of(self) else None
        return dev, V[k]

    def _device_column_weights(self, k):
        """What a subclass's `_scale_X` / `_scale_X_inverse` do beyond `- mean`, `/ std` to field k, for the device transforms:
        `(forward, inverse)`, two (N',) float64 arrays - `_scale_X` multiplies by `forward` last, `_scale_X_inverse` divides by
        `inverse` first - or None (nothing, the array class).  A subclass that overrides the scaling methods without overriding
        this hook keeps the host route (`_transform_vectors`)."""
        return None

    def _scaling_known_to_device(self):
        """False for a subclass that overrides `_scale_X` / `_scale_X_inverse` without stating it through `_device_column_weights`."""
        cls = type(self)
        return ((cls._scale_X is MCA._scale_X and cls._scale_X_inverse is MCA._scale_X_inverse)
                or cls._device_column_weights is not MCA._device_column_weights)

    def _inverse_scaling(self, k, original_scale):
        """(mean, std, inv_weight) of field k that the device's reconstructions undo for `original_scale`, else three None."""
        if not original_scale:
            return None, None, None
        weights = self._device_column_weights(k)
        return (self._field_means[k], self._field_stds[k] if self._analysis['is_normalized'] else None,
                None if weights is None else weights[1])

    def _reconstruct_on_device(self, mode, original_scale, full, alloc=None):
        """`(pcs(mode, 'eigen') @ V_rot^H).real`, scaled back and (full) with the masked points re-inserted as NaN, as one product
        over the vectors on the device per field (xmca_reconstruct): B = P A^H (T x m, `_reconstruct_coefficients`) is the only
        host work.  Returns {k: T x N (full) or T x N'} or None when the host path has to run."""
        route = {k: self._transform_vectors(k) for k in self._keys}
        if any(r is None for r in route.values()):
            return None
        rotated = self._analysis['is_rotated']
        keep = self._get_slice(mode)
        max_mode = self._max_mode(mode, rotated)
        max_mode = self._analysis['rank'] if max_mode is None else min(int(max_mode), self._analysis['rank'])
        for dev, Vh in route.values():
            max_mode = min(max_mode, self._V._rank if Vh is None else Vh.shape[1])
        P = self._get_pcs(n=mode, scaling='eigen', rotated=True)
        T = self._n_observations['left']
        out = {}
        for side, k in enumerate(self._keys):
            dev, Vh = self._transform_vectors(k)          # (again: the projection above may have fetched the vectors)
            vdt = self._resident_dtype() if Vh is None else Vh.dtype
            if rotated:
                A = _rotated_mix(self._get_svals(max_mode), self.rotation_matrix(), self._get_norm(max_mode, sorted=False)[k],
                                 self._var_idx, keep)
                vdt = np.result_type(vdt, np.float64)
            else:
                A = np.eye(max_mode)[:, keep]
            B = _reconstruct_coefficients(P[k], A) if A.shape[1] else np.zeros((T, 0))
            dtype = _real_dtype(np.result_type(P[k].dtype, vdt))            # the reference's (U @ V^H).real
            n_keep = self._fields_store[k].shape[1]
            mean, std, inv_weight = self._inverse_scaling(k, original_scale)
            keep_idx, n_full = self._kept_columns(k) if full else (None, n_keep)      # (not full: the compact columns, no scatter)
            X = dev.reconstruct(side, B, None if Vh is None else Vh[:, :B.shape[1]], n_keep, keep_idx=keep_idx,
                                N_full=n_full, mean=mean, std=std, inv_weight=inv_weight, alloc=alloc)
            out[k] = X if full else X.astype(dtype, copy=False)
        return out

    def _reconstructed_X(self, mode=None, original_scale=True):
        rec = self._reconstruct_on_device(mode, original_scale, full=False)
        if rec is not None:
            return rec
        V = self._get_V(n=mode, rotated=True)
        U = self._get_pcs(n=mode, scaling='eigen', rotated=True)
        Xrec = {k: (U[k] @ V[k].conj().T).real for k in self._keys}
        if original_scale:
            Xrec = self._scale_X_inverse(Xrec)
        return Xrec

    def reconstructed_fields(self, mode=None, original_scale=True):
        n_obs = self._n_observations['left']
        rec = self._reconstruct_on_device(mode, original_scale, full=True, alloc=self._alloc())
        if rec is not None:                  # final layout from the device: NaN at the masked points, float64
            return {k: X.reshape((-1,) + self._fields_spatial_shape[k]) for k, X in rec.items()}
        out = {}
        for k, X in self._reconstructed_X(mode=mode, original_scale=original_scale).items():
            full = self._with_nan_columns(k, np.asarray(X, dtype=float), (n_obs,))
            out[k] = full.reshape((-1,) + self._fields_spatial_shape[k])
        return self._deliver(out)

    _reconstructed_fields = reconstructed_fields

    # ------------------------------------------------------------------------------------------
    # predict (array.py:1299-1428)
    # ------------------------------------------------------------------------------------------
    def predict(self, left=None, right=None, n=None, scaling='None', phase_shift=0):
        """Project new data on the singular vectors (rotated if the model is).  Real new data of the model's field dtype is
        projected on the device (xmca_predict: the vectors stay there), anything else on the host as the reference does."""
        given = {k: d for k, d in zip(self._keys, [left, right]) if d is not None}
        given = {k: d.detach() if _is_tensor(d) else d for k, d in given.items()}
        given = {k: d.numpy() if _is_tensor(d) and d.device.type == 'cpu' else d for k, d in given.items()}

        def device_ready(k, d):   # real new data of the field's dtype: a numpy array, or a tensor the handle's GPU can read in place
            if _is_tensor(d):
                dtype = _tensor_np_dtype(d) if d.device.type == 'cuda' and d.device.index == self._device().device else None
            else:
                dtype = d.dtype if isinstance(d, np.ndarray) else None
            return dtype == _real_dtype(self._fields_store[k].dtype) and self._transform_vectors(k) is not None
        on_device = all(device_ready(k, d) for k, d in given.items())
        if not on_device:         # the host route, as the reference: tensors come down first
            given = {k: d.cpu().numpy() if _is_tensor(d) else d for k, d in given.items()}
        if on_device:
            V = None
            svals = self._get_svals()
        else:
            given = {k: d.copy() for k, d in given.items()}
            V = self._get_V(rotated=False)
            sqrt_svals = np.sqrt(self._get_svals())
        R = self.rotation_matrix(inverse_transpose=True)
        n_rot = R.shape[0]
        if n is None:
            n = n_rot
        out = {}
        for k, x in given.items():
            try:
                if _is_tensor(x):     # (stays as it lies in memory: `_device_view` flattens it)
                    if x.dim() < 1 or x.shape[0] * self._n_variables[k] != x.numel():
                        raise ValueError('cannot flatten the tensor to (time, {:})'.format(self._n_variables[k]))
                else:
                    x = x.reshape(x.shape[0], self._n_variables[k])
                if not on_device:
                    x = x[:, self._no_nan_index[k]]
            except ValueError as err:
                if len(x.shape) != len(self._shape[k]):
                    msg = ('Error in {:} field. Dimension of new data ({:}) and the original field ({:}) do not match. '
                           'Did you forget the time dimension?').format(k, len(x.shape), len(self._shape[k]))
                elif x.shape[1:] != self._field_means[k].shape:
                    msg = ('Error in {:} field. Spatial dimensions of new data {:} and the original field {:} '
                           'do not match.').format(k, x.shape[1:], self._shape[k][1:])
                else:
                    msg = 'Dimension mismatch in {:} field.'.format(k)
                raise ValueError(msg) from err
            if on_device:
                pcs = self._predict_on_device(k, x, svals, R, n_rot, n)
            else:
                try:
                    x = self._scale_X({k: x})[k]
                except ValueError as err:
                    msg = ('Error in {:} field. Spatial dimensions of new data {:} and the original field {:} '
                           'do not match.').format(k, x.shape[1:], self._field_means[k].shape)
                    raise ValueError(msg) from err
                pcs = (x @ V[k][:, :n_rot] / sqrt_svals[:n_rot]) @ R
                pcs = pcs[:, self._var_idx][:, :n]
            if self._analysis['is_complex']:
                pcs = pcs * cmath.rect(1, phase_shift)
            if scaling == 'None':
                pass
            elif scaling == 'eigen':
                pcs = pcs * self._get_norm(n, sorted=True)[k]
            elif scaling == 'max':
                pcs = pcs / np.nanmax(abs(self._get_pcs(n, 'None', phase_shift)[k].real), axis=0)
            elif scaling == 'std':
                pcs = pcs / np.nanstd(self._get_pcs(n, 'None', phase_shift)[k].real, axis=0)
            else:
                raise ValueError(_SCALINGS_MSG.format(scaling))
            out[k] = pcs
        return self._deliver(out)

    def _predict_on_device(self, k, x, svals, R_inv_t, n_rot, n):
        """`(x[:, kept] - mean) / std @ V[:, :n_rot] / sqrt(s) @ R^-H`, columns ordered and selected, for the raw T' x N new data x
        of field k: one ingest + product on the device (xmca_predict) with the m x q mix of `_predict_mix`.  As `_scale_X` is called
        with this field alone, it is divided by std whenever the model is normalized; a subclass's column weights
        (`_device_column_weights`) come last."""
        W = _predict_mix(svals, R_inv_t, self._var_idx, n_rot, n)
        if W.shape[1] == 0:
            return np.zeros((x.shape[0], 0), dtype=np.result_type(W.dtype, self._resident_dtype()))
        dev, Vh = self._transform_vectors(k)
        keep_idx = self._kept_columns(k)[0]
        std = self._field_stds[k] if self._analysis['is_normalized'] else None
        side = self._keys.index(k)
        weights = self._device_column_weights(k)
        if _is_tensor(x):         # (T', N) as it lies on the GPU; its producer on the caller's stream has finished first
            x = _device_view(x)
            _torch().cuda.current_stream(dev.device).synchronize()
        return dev.predict(side, x, keep_idx, self._field_means[k], std, None if Vh is None else Vh[:, :W.shape[0]], W,
                           weight=None if weights is None else weights[0])

    # ------------------------------------------------------------------------------------------
    # significance (array.py:1716-1952)
    # ------------------------------------------------------------------------------------------
    def lag1_autocorrelation(self):
        """Lag-1 autocorrelation of every grid point's series, estimated on the device from the centred real fields (a complex
        model: their real parts): {field name: float64 array in the field's spatial shape, NaN at masked points}.

        phi_c = sum_t (x[t] - m)(x[t+1] - m) / sum_t (x[t] - m)^2, in float64 for either field dtype, 0 for a constant series.  It
        does not change when a column is rescaled (`normalize`, `apply_weights`).  The fields are made resident as for the
        projections; only the values themselves come back.  This is the phi of `rule_n(noise='ar1')`."""
        self._get_svals(1)                    # (before `solve`: the getters' RuntimeError)
        dev = self._resident_device()
        out = {}
        for side, k in enumerate(self._keys):
            phi = dev.lag1_autocorrelation(side, int(np.count_nonzero(self._no_nan_index[k])))
            out[k] = self._with_nan_columns(k, phi, ()).reshape(self._fields_spatial_shape[k])
        return out

    def _phi_columns(self, phi):
        """`phi` of `rule_n(noise='ar1')` as one float64 array per field, a value for every column of the surrogates: the kept
        points take the given values, the masked ones 0 (their columns stay white, as in the white test).  ValueError for anything
        else than the documented forms, and for a value at a kept point that is not finite or has |phi| >= 1."""
        keys = self._keys
        if isinstance(phi, dict):
            extra = [k for k in phi if k not in keys]
            if extra or any(k not in phi for k in keys):
                raise ValueError('`phi` must hold one entry for each field {:}; got {:}'.format(list(keys), list(phi)))
            per_field = [phi[k] for k in keys]
        elif isinstance(phi, tuple):
            if len(phi) != 2:
                raise ValueError('`phi` as a tuple is the pair (left, right or None)')
            if (phi[1] is not None) != (len(keys) == 2):
                raise ValueError('`phi` must hold one entry for each field {:}, and none for a field the model lacks'.format(list(keys)))
            per_field = list(phi[:len(keys)])
        elif np.ndim(phi) == 0:
            per_field = [phi] * len(keys)
        elif len(keys) == 1:
            per_field = [phi]
        else:
            raise ValueError('`phi` of a model of two fields is a scalar, a dict or the pair (left, right)')
        out = []
        for k, value in zip(keys, per_field):
            keep = np.asarray(self._no_nan_index[k], dtype=bool)
            n_all, n_keep = keep.size, int(np.count_nonzero(keep))
            try:
                value = np.asarray(value, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError('`phi` of field {:} is not numeric'.format(k))
            if value.ndim == 0:
                kept = np.full(n_keep, float(value))
            elif value.shape == tuple(self._fields_spatial_shape[k]) or value.shape == (n_all,):
                kept = value.reshape(-1)[keep]              # (NaN at masked points, as `lag1_autocorrelation` returns them, is dropped here)
            elif value.shape == (n_keep,):
                kept = value
            else:
                raise ValueError('`phi` of field {:} has shape {:}; expected a scalar, {:}, ({:},) or ({:},)'.format(
                    k, value.shape, tuple(self._fields_spatial_shape[k]), n_all, n_keep))
            if not np.all(np.abs(kept) < 1.0):              # (False for NaN)
                raise ValueError('`phi` of field {:} must be finite with |phi| < 1 at every kept point'.format(k))
            full = np.zeros(n_all, dtype=np.float64)
            full[keep] = kept
            out.append(full)
        return out[0], (out[1] if len(out) == 2 else None)

    def rule_n(self, n_runs, n_modes=None, seed=None, dtype=np.float64, noise='white', phi=None):
        """Rule N (Overland & Preisendorfer 1982): spectra of `n_runs` Gaussian surrogates, scaled to the model's sum.

        The surrogate loop (array.py:1753-1765) runs on the device; when `torch.distributed` is initialised the
        runs are sharded over the ranks (contiguous blocks) and gathered with one collective.
        `seed` (extension): key of the counter-based device generator; default: drawn from numpy's global RNG, so
        `np.random.seed(s)` makes the result reproducible like the reference's use of the global stream.
        `noise` (extension): 'white' - uncorrelated surrogates, the reference's test; 'ar1' - red noise: every column of a surrogate
        is an AR(1) series of unit variance with the lag-1 autocorrelation `phi` of its grid point, made on the device from the same
        normals (phi = 0 gives the white surrogates bit for bit).  `phi`: None - estimated from the model's fields
        (`lag1_autocorrelation`); a scalar; or per field (a dict by field name, or the pair (left, right)) a scalar or an array in
        the field's spatial shape, flat over all grid points, or flat over the kept ones.  Masked points take no phi (NaN is
        accepted there): their surrogate columns stay white.  With several ranks every rank must pass the same phi.
        Returns an array (modes x kept runs); runs whose rotation does not converge are dropped (array.py:1762-1763).
        """
        from . import dist
        if noise not in ('white', 'ar1'):
            raise ValueError("{:} is not a valid noise model. Either 'white' or 'ar1'.".format(noise))
        if noise == 'white' and phi is not None:
            raise ValueError("`phi` belongs to noise='ar1'; white surrogates have none.")
        red = {}
        if noise == 'ar1':
            # (estimated before the surrogates take over the handle)
            red['ar1'] = self._phi_columns(self.lag1_autocorrelation() if phi is None else phi)
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2 ** 31 + int(np.random.randint(0, 2 ** 31 - 1))
        m = self._n_observations
        n = self._n_variables
        rotated = self._analysis['is_rotated']
        n_rot = self._analysis['n_rot']
        rank = min([m['left']] + [n[k] for k in self._keys])
        n_out = n_rot if rotated else rank
        spectra, kept = dist.sharded_rule_n(
            self._device(), n_runs, T=m['left'], Nx=n['left'], Ny=n.get('right', 0), n_fields=len(self._keys),
            complexify=self._analysis['is_complex'], rotated=rotated, p=n_rot, power=self._analysis['power'],
            tol=1e-8, seed=seed, dtype=dtype, n_out=n_out, **red)
        svals = spectra[kept.astype(bool)].T          # modes x kept runs
        ref = self._get_variance()
        svals /= svals.sum(axis=0) / ref.sum()
        return svals[self._get_slice(n_modes)]

    def rule_north(self, n=None):
        """North's rule of thumb (x sqrt(2) for complex models, Horel 1984)."""
        err = self._get_svals(n) * np.sqrt(2. / self._n_observations['left'])
        if self._analysis['is_complex']:
            err *= np.sqrt(2)
        return err

    def bootstrapping(self, n_runs, n_modes=20, axis=0, on_left=True, on_right=False, block_size=1, replace=True,
                      strategy='standard', disable_progress=False):
        """Monte Carlo (moving-block) bootstrap / permutation of the model (array.py:1813-1952).

        The block indices are drawn on the host from numpy's global RNG exactly as the reference draws them
        (tools/array.py:91-138) and composed over the replicates (`compose_bootstrap_indices`); the replicates themselves -
        cumulative resampling of rows (`axis=0`) or of columns (`axis=1`; of the concatenation [left | right] when both sides are
        resampled), centering, solve, rotation, variance - run on the device (`xmca_bootstrap_runs`, `xmca_bootstrap_runs_columns`).
        A model solved with extend='exp' runs there too, every replicate complexified with the same extended operator in float64
        (`xmca_bootstrap_runs_extended`, `xmca_bootstrap_runs_columns_extended`).  So does a model solved with extend='theta':
        the Theta fit is not linear in a column, so every replicate is fitted again after it has been gathered and centered, by the
        kernels of the solve, and complexified as X_im = G0 X + B C (`xmca_bootstrap_runs_theta`,
        `xmca_bootstrap_runs_columns_theta`; statsmodels is not needed).  All of these keep several replicates in flight and are
        sharded over the ranks of a `torch.distributed` job.  The reference's host loop over the replicates - one model per
        replicate - remains only for a model whose extension was applied on the host (`_extend_on_host`, private) and behind
        `_bootstrap_on_host` (private), for comparison.
        """
        complexify = self._analysis['is_complex']
        extend = self._analysis['extend']
        period = self._analysis['theta_period']
        is_rotated = self._analysis['is_rotated']
        n_rot = self._analysis['n_rot']
        power = self._analysis['power']
        n_modes_max = self._get_min_mode(n_modes, rotated=True)
        var_surr = np.zeros([n_modes_max, n_runs])
        extend_exp = bool(complexify) and extend == 'exp' and getattr(self, '_device_extend', None) is not None
        extend_theta = bool(complexify) and extend == 'theta' and getattr(self, '_device_theta', None) is not None
        on_device = (not extend or extend_exp or extend_theta) and not getattr(self, '_bootstrap_on_host', False)
        extension = {}
        if extend_exp:
            extension['extend_period'] = period
        if extend_theta:
            extension['theta_period'] = period
        if axis == 1:
            extension['axis'] = 1
        dev = self._device()
        n_obs = self._n_observations['left']
        for mode in range(n_modes):
            X_surr = self._real_fields() if self._device_extension() else self._get_X(original_scale=False, real=True)
            if strategy == 'iterative':
                X_rec = self._reconstructed_X(mode=mode, original_scale=False)
                for k in X_surr:
                    X_surr[k] -= X_rec[k]
            if on_device:
                widths = [X_surr[k].shape[1] for k in self._keys]
                # (the reference's errors, before any device work)
                idx_left, idx_right = compose_bootstrap_indices(n_runs, axis, n_obs, widths, on_left, on_right, block_size, replace)
                for side, k in enumerate(self._keys):
                    dev.set_field(side, _device_ready(np.ascontiguousarray(X_surr[k])))
                dev.bootstrap_begin(len(self._keys))
                rank = min([n_obs] + widths)
                n_out = n_rot if is_rotated else rank
                # (replicates are independent once composed: sharded over the ranks of a torch.distributed job like the Rule-N runs)
                from . import dist
                spec, kept = dist.sharded_bootstrap(dev, n_runs, T=n_obs, complexify=complexify, idx_left=idx_left, idx_right=idx_right,
                                                    rotated=is_rotated, p=n_rot, power=max(power, 1), tol=1e-8, n_out=n_out, **extension)
                for run in range(n_runs):
                    if kept[run]:
                        var_surr[mode:, run] = spec[run, :n_modes_max - mode]
                if strategy == 'standard':
                    break
                continue
            for run in range(n_runs):
                if on_left and not on_right:
                    X_surr['left'] = block_bootstrap(X_surr['left'], axis=axis, block_size=block_size, replace=replace)
                elif on_right and not on_left:
                    try:
                        X_surr['right'] = block_bootstrap(X_surr['right'], axis=axis, block_size=block_size,
                                                          replace=replace)
                    except KeyError as err:
                        raise ValueError('No bootstrapping possible. There is no right field. '
                                         'Set `on_right=False`.') from err
                elif on_left and on_right:
                    n_left = X_surr['left'].shape[1]
                    both = block_bootstrap(np.concatenate(list(X_surr.values()), axis=1), axis=axis,
                                           block_size=block_size, replace=replace)
                    X_surr['left'], X_surr['right'] = both[:, :n_left], both[:, n_left:]
                model = MCA(*list(X_surr.values()), handle=self._handle_override)
                model._extend_on_host = getattr(self, '_extend_on_host', False)
                model.solve(complexify=complexify, extend=extend, period=period)
                if is_rotated:
                    try:
                        model.rotate(n_rot, power)
                    except RuntimeError:
                        continue
                var_surr[mode:, run] = model._get_variance(n_modes_max - mode)
            if strategy == 'standard':
                break
        return var_surr

    def bootstrap_eofs(self, n_runs, n_modes=10, block_size=1, seed=None, indices=None):
        """Bootstrap mean and standard error of the leading EOFs at every grid point (an extension).

        `n_runs` (>= 2) replicates resample the time steps of all fields with the same moving-block index (a pairs bootstrap;
        `bootstrap_row_indices(n_runs, T, block_size, seed)`, or `indices`, an (n_runs, T) integer array, instead of the draw).
        The replicates are independent draws from the model's fields as `solve` saw them - weights and standardisation are
        kept, not estimated again - and are centred, Hilbert-transformed if the model is complex, and solved on the device,
        several in flight.  The first `n_modes` singular vectors of a replicate are aligned with the model's - one sign (real) or
        phase (complex) per mode, shared by both fields - and their deviation from the model's is accumulated on the device in
        float64; only the statistics come back.

        Returns a dict: 'mean' and 'std' - per field an array in the layout of `eofs(n_modes)`, spatial shape + (n_modes,), NaN at
        masked points; the mean is complex for a complex model, the standard error (ddof = 1, both parts of a complex vector) is
        real; 'congruence' - n_modes x n_runs, |<v0, v_r>| / number of fields in [0, 1], small where a replicate's mode is not the
        model's (degenerate or swapped modes inflate 'std' there); 'singular_values' - n_modes x n_runs, the replicates'.

        The results are float64 / complex128 numpy arrays for every field dtype, also for a model made with output='torch'.
        Under an initialised `torch.distributed` group every rank computes all replicates: nothing is sharded and no collective
        is called.  Rotated models and models solved with `extend=` are not supported (ValueError)."""
        self._get_svals(1)                    # (before `solve`: the getters' RuntimeError)
        if not _is_int(n_runs) or n_runs < 2:
            raise ValueError('`n_runs` must be an integer >= 2 (a standard error needs two replicates), not {!r}'.format(n_runs))
        if self._analysis['is_rotated']:
            raise ValueError('bootstrap_eofs does not support rotated models (out of scope: the modes of a replicate would have '
                             'to be matched with the rotated ones)')
        if self._analysis['extend']:
            raise ValueError('bootstrap_eofs does not support models solved with `extend=` (out of scope)')
        resident = len(self._singular_values)
        if not _is_int(n_modes) or not 1 <= n_modes <= resident:
            raise ValueError('`n_modes` must be an integer between 1 and the {:} modes the model holds, not {!r}'.format(resident, n_modes))
        n_runs, k = int(n_runs), int(n_modes)
        n_obs = self._n_observations['left']
        if indices is None:
            indices = bootstrap_row_indices(n_runs, n_obs, block_size=block_size, seed=seed)
        else:
            indices = np.asarray(indices)
            if indices.shape != (n_runs, n_obs) or not np.issubdtype(indices.dtype, np.integer):
                raise ValueError('`indices` must be an integer array of shape (n_runs, n_obs) = ({:}, {:})'.format(n_runs, n_obs))
            if indices.min() < 0 or indices.max() >= n_obs:
                raise ValueError('`indices` must lie in [0, {:})'.format(n_obs))
        complexify = bool(self._analysis['is_complex'])
        V0 = self._get_V(k, rotated=False)              # (fetched before the replicates take over the handle)
        dev = self._device()
        if not self._owns_device_fields(dev):
            X = self._get_X(original_scale=False, real=True)
            for side, key in enumerate(self._keys):
                dev.set_field(side, _device_ready(np.ascontiguousarray(X[key])))
        # (else the fields solve() worked on are still resident: their real planes are what the replicates resample, and
        #  the replicates work on copies, so the model keeps owning them)
        dev.bootstrap_begin(len(self._keys))
        mean, std, congruence, sigma, _ = dev.bootstrap_patterns(
            n_obs, complexify, indices, n_runs, k, V0[self._keys[0]], V0[self._keys[1]] if len(self._keys) == 2 else None)
        out = {'mean': {}, 'std': {}, 'congruence': np.ascontiguousarray(congruence.T), 'singular_values': np.ascontiguousarray(sigma.T)}
        for side, key in enumerate(self._keys):
            shape = self._fields_spatial_shape[key] + (k,)
            for name, values in (('mean', mean[side]), ('std', std[side])):
                full = self._with_nan_columns(key, np.asarray(values).T, (k,)).T
                out[name][key] = np.ascontiguousarray(full).reshape(shape)
        return out

    def _lag_window(self, what, embedding, tau, arg_error):
        """The argument checks and window arithmetic shared by `extended_eofs` and `extended_reconstruct` (`what`): `embedding` and
        `tau` integers >= 1, the caller's own argument (`arg_error`: its message, or None), one real field, T' >= 2.  Returns
        (M, tau, key, T, n_kept, T', min(T' - 1, M * n_kept))."""
        for name, value in (('embedding', embedding), ('tau', tau)):
            if not _is_int(value) or value < 1:
                raise ValueError('`{:}` must be an integer >= 1, not {!r}'.format(name, value))
        if arg_error is not None:
            raise ValueError(arg_error)
        if len(self._keys) != 1:
            raise ValueError('{:} takes a model of one field (extended MCA of two fields is out of scope)'.format(what))
        if self._analysis['is_complex']:
            raise ValueError('{:} does not support complex models (out of scope)'.format(what))
        M, tau = int(embedding), int(tau)
        key = self._keys[0]
        T = self._n_observations[key]
        n_kept = int(np.count_nonzero(self._no_nan_index[key]))
        n_win = T - (M - 1) * tau
        if n_win < 2:
            raise ValueError('embedding = {:} with tau = {:} leaves T - (embedding - 1) * tau = {:} of {:} time steps; at least 2 '
                             'are needed'.format(M, tau, n_win, T))
        return M, tau, key, T, n_kept, n_win, min(n_win - 1, M * n_kept)

    def extended_eofs(self, embedding, tau=1, n_modes=10):
        """Extended EOF analysis (EEOF; Weare & Nasstrom 1982; with a long window, multichannel SSA) of one real field: the EOFs
        of the field embedded with its own time lags (an extension).

        With X the field exactly as `solve()` sees it (T x N: centred, normalised / weighted if asked, masked columns removed),
        M = `embedding` and T' = T - (M - 1) * `tau`, the embedded matrix is Y = [X_0 | X_1 | ... | X_{M-1}] with
        X_j = X[j tau : j tau + T', :].  Every column of Y is centred over its T' rows and Y_c = U S V^H decomposed, with the
        one-field conventions of `solve()`, so that `extended_eofs(1)` is `solve()`.  Y is never formed: the device sums M
        diagonal shifts of the field's Gram matrix, centres the sum from both sides, takes `n_modes` leading eigenvectors and
        back-projects them on row-offset views of the resident field.  A prior `solve()` is not needed; a solved (and rotated)
        model keeps its result.

        Returns a dict of float64 numpy arrays (for float32 fields and for models made with output='torch' too):
        'singular_values' (n_modes,): S^2 / (T' - 1);  'explained_variance' (n_modes,): percent of the sum of all T' eigenvalues;
        'pcs' (T', n_modes): U sqrt(T' - 1), row t the window that starts at time step t;  'eofs': {field name: array of shape
        (embedding,) + spatial shape + (n_modes,)}, slice [j] the pattern at lag j * tau, NaN at masked points; a mode's patterns
        have unit norm over all lags and grid points together.

        Sign: the entry of largest magnitude of a mode's lag-0 pattern is positive (the first such entry on a tie), so repeated
        calls return the same bits.  Under an initialised `torch.distributed` group every rank computes everything: nothing is
        sharded and no collective is called.  ValueError: `embedding` or `tau` not an integer >= 1, T' < 2, `n_modes` not an
        integer in [1, min(T' - 1, M * N)], a model of two fields, a complex model."""
        M, tau, key, T, n_kept, n_win, most = self._lag_window(
            'extended_eofs', embedding, tau,
            None if _is_int(n_modes) else '`n_modes` must be an integer >= 1, not {!r}'.format(n_modes))
        k = int(n_modes)
        if not 1 <= k <= most:
            raise ValueError('`n_modes` must be an integer between 1 and min(T\' - 1, embedding * N) = {:}, not {!r}'.format(most, n_modes))
        dev = self._resident_device()
        lam, pcs, eofs = dev.extended_eofs(T, n_kept, M, tau, k, *self._kept_columns(key))
        total = np.maximum(lam, 0.0).sum()
        return {'singular_values': lam[:k] / (n_win - 1),
                'explained_variance': lam[:k] / total * 100.0,
                'pcs': pcs,
                'eofs': {key: eofs.reshape((M,) + tuple(self._fields_spatial_shape[key]) + (k,))}}

    def extended_rule_n(self, embedding, tau=1, n_runs=100, n_modes=10, seed=None, phi=None):
        """Monte-Carlo SSA test (Allen & Smith 1996) of the modes of `extended_eofs(embedding, tau, n_modes)` against red noise: which
        modes, and above all which oscillatory pair, carry more variance than AR(1) noise would put there (an extension;
        DESIGN.md 2.17).

        With Y_c = U S V^H the centred embedded matrix of `extended_eofs` and lambda_k = s_k^2, every run draws a surrogate field R
        from the null, embeds it like the data (Y_R, every column centred over its T' rows) and projects it on the DATA's patterns:
        Lambda_k(R) = ||Y_R,c v_k||^2, to be compared with lambda_k = Lambda_k(X).  No surrogate is decomposed and Y_R is never
        formed: per run the device generates R, forms W = R [V_0 | ... | V_{M-1}] with one thin product and sums M row-shifted
        column blocks of W.

        The null: column c of R is an AR(1) series with the lag-1 autocorrelation phi_c and the sample standard deviation
        (ddof = 1) of column c of the field as `solve()` sees it - the generator, segments and key (seed, run) of
        `rule_n(noise='ar1')`.  Unlike `rule_n`, whose surrogates have a (white) column for every masked grid point too, these have
        the kept columns only: a masked point has no pattern and takes no part.  No bias correction is applied to phi or to the
        variance (both are biased low in short records); pass corrected values as `phi`.  `phi`: None - estimated from the field
        (the values of `lag1_autocorrelation()`); else as in `rule_n`: a scalar or an array in the field's spatial shape, flat over
        all grid points, or flat over the kept ones.  `seed` as in `rule_n`.

        Returns a dict of float64 numpy arrays: 'singular_values' (n_modes,): lambda / (T' - 1), those of `extended_eofs`;
        'surrogates' (n_modes, n_runs): Lambda / (T' - 1);  'exceedance' (n_modes,): the share of runs with Lambda_k(R) >= lambda_k;
        'phi' and 'scale': the null's parameters in the field's spatial shape, NaN at masked points.

        A prior `solve()` is not needed; a solved (and rotated) model keeps its result.  Repeated calls with one seed return the
        same bits.  Under an initialised `torch.distributed` group every rank computes everything: nothing is sharded and no
        collective is called.  ValueError: the argument rules of `extended_eofs`, `n_runs` not an integer >= 1, a `phi` that
        `rule_n` would refuse."""
        M, tau, key, T, n_kept, n_win, most = self._lag_window(
            'extended_rule_n', embedding, tau,
            None if _is_int(n_modes) else '`n_modes` must be an integer >= 1, not {!r}'.format(n_modes))
        k = int(n_modes)
        if not 1 <= k <= most:
            raise ValueError('`n_modes` must be an integer between 1 and min(T\' - 1, embedding * N) = {:}, not {!r}'.format(most, n_modes))
        if not _is_int(n_runs) or n_runs < 1:
            raise ValueError('`n_runs` must be an integer >= 1, not {!r}'.format(n_runs))
        keep = np.asarray(self._no_nan_index[key], dtype=bool)
        phi_kept = None if phi is None else self._phi_columns(phi)[0][keep]
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2 ** 31 + int(np.random.randint(0, 2 ** 31 - 1))
        dev = self._resident_device()
        if phi_kept is None:
            phi_kept = dev.lag1_autocorrelation(0, n_kept)
        lam, scale, runs = dev.extended_rule_n(T, n_kept, M, tau, k, phi_kept, 0, int(n_runs), seed)
        shape = tuple(self._fields_spatial_shape[key])
        svals, null = lam[:k] / (n_win - 1), np.ascontiguousarray(runs.T) / (n_win - 1)
        return {'singular_values': svals,
                'surrogates': null,
                'exceedance': np.mean(null >= svals[:, None], axis=1),
                'phi': self._with_nan_columns(key, np.asarray(phi_kept, dtype=np.float64), ()).reshape(shape),
                'scale': self._with_nan_columns(key, scale, ()).reshape(shape)}

    def extended_reconstruct(self, embedding, tau=1, mode=None, original_scale=True):
        """Reconstructed component (RC) of a group of extended EOF modes: the part of the field, on its own T time steps and its own
        grid, that the chosen modes of `extended_eofs(embedding, tau)` carry (an extension) - the M-SSA counterpart
        of `reconstructed_fields`.

        With Y_c = U S V^H the centred embedded matrix of `extended_eofs` and Y^ its truncation to the chosen modes, time step t of
        the RC is the average of Y^[t - j tau, lag j] over the c_t windows j that hold t (diagonal averaging).  The device forms it
        as one product diag(1 / c) A~ P of the lag-placed eigenvectors with their back-projections on row-offset views of the
        resident field; neither Y nor the patterns are formed, and nothing but the result leaves the device.

        `mode` as in `reconstructed_fields`: None - all min(T' - 1, M N) modes; an int n - modes 1..n; a slice - 1-based with an
        inclusive stop.  original_scale=False: the RC in the units `solve()` sees.  original_scale=True: the window means that the
        centring of the embedded columns took out are added back (averaged the same way), then weights, `normalize()` and the
        field's mean are undone as in `reconstructed_fields(original_scale=True)`; with all modes the result is the field.

        Returns {field name: float64 array (T,) + spatial shape}, NaN at masked points; for output='torch' models a tensor written
        on the GPU.  A prior `solve()` is not needed; a solved (and rotated) model keeps its result.  Each call is self-contained:
        nothing is kept from an earlier `extended_eofs`.  ValueError: the argument rules of `extended_eofs`, `tau` > T' with
        `embedding` > 1 (time steps that lie in no window), a `mode` that is neither None, int nor slice, a selection that is
        empty or reaches past min(T' - 1, M N), a model of two fields, a complex model, `original_scale` on a subclass that
        overrides the scaling methods without the `_device_column_weights` hook."""
        M, tau, key, T, n_kept, n_win, most = self._lag_window(
            'extended_reconstruct', embedding, tau,
            None if mode is None or isinstance(mode, slice) or _is_int(mode)
            else 'Invalid `mode` {!r}. Must be None, an int or a slice.'.format(mode))
        if M > 1 and tau > n_win:
            raise ValueError('tau = {:} is above the window count T\' = {:}: some time steps lie in no window and cannot be '
                             'reconstructed'.format(tau, n_win))
        if mode is None:
            first, stop, step = 0, most, 1
        elif isinstance(mode, slice):
            first = 0 if mode.start is None else int(mode.start) - 1
            stop = most if mode.stop is None else int(mode.stop)
            step = 1 if mode.step is None else int(mode.step)
        else:
            first, stop, step = 0, int(mode), 1
        modes = np.arange(first, stop, step) if step >= 1 else np.arange(0)
        if first < 0 or modes.size < 1 or modes[-1] >= most:
            raise ValueError('`mode` = {!r} must select at least one of the modes 1..min(T\' - 1, embedding * N) = {:}'.format(mode, most))
        if original_scale and not self._scaling_known_to_device():
            raise ValueError('this class scales its fields in its own `_scale_X_inverse` without a `_device_column_weights`: '
                             'only original_scale=False is available')
        dev = self._resident_device()
        mean, std, inv_weight = self._inverse_scaling(key, original_scale)
        keep_idx, n_full = self._kept_columns(key)
        X = dev.extended_reconstruct(T, n_kept, M, tau, modes, bool(original_scale), keep_idx=keep_idx, N_full=n_full, mean=mean, std=std,
                                     inv_weight=inv_weight, alloc=self._alloc())
        return {key: X.reshape((-1,) + tuple(self._fields_spatial_shape[key]))}

    # ------------------------------------------------------------------------------------------
    # truncation / persistence (array.py:1602-1714, :1954-2012)
    # ------------------------------------------------------------------------------------------
    def truncate(self, n):
        """Keep only the first `n` modes (must not cut into a rotated solution)."""
        if self._analysis['is_rotated'] and n < self._analysis['n_rot']:
            raise ValueError('Cannot truncte rotated solution. Please ensure `n` > `n_rot`')
        if n < self._singular_values.size:
            self._singular_values = self._singular_values[:n]
            for k in self._keys:
                self._V[k] = self._V[k][:, :n]
            self._analysis['is_truncated'] = True
            self._analysis['is_truncated_at'] = n

    def _get_analysis_path(self, path=None):
        if path is None:
            folder = secure_str('_'.join(self._field_names.values()))
            return os.path.join(os.getcwd(), 'xmca', folder)
        return path if os.path.isabs(path) else os.path.abspath(path)

    def _create_analysis_path(self, path):
        path = self._get_analysis_path(path)
        os.makedirs(path, exist_ok=True)

    def _create_info_file(self, path):
        """`info.xmca`: `key : value` lines in the reference's layout (array.py:1629-1659)."""
        sep = '\n#' + '-' * 79
        lines = [wrap_str('This file contains information neccessary to load stored analysis'
                          'data from xmca module.'),
                 '\n# To load this analysis use:', '\n# from xmca.xarray import xMCA', '\n# mca = xMCA()',
                 '\n# mca.load_analysis(PATH_TO_THIS_FILE)', '\n', sep, sep,
                 '\n{:<20} : {:<57}'.format('created', datetime.now().strftime("%Y-%m-%d %H:%M:%S")), sep]
        for key, name in self._field_names.items():
            lines.append('\n{:<20} : {:<57}'.format(key, str(name)))
        lines.append(sep)
        for key, info in self._analysis.items():
            if key in ['is_bivariate', 'is_complex', 'is_rotated', 'is_truncated']:
                lines.append(sep)
            lines.append('\n{:<20} : {:<57}'.format(key, str(info)))
        with open(os.path.join(path, 'info.xmca'), 'w+') as fh:
            fh.write(''.join(lines))

    def _get_file_names(self, format):
        fields, eofs = {}, {}
        for key, variable in self._field_names.items():
            variable = secure_str(variable)
            fields[key] = '.'.join([variable, format])
            eofs[key] = '.'.join(['_'.join([variable, 'eofs']), format])
        return {'fields': fields, 'eofs': eofs, 'pcs': {}, 'singular': '.'.join(['singular_values', format]), 'norm': {}}

    def _save_data(self, data_array, path, *args, **kwargs):
        raise NotImplementedError('only works for `xarray`')

    def _set_analysis(self, key, value):
        try:
            key_type = type(self._analysis[key])
        except KeyError:
            raise KeyError("Key `{}` not found in info file.".format(key))
        self._analysis[key] = (value == 'True') if key_type == bool else key_type(value)

    def _set_info_from_file(self, path):
        with open(path, 'r') as fh:
            for line in fh.readlines():
                if line[0] == '#':
                    continue
                key = line.split(':')[0].rstrip()
                if key in ['left', 'right']:
                    self._field_names[key] = line.split(':')[1].strip()
                if key in self._analysis.keys():
                    if key == 'version':
                        continue                      # the file's writer, not this package
                    self._set_analysis(key, line.split(':')[1].strip())

    def plot(self, *args, **kwargs):
        """Not part of the accelerated path (xmca/array.py:1430-1711 draws with matplotlib / cartopy): every number the
        reference's figure shows is available from `eofs()`, `pcs()`, `explained_variance()`."""
        raise NotImplementedError('xmca_amd does not draw: plot()/save_plot() of the reference need matplotlib and cartopy; '
                                  'use eofs(), pcs(), explained_variance() of this model with your own plotting code')

    def save_plot(self, *args, **kwargs):
        return self.plot(*args, **kwargs)

    def load_analysis(self, path, fields=None, eofs=None, singular_values=None):
        """Restore a model written by `save_analysis` (fields / eofs / singular values supplied by the caller)."""
        self._set_info_from_file(path)
        self._keys = ['left', 'right'] if self._analysis['is_bivariate'] else ['left']
        self._ingest(fields)
        if self._analysis['is_normalized']:
            self.normalize()
        if self._analysis['is_complex']:
            self._fields = self._complexify(self._fields)
        self._V = {}
        self._norm = {}
        self._singular_values = singular_values
        self._variance = singular_values
        self._var_idx = np.argsort(singular_values)[::-1]
        for key in self._keys:
            self._norm[key] = np.sqrt(singular_values)
            n_modes = eofs[key].shape[-1]
            flat = eofs[key].reshape(self._n_variables[key], n_modes)
            self._V[key] = remove_nan_cols(flat.T).T
        if self._analysis['is_rotated']:
            self.rotate(self._analysis['n_rot'], self._analysis['power'])

    def summary(self):
        """Print the analysis meta information."""
        import yaml
        print(yaml.dump({k: str(v) for k, v in self._analysis.items()}, sort_keys=False, default_flow_style=False))


def compose_bootstrap_indices(n_runs, axis, n_obs, widths, on_left, on_right, block_size=1, replace=True):
    """The resampling of `bootstrapping` as indices: (idx_left, idx_right), each (n_runs, length) int64 or None for a side that
    is not resampled, for fields of n_obs rows and widths = [Nl] or [Nl, Nr] columns.  No device is involved.

    Per replicate one `np.random.choice(n_blocks, size=n_blocks, replace=replace)` is drawn from numpy's global generator, exactly as
    tools/array.py:132 does, and expanded from blocks to rows / columns.  The reference resamples cumulatively (X_surr is
    overwritten, array.py:1902-1928), so replicate r sees c_r = c_{r-1}[idx_r] of the original fields: the composed c_r are
    returned.  axis=0: row indices < n_obs, the same for both sides when both are resampled.  axis=1: column indices into
    [left | right] - a left-only draw lives in [0, Nl), a right-only draw in Nl + [0, Nr), and with both sides the concatenation
    of Nl + Nr columns is resampled with one draw (blocks may straddle the seam) and split again at Nl, so either side may
    receive columns of the other.  Raises the reference's ValueErrors (no right field, length not a multiple of block_size,
    invalid axis)."""
    n_fields = len(widths)
    if axis == 0:
        if on_right and n_fields < 2:
            raise ValueError('No bootstrapping possible. There is no right field. Set `on_right=False`.')
        length, offset = n_obs, 0
    else:
        if not (on_left or on_right):
            return None, None
        if on_right and not on_left and n_fields < 2:
            raise ValueError('No bootstrapping possible. There is no right field. Set `on_right=False`.')
        if axis != 1:
            raise ValueError('{:} not a valid axis. either 0 or 1.'.format(axis))
        if on_left and on_right:
            length, offset = sum(widths), 0
        elif on_left:
            length, offset = widths[0], 0
        else:
            length, offset = widths[1], widths[0]
    if length % block_size:
        raise ValueError('Length of data array ({:}) must be a multiple of block size {:}'.format(length, block_size))
    n_blocks = length // block_size
    cum = np.arange(length)
    composed = np.empty((n_runs, length), dtype=np.int64)
    for run in range(n_runs):
        if on_left or on_right:
            # one draw per replicate, like tools/array.py:132 (both sides share it when both are resampled)
            pick = np.random.choice(n_blocks, size=n_blocks, replace=replace)
            cum = cum[(pick[:, None] * block_size + np.arange(block_size)[None, :]).reshape(-1)]
        composed[run] = cum
    if axis == 0:
        return (composed if on_left else None), (composed if on_right else None)
    composed += offset
    if on_left and on_right:
        n_left = widths[0]
        return np.ascontiguousarray(composed[:, :n_left]), (np.ascontiguousarray(composed[:, n_left:]) if n_fields == 2 else None)
    return (composed, None) if on_left else (None, composed)


def bootstrap_row_indices(n_runs, T, block_size=1, seed=None):
    """Row indices of a moving-block bootstrap, (n_runs, T) int64: every run is ceil(T / block_size) blocks of `block_size`
    consecutive time steps with independently drawn starts in [0, T - block_size], cut to T rows.  The runs are independent draws
    from the original series (not composed like `compose_bootstrap_indices`).  `seed` keys `np.random.default_rng`; None draws
    one from numpy's global RNG, so `np.random.seed(s)` makes the result reproducible.  No device is involved."""
    n_runs, T, b = int(n_runs), int(T), int(block_size)
    if T < 1 or n_runs < 0:
        raise ValueError('`n_runs` must be >= 0 and `T` >= 1')
    if not 1 <= b <= T:
        raise ValueError('`block_size` must be between 1 and the number of time steps ({:}), not {:}'.format(T, block_size))
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2 ** 31 + int(np.random.randint(0, 2 ** 31 - 1))
    rng = np.random.default_rng(seed)
    nb = -(-T // b)
    starts = rng.integers(0, T - b + 1, (n_runs, nb))
    rows = (starts[..., None] + np.arange(b)).reshape(n_runs, nb * b)[:, :T]
    return np.ascontiguousarray(rows, dtype=np.int64)


def _gpu_visible():
    try:
        return _hip.load_library().xmca_device_count() > 0
    except Exception:
        return False


def secure_str(string):
    """file name form of a field name (info.xmca / netCDF names of save_analysis, array.py:1602-1627)"""
    return string.lower().replace(' ', '_')


def wrap_str(string):
    """'# '-prefixed comment block (header of info.xmca, array.py:1629-1640)"""
    import textwrap
    return textwrap.indent(textwrap.fill(string, width=80), '# ')


def _real_dtype(dt):
    dt = np.dtype(dt)
    if dt in (np.float32, np.complex64):
        return np.float32
    return np.float64


def _device_ready(field):
    """float32/float64 (or their complex pairs) pass through; anything else is promoted to float64."""
    dt = np.dtype(field.dtype)
    if dt in (np.float32, np.float64, np.complex64, np.complex128):
        return field
    return field.astype(np.complex128 if np.iscomplexobj(field) else np.float64)
