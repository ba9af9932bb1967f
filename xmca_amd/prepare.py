"""`xmca_amd.prepare` - anomalies of a field on the device: seasonal cycle and trend removed.

Every analysis of this package starts from anomalies: the field minus its seasonal cycle, and often minus a linear trend.  The model
classes remove one mean per grid point and nothing else; `anomalies` regresses every grid point on a small basis of time functions
- phase means or harmonics of a period, a trend, or a basis of the caller's - and returns the residual.  The fit is over the present
values of a grid point, so a record with gaps (NaN) can be prepared before `fill_gaps` completes it; the whole step runs on the
device (xmca_column_regress) and takes a GPU tensor where it lies.

    from xmca_amd.prepare import anomalies, remove, time_basis
    from xmca_amd.gaps import fill_gaps
    prep = anomalies(sst, period=12, trend=True)              # monthly means and a trend, fitted over the present values
    full = fill_gaps(prep['field'], n_modes=6)
    model = MCA(full['field']); model.solve()
    later = remove(sst_new, time_basis(len(sst_new), period=12, trend=True, start=len(sst), span=len(sst)), prep['coefficients'])

The model that was removed is not remembered anywhere else: keep the dict and call `remove` on new time steps.
"""
import numpy as np

from . import _hip
from .gaps import _is_tensor

MAX_COLUMNS = 16          # most basis columns (csrc/regress.h REG_K)
PIVOT_MIN = 1e-8          # the definiteness criterion (csrc/regress.h REG_PIVOT_MIN)


def _int(what, name, v, least):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
        raise ValueError("%s: %s must be an int of at least %d, got %r" % (what, name, least, v))
    return int(v)


def time_basis(n_steps, period=None, harmonics=None, trend=False, start=0, span=None):
    """The float64 (n_steps, k) basis of `anomalies`; row i is for the time step t = start + i.

    period=None                one constant column
    period=m, harmonics=None   the m indicator columns of t mod m (phase means)
    period=m, harmonics=H      the constant, then cos(2 pi h t / m), sin(2 pi h t / m) for h = 1 .. H; needs 1 <= H <= (m - 1) // 2
    trend=True                 appends (t - (span - 1) / 2) / span, span defaulting to n_steps
    start, span                evaluate the model of a fitted record on later time steps: the basis of a record of 2 T steps is
                               time_basis(T, ..., span=2 T) over time_basis(T, ..., start=T, span=2 T)

    k is at most 16 (monthly means + trend: 13; seven harmonics + trend: 16); anything else is a ValueError."""
    what = "time_basis"
    T = _int(what, "n_steps", n_steps, 1)
    start = _int(what, "start", start, 0)
    if not isinstance(trend, (bool, np.bool_)):
        raise ValueError("%s: trend must be True or False, got %r" % (what, trend))
    if span is not None:
        span = _int(what, "span", span, 1)
        if not trend:
            raise ValueError("%s: span is the scale of the trend column; it needs trend=True" % what)
    if period is None:
        if harmonics is not None:
            raise ValueError("%s: harmonics need a period" % what)
        k = 1
    else:
        m = _int(what, "period", period, 1)
        if harmonics is None:
            k = m
        else:
            H = _int(what, "harmonics", harmonics, 1)
            if H > (m - 1) // 2:
                raise ValueError("%s: harmonics must lie in [1, (period - 1) // 2] = [1, %d], got %d" % (what, (m - 1) // 2, H))
            k = 1 + 2 * H
    k += int(bool(trend))
    if k > MAX_COLUMNS:
        raise ValueError("%s: %d basis columns, at most %d are supported" % (what, k, MAX_COLUMNS))
    t = np.arange(start, start + T, dtype=np.int64)
    B = np.zeros((T, k), dtype=np.float64)
    if period is None:
        B[:, 0] = 1.0
    elif harmonics is None:
        B[np.arange(T), t % m] = 1.0
    else:
        B[:, 0] = 1.0
        phase = (t % m).astype(np.float64)          # (the angle of t mod m: exact periodicity however large t is)
        for h in range(1, H + 1):
            B[:, 2 * h - 1] = np.cos(2.0 * np.pi * h * phase / m)
            B[:, 2 * h] = np.sin(2.0 * np.pi * h * phase / m)
    if trend:
        s = T if span is None else span
        B[:, -1] = (t.astype(np.float64) - (s - 1) / 2.0) / s
    return B


def _check_basis(what, basis, T):
    B = np.asarray(basis)
    if B.dtype.kind not in 'fiu' or B.ndim != 2:
        raise ValueError("%s: the basis must be a real (T, k) array, got %s of shape %s" % (what, B.dtype, B.shape))
    if B.shape[0] != T:
        raise ValueError("%s: the basis has %d rows, the field %d time steps" % (what, B.shape[0], T))
    if not 1 <= B.shape[1] <= MAX_COLUMNS:
        raise ValueError("%s: the basis has %d columns, between 1 and %d are supported" % (what, B.shape[1], MAX_COLUMNS))
    B = np.ascontiguousarray(B, dtype=np.float64)
    if not np.isfinite(B).all():
        raise ValueError("%s: the basis holds a NaN or an Inf" % what)
    return B


def _check_field(what, X, handle):
    """(flat field or DeviceView, shape, is a tensor): the field checked - without a device for a numpy array."""
    if _is_tensor(X):
        from .array import _device_view, _tensor_np_dtype
        if X.device.type == 'cpu':
            raise ValueError("%s: a tensor must lie on the handle's GPU (pass tensor.numpy() for a host field)" % what)
        if X.device.type != 'cuda':
            raise ValueError("%s: the field is on %s, the library works on a GPU" % (what, X.device))
        if _tensor_np_dtype(X) not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("%s: the field must be real float32 or float64, got %s" % (what, X.dtype))
        if X.dim() < 2:
            raise ValueError("%s: the field needs time first and at least one spatial dimension, got shape %s" % (what, tuple(X.shape)))
        shape = tuple(int(n) for n in X.shape)
        if min(shape) < 1:
            raise ValueError("%s: the field is empty, shape %s" % (what, shape))
        h = handle if handle is not None else _hip.default_handle()          # (every check that needs no device has passed)
        if X.device.index != h.device:
            raise ValueError("%s: the field is on %s, the handle works on GPU %d" % (what, X.device, h.device))
        import torch
        X = X.detach()
        if bool(torch.isinf(X).any()):
            raise ValueError("%s: the field holds an Inf (NaN marks a missing value)" % what)
        # The view first, the synchronisation after it: where no two strides express (T, N) - a spatial sub-box, permuted spatial
        # axes - `_device_view` lets torch make a contiguous copy, queued on the caller's stream.  The library reads on a stream
        # of its own, so the caller's stream is drained once the view, and any copy behind it, exists (as `MCA._ingest` does).
        view = _device_view(X)
        torch.cuda.current_stream(X.device).synchronize()
        return view, shape, True
    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        raise ValueError("%s: the field must be real float32 or float64, got %s" % (what, X.dtype))
    if X.ndim < 2:
        raise ValueError("%s: the field needs time first and at least one spatial dimension, got shape %s" % (what, X.shape))
    if X.size == 0:
        raise ValueError("%s: the field is empty, shape %s" % (what, X.shape))
    flat = np.ascontiguousarray(X.reshape(X.shape[0], -1))
    if np.isinf(flat).any():
        raise ValueError("%s: the field holds an Inf (NaN marks a missing value)" % what)
    return flat, X.shape, False


def _tensor_alloc(device_index):
    import torch
    device = torch.device('cuda', device_index)

    def alloc(shape, dtype):
        t = torch.empty(tuple(int(n) for n in shape), dtype=getattr(torch, np.dtype(dtype).name), device=device)
        return t, t.data_ptr()
    return alloc


def anomalies(X, period=None, harmonics=None, trend=False, basis=None, handle=None):
    """`X` minus its least-squares fit on a basis of time functions, grid point by grid point, on the device.

    X            time first and any spatial shape, real float32 or float64, NaN marking a missing value (an Inf is refused): a numpy
                 array, or a `torch.Tensor` on the handle's GPU in any layout (two strides are read where they lie, as `MCA(tensor)`)
    period, harmonics, trend   the basis `time_basis(T, period, harmonics, trend)`
    basis        instead of those three: the caller's own (T, k) basis, k <= 16, e.g. to regress out an index
    handle       a `_hip.Handle` (default: the one of the device); its resident fields and results are left as they are

    For every grid point the coefficients c are the least-squares fit of its PRESENT values on the basis rows of those time steps, in
    float64 whatever the dtype of X; the result is x - B c at the present entries, computed in float64 and rounded once to the dtype
    of X.  A missing entry stays NaN.  A grid point is fitted when it has at least k present values and its k x k normal matrix
    sum_present b b^T passes the definiteness criterion; a grid point that is not fitted comes back all NaN.

    The definiteness criterion (a definition): in the Cholesky factorisation of the normal matrix A, taken in the order of the basis
    columns, every pivot d_j = A[j][j] - sum_{i<j} L[j][i]^2 exceeds 1e-8 A[j][j].  d_j / A[j][j] is the share of basis column j -
    over the present time steps - that the columns before it do not explain: 0.5 and above for a well-posed column, exactly 0 for a
    phase without any value.

    Returns a dict: 'field' (shape and dtype of X; a tensor on the GPU, written there by the device, when X was one),
    'coefficients' ((k,) + spatial shape, float64, numpy, NaN where not fitted), 'fitted' (bool, spatial shape), 'basis' (the (T, k)
    array used).  Every argument error is a ValueError raised before the library's device code is reached."""
    what = "anomalies"
    if basis is not None and (period is not None or harmonics is not None or trend):
        raise ValueError("%s: give basis, or period / harmonics / trend, not both" % what)
    if _is_tensor(X):
        T = int(X.shape[0]) if X.dim() >= 1 else 0
    else:
        T = int(np.shape(X)[0]) if np.ndim(X) >= 1 else 0
    if T < 1:
        raise ValueError("%s: the field needs time first and at least one spatial dimension" % what)
    B = _check_basis(what, basis, T) if basis is not None else time_basis(T, period, harmonics, trend)
    field, shape, tensor = _check_field(what, X, handle)
    h = handle if handle is not None else _hip.default_handle()
    res, coef, fitted = h.column_regress(field, B, alloc=_tensor_alloc(h.device) if tensor else None)
    return {'field': res.reshape(shape), 'coefficients': coef.reshape((B.shape[1],) + shape[1:]), 'fitted': fitted.reshape(shape[1:]),
            'basis': B}


def remove(X, basis, coefficients, handle=None):
    """The residual step of `anomalies` alone: `X` minus basis @ coefficients at its present entries, no fit - a model fitted on one
    record subtracted from new time steps (what `MCA.predict(new data)` needs).  `basis`: (T, k) for the T time steps of X
    (`time_basis(T, ..., start=, span=)` continues the basis of the fitted record); `coefficients`: (k,) + spatial shape, as
    `anomalies` returned them - a grid point with a NaN among its coefficients comes back all NaN.  With the basis and coefficients
    that `anomalies(X)` returned, the bits of its 'field'.  Returns the field alone: shape, dtype and kind (numpy / GPU tensor) of X."""
    what = "remove"
    T = int(X.shape[0]) if hasattr(X, 'shape') and len(X.shape) >= 1 else (int(np.shape(X)[0]) if np.ndim(X) >= 1 else 0)
    if T < 1:
        raise ValueError("%s: the field needs time first and at least one spatial dimension" % what)
    B = _check_basis(what, basis, T)
    C = np.asarray(coefficients)
    if C.dtype.kind not in 'fiu':
        raise ValueError("%s: the coefficients must be real, got %s" % (what, C.dtype))
    spatial = tuple(int(n) for n in X.shape[1:]) if hasattr(X, 'shape') else np.shape(X)[1:]
    if C.shape != (B.shape[1],) + tuple(spatial):
        raise ValueError("%s: the coefficients must have shape (k,) + spatial shape = %s, got %s" % (what, (B.shape[1],) + tuple(spatial), C.shape))
    if np.isinf(C).any():
        raise ValueError("%s: the coefficients hold an Inf (NaN marks a grid point that is not fitted)" % what)
    field, shape, tensor = _check_field(what, X, handle)
    h = handle if handle is not None else _hip.default_handle()
    C = np.ascontiguousarray(C.reshape(B.shape[1], -1), dtype=np.float64)
    res = h.column_residual(field, B, C, alloc=_tensor_alloc(h.device) if tensor else None)
    return res.reshape(shape)
