"""`xmca_amd.prepare` - a field prepared on the device: seasonal cycle and trend removed (`anomalies`), then
band-limited along time (`time_filter`).  The workflow: anomalies -> time_filter -> fill_gaps -> MCA.

Every analysis of this package starts from anomalies: the field minus its seasonal cycle, and often minus a linear trend.  The model
classes remove one mean per grid point and nothing else; `anomalies` regresses every grid point on a small basis of time functions
- phase means or harmonics of a period, a trend, or a basis of the caller's - and returns the residual.  The fit is over the present
values of a grid point, so a record with gaps (NaN) can be prepared before `fill_gaps` completes it; the whole step runs on the
device (xmca_column_regress) and takes a GPU tensor where it lies.

    from xmca_amd.prepare import anomalies, lanczos_weights, remove, time_basis, time_filter
    from xmca_amd.gaps import fill_gaps
    prep = anomalies(sst, period=12, trend=True)              # monthly means and a trend, fitted over the present values
    low = time_filter(prep['field'], lanczos_weights(121, 1 / 60), missing='renormalise')     # gaps stay gaps
    full = fill_gaps(low, n_modes=6)
    model = MCA(full['field']); model.solve()
    later = remove(sst_new, time_basis(len(sst_new), period=12, trend=True, start=len(sst), span=len(sst)), prep['coefficients'])

The model that was removed is not remembered anywhere else: keep the dict and call `remove` on new time steps.
"""
import numpy as np

from . import _hip
from .gaps import _is_tensor

MAX_COLUMNS = 16          # most basis columns (csrc/regress.h REG_K)
PIVOT_MIN = 1e-8          # the definiteness criterion (csrc/regress.h REG_PIVOT_MIN)
MAX_WEIGHTS = 1025        # most weights of a time filter (csrc/time_filter.h TF_MAX_WEIGHTS)


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


def _lowpass(L, fc):
    h = (L - 1) // 2
    j = np.arange(-h, h + 1, dtype=np.float64)
    w = np.empty(L, dtype=np.float64)
    nz = j != 0.0
    a = np.pi * j[nz] / (h + 1)
    w[nz] = np.sin(2.0 * np.pi * fc * j[nz]) / (np.pi * j[nz]) * (np.sin(a) / a)
    w[h] = 2.0 * fc
    w = 0.5 * (w + w[::-1])          # (the formula is even in j: keep the array so to the bit)
    return w / w.sum()


def lanczos_weights(n_weights, cutoff):
    """The float64 (n_weights,) weights of a Lanczos filter (Duchon 1979) for `time_filter`.

    n_weights    odd, L = 2 h + 1, 1 <= L <= 1025
    cutoff       a scalar f_c in cycles per time step, 0 < f_c < 0.5: the low-pass weights - with j = k - h,
                 w_j ~ sin(2 pi f_c j) / (pi j) * sin(pi j / (h + 1)) / (pi j / (h + 1)), w_0 ~ 2 f_c - normalised to sum to 1
                 (L = 1: [1.0]);  a pair (f_lo, f_hi), 0 < f_lo < f_hi < 0.5: the band-pass weights low(f_hi) - low(f_lo), their
                 sum brought to 0 at rounding level

    `time_filter(X, w, complement=True)` is the high-pass of low-pass weights w.  Anything else is a ValueError."""
    what = "lanczos_weights"
    L = _int(what, "n_weights", n_weights, 1)
    if L % 2 != 1 or L > MAX_WEIGHTS:
        raise ValueError("%s: n_weights must be odd and at most %d, got %d" % (what, MAX_WEIGHTS, L))

    def freq(v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 < float(v) < 0.5:
            raise ValueError("%s: a cutoff must be a number in (0, 0.5) cycles per time step, got %r" % (what, v))
        return float(v)
    if isinstance(cutoff, (tuple, list, np.ndarray)):
        if len(np.shape(cutoff)) != 1 or len(cutoff) != 2:
            raise ValueError("%s: cutoff must be a frequency or a pair (f_lo, f_hi), got %r" % (what, cutoff))
        lo, hi = freq(cutoff[0]), freq(cutoff[1])
        if not lo < hi:
            raise ValueError("%s: a band needs f_lo < f_hi, got %r" % (what, cutoff))
        w = _lowpass(L, hi) - _lowpass(L, lo)
        return w - w.sum() / L if L > 1 else w          # (the difference of two unit sums, brought to zero at rounding level)
    return _lowpass(L, freq(cutoff))


def _weight_sum(w):
    """sum(w) in ascending order, in float64: the chain the device runs for the denominator of a full window"""
    s = np.float64(0.0)
    for v in w:
        s = s + v
    return float(s)


def _check_weights(what, weights):
    w = np.asarray(weights)
    if w.dtype.kind not in 'fiu' or w.ndim != 1:
        raise ValueError("%s: the weights must be a real vector, got %s of shape %s" % (what, w.dtype, w.shape))
    if w.size % 2 != 1 or w.size > MAX_WEIGHTS:
        raise ValueError("%s: the number of weights must be odd and at most %d, got %d" % (what, MAX_WEIGHTS, w.size))
    w = np.ascontiguousarray(w, dtype=np.float64)
    if not np.isfinite(w).all():
        raise ValueError("%s: the weights hold a NaN or an Inf" % what)
    return w


def time_filter(X, weights, complement=False, missing='nan', min_weight=0.5, edges='nan', handle=None):
    """`X` filtered along time by the FIR weights `weights`, grid point by grid point, on the device.

    X            as in `anomalies`: time first and any spatial shape, real float32 or float64, NaN marking a missing value (an Inf
                 is refused): a numpy array, or a `torch.Tensor` on the handle's GPU in any layout
    weights      a real finite vector of odd length L = 2 h + 1 <= 1025, symmetric or not, e.g. `lanczos_weights(121, 1 / 60)`
    complement   False: the smoother S;  True: X - S, the high-pass of low-pass weights
    missing      'nan' (strict): an output entry is NaN exactly when one of the L entries of its window is missing or lies outside
                 the record;  'renormalise': S = num / den, the sums of w_k x and of w_k over the present entries of the window
                 only (steps outside the record count as missing) - an output entry is NaN exactly when X[t, n] itself is missing
                 or den < min_weight * sum(w).  It needs sum(w) > 0 (so no band-pass weights), 0 < min_weight <= 1 and edges='nan'
    edges        'nan': the shape of X, the first and last h steps NaN under missing='nan';  'trim' (missing='nan' only, T >= L):
                 the T - 2 h steps h .. T - h - 1 whose window lies inside the record, with the bits they have under 'nan' - `MCA`
                 drops every grid point with a NaN
    handle       a `_hip.Handle` (default: the one of the device); its resident fields and results are left as they are

    The smoother is a correlation, S[t, n] = sum_k weights[k] X[t + k - h, n]: weights[0] multiplies the earliest step.  It is one
    float64 fma chain in ascending k that starts from +0.0, whatever the dtype of X, and the output is rounded once to that dtype.
    The threshold min_weight * sum(w) is formed once on the host in float64 (sum(w) in ascending order).

    Returns the field alone: dtype and kind of X (a GPU tensor, written there by the device, when X was one).  Every argument error
    is a ValueError raised before the library's device code is reached."""
    what = "time_filter"
    w = _check_weights(what, weights)
    if not isinstance(complement, (bool, np.bool_)):
        raise ValueError("%s: complement must be True or False, got %r" % (what, complement))
    if not isinstance(missing, str) or missing not in ('nan', 'renormalise'):
        raise ValueError("%s: missing must be 'nan' or 'renormalise', got %r" % (what, missing))
    if not isinstance(edges, str) or edges not in ('nan', 'trim'):
        raise ValueError("%s: edges must be 'nan' or 'trim', got %r" % (what, edges))
    renorm, trim = missing == 'renormalise', edges == 'trim'
    den_min = 0.0
    if renorm:
        if trim:
            raise ValueError("%s: missing='renormalise' keeps the edges; it needs edges='nan'" % what)
        if isinstance(min_weight, (bool, np.bool_)) or not isinstance(min_weight, (int, float, np.integer, np.floating)) \
                or not 0.0 < float(min_weight) <= 1.0:
            raise ValueError("%s: min_weight must lie in (0, 1], got %r" % (what, min_weight))
        total = _weight_sum(w)
        if not total > 0.0:
            raise ValueError("%s: missing='renormalise' divides by the sum of the present weights; it needs sum(weights) > 0, got %g "
                             "(band-pass weights sum to 0)" % (what, total))
        den_min = float(np.float64(min_weight) * np.float64(total))
        if not den_min > 0.0:
            raise ValueError("%s: min_weight * sum(weights) underflows to zero" % what)
    if _is_tensor(X):
        T = int(X.shape[0]) if X.dim() >= 1 else 0
    else:
        T = int(np.shape(X)[0]) if np.ndim(X) >= 1 else 0
    if T < 1:
        raise ValueError("%s: the field needs time first and at least one spatial dimension" % what)
    if trim and T < w.size:
        raise ValueError("%s: edges='trim' needs at least as many time steps as weights, got %d steps and %d weights" % (what, T, w.size))
    field, shape, tensor = _check_field(what, X, handle)
    h = handle if handle is not None else _hip.default_handle()
    res = h.time_filter(field, w, complement=bool(complement), renormalise=renorm, den_min=den_min, trim=trim,
                        alloc=_tensor_alloc(h.device) if tensor else None)
    return res.reshape((shape[0] - (w.size - 1) if trim else shape[0],) + tuple(shape[1:]))
