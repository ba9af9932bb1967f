"""`xmca_amd.spectral` - Welch spectra and coherence maps on the device: the power spectrum of every grid point of a field with gaps,
and its coherence, phase and gain against index series, frequency by frequency.

The frequency-domain ends of the pipeline: before `time_filter`, the spectrum that the cut-offs of `lanczos_weights` are read from;
after the decomposition, the frequency-resolved counterpart of `lead_lag_maps` - at which periods does the field follow PC 1, and by
how much does it lag there.  The field may have gaps (NaN) - a missing value drops the segments that hold it and nothing else - and
may be a GPU tensor, read where it lies.

    from xmca_amd.spectral import spectral_maps
    model = MCA(full['field']); model.solve()
    maps = spectral_maps(prep['field'], model.pcs(1)['left'], nperseg=256)
    follows = (maps['p'] < 0.05) & (maps['phase'] < 0)          # coherent, the index leading
"""
import numpy as np

from . import _hip
from .gaps import _is_tensor
from .lagged import _check_index, center_index
from .prepare import _check_field, _tensor_alloc

MAX_INDICES = 4           # most index series (csrc/spectral.h SP_MAX_Q)
MIN_NPERSEG, MAX_NPERSEG = 8, 4096          # csrc/spectral.h SP_MIN_L, SP_MAX_L

_PI = np.longdouble("3.14159265358979323846264338327950288")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def welch_window(name_or_array, nperseg):
    """The `nperseg` float64 weights the device gets: 'hann' - the periodic Hann window 0.5 - 0.5 cos(2 pi j / L), scipy's default,
    evaluated in extended precision and rounded once; 'boxcar' - all ones; or an array of L finite values with a positive sum of
    squares, converted to float64."""
    what = "spectral_maps"
    if not _is_int(nperseg) or not MIN_NPERSEG <= int(nperseg) <= MAX_NPERSEG:
        raise ValueError("%s: nperseg must be an integer in [%d, %d], got %r" % (what, MIN_NPERSEG, MAX_NPERSEG, nperseg))
    L = int(nperseg)
    if isinstance(name_or_array, str):
        if name_or_array == 'hann':
            c = np.cos(2 * _PI * np.arange(L, dtype=np.longdouble) / L)
            return (np.longdouble(0.5) - np.longdouble(0.5) * c).astype(np.float64)
        if name_or_array == 'boxcar':
            return np.ones(L, dtype=np.float64)
        raise ValueError("%s: window must be 'hann', 'boxcar' or an array of nperseg weights, got %r" % (what, name_or_array))
    try:
        w = np.asarray(name_or_array)
    except Exception:
        raise ValueError("%s: window must be 'hann', 'boxcar' or an array of nperseg weights" % what) from None
    if w.dtype.kind not in 'fiu' or w.shape != (L,):
        raise ValueError("%s: a window array must hold nperseg = %d real weights, got dtype %s and shape %s" % (what, L, w.dtype, w.shape))
    w = np.ascontiguousarray(w, dtype=np.float64)
    if not np.isfinite(w).all():
        raise ValueError("%s: the window holds a NaN or an Inf" % what)
    w2 = float(np.sum(w.astype(np.longdouble) ** 2))
    if not (w2 > 0.0 and np.isfinite(w2)):
        raise ValueError("%s: the sum of the squared weights must be positive and finite" % what)
    return w


def _twiddle_extended(L):
    """(cos t, -sin t) at t = 2 pi i / L, i < L, in extended precision: the angle is folded into [0, pi / 4] by integer arithmetic, so
    the entries at the multiples of a quarter turn are exact."""
    a = 4 * np.arange(L, dtype=np.int64)
    ss = np.where(a > 2 * L, -1, 1)
    a = np.where(a > 2 * L, 4 * L - a, a)
    cs = np.where(a > L, -1, 1)
    a = np.where(a > L, 2 * L - a, a)
    swap = 2 * a > L
    a = np.where(swap, L - a, a)
    t = _PI * a.astype(np.longdouble) / np.longdouble(2 * L)
    c, s = np.cos(t), np.sin(t)
    c, s = np.where(swap, s, c), np.where(swap, c, s)
    return cs * c, -(ss * s)


def twiddle_table(nperseg):
    """(L, 2) float64: (cos t, -sin t) at t = 2 pi i / L - the table of the device (csrc/spectral.h sp_twiddle), evaluated in extended
    precision and rounded once."""
    c, ms = _twiddle_extended(int(nperseg))
    return np.stack([c.astype(np.float64), ms.astype(np.float64)], axis=1)


def effective_segments(K, weights, step):
    """The equivalent number of independent segments of K overlapping ones (Welch 1967), float64:
    Ke = K / (1 + 2 sum_{j >= 1, j step < L, j < K} (1 - j / K) rho_j^2) with rho_j = sum_i w_i w_{i + j step} / sum w^2; 0 at K = 0.
    K may be an array.  Segments that do not overlap (step = L) give Ke = K."""
    w = np.asarray(weights, dtype=np.float64).astype(np.longdouble)
    L, step = w.size, int(step)
    if step < 1:
        raise ValueError("effective_segments: step must be at least 1, got %r" % (step,))
    w2 = np.longdouble(0)
    for v in w:
        w2 = w2 + v * v
    rho2 = []
    j = 1
    while j * step < L:
        s = np.longdouble(0)
        for i in range(L - j * step):
            s = s + w[i] * w[i + j * step]
        rho2.append((s / w2) * (s / w2))
        j += 1
    Ks = np.atleast_1d(np.asarray(K))
    if Ks.dtype.kind not in 'iu' or (Ks < 0).any():
        raise ValueError("effective_segments: K must be a non-negative integer, got %r" % (K,))
    out = np.zeros(Ks.shape, dtype=np.float64)
    for at, k in np.ndenumerate(Ks):
        k = int(k)
        if k == 0:
            continue
        den = np.longdouble(1)
        for j in range(1, min(len(rho2), k - 1) + 1):
            den = den + np.longdouble(2) * (np.longdouble(1) - np.longdouble(j) / np.longdouble(k)) * rho2[j - 1]
        out[at] = np.float64(np.longdouble(k) / den)
    return out if np.ndim(K) else out[0]


def _check_bins(what, bins, L):
    if bins is None:
        return np.arange(L // 2 + 1, dtype=np.int64)
    try:
        seq = list(bins)
    except TypeError:
        raise ValueError("%s: bins must be None or a sequence of integers, got %r" % (what, bins)) from None
    if not seq:
        raise ValueError("%s: bins must not be empty" % what)
    for v in seq:
        if not _is_int(v):
            raise ValueError("%s: a bin must be an integer, got %r" % (what, v))
    out = np.array([int(v) for v in seq], dtype=np.int64)
    if len(set(out.tolist())) != out.size:
        raise ValueError("%s: the bins must be distinct, got %s" % (what, out.tolist()))
    if out.min() < 0 or out.max() > L // 2:
        raise ValueError("%s: a bin must lie in [0, nperseg // 2] = [0, %d], got %s" % (what, L // 2, out.tolist()))
    return out


def spectral_maps(X, index=None, nperseg=256, step=None, window='hann', detrend='mean', bins=None, fs=1.0, min_segments=2, handle=None):
    """Welch power spectra of the field `X`, grid point by grid point over the segments that are present, and - with `index` - its
    cross-spectrum, coherence, phase, gain and a p-value of the coherence against the index series, on the device.

    X            as in `lead_lag_maps`: time first and any spatial shape S, real float32 or float64, NaN marking a missing value (an
                 Inf is refused): a numpy array, or a `torch.Tensor` on the handle's GPU in any layout
    index        None, or shape (T,) or (T, q), 1 <= q <= 4: real and finite, no column constant.  It is converted to float64 and
                 its column means (ascending float64 sum / T) are subtracted on the host
    nperseg      L, an integer in [8, 4096], L <= T
    step         an integer in [ceil(L / 4), L]; default L // 2.  Segment m covers the rows m step .. m step + L - 1 for
                 m = 0 .. K - 1, K = (T - L) // step + 1: scipy's layout with noverlap = L - step
    window       'hann' (periodic, scipy's default), 'boxcar', or L finite weights with a positive sum of squares (`welch_window`)
    detrend      'mean': the mean of every segment is removed before the window is applied;  None: nothing is removed
    bins         None - all of 0 .. L // 2 - or a sequence of distinct integers in that range, in any order
    fs           the sampling frequency, positive; 'freqs' = bins fs / L
    min_segments an integer >= 1: a grid point with fewer present segments is NaN in every map
    handle       a `_hip.Handle` (default: the one of the device); its resident fields and results are left as they are

    Segment m is present for a grid point exactly when all of its L values are; K_n counts them ('segments').  A missing value drops
    the segments that hold it and nothing else; nothing is interpolated.  With c_n the mean of the present values of the grid
    point (one ascending float64 chain; it guards against cancellation and is 0 with detrend=None) and x' = x - c_n, the segment
    DFT A_k = sum_j (w_j x'_j) (cos t - i sin t), t = 2 pi ((k j) mod L) / L, is one float64 fma chain per part in ascending j from
    +0.0, whatever the dtype, with the cosines and sines from a table built on the host in extended precision.  Z_k = A_k - mu W_k
    with mu = sum_j x'_j / L and W the DFT of the weights: the DFT of the de-meaned, windowed segment (mu = 0 with detrend=None).
    The index goes through the same code and gives Y.  Over the present segments in ascending m: Sxx = sum |Z|^2,
    Syy = sum |Y|^2, C = sum conj(Y) Z.  With side = 1 at bin 0 and at bin L / 2 of an even L, else 2, and
    scale = side / (fs sum w^2 K_n), the result is a dict; with F = len(bins):
        'power'          (F,) + S, dtype of X: scale Sxx - what `scipy.signal.welch` returns
        'segments'       S, int32: K_n, for every grid point
        'freqs'          (F,) float64;  'bins' (F,) int64, a numpy copy of the argument in the caller's order
    and with an index
        'index_power'    (F,) + S + (q,), dtype of X: scale Syy - over the present segments of the grid point
        'cospectrum', 'quadrature'   scale Re C, scale Im C: `scipy.signal.csd(index, x)`
        'coherence'      |C|^2 / (Sxx Syy), clamped to [0, 1]
        'phase'          atan2(Im C, Re C): negative at frequency f where the index leads the field, by -phase / (2 pi f) steps
        'gain'           |C| / Syy, field units per index unit
        'p'              float64: (1 - coherence)^(Ke - 1) from the returned coherence, Ke = `effective_segments(K_n, w, step)`; the
                         present segments of a gappy grid point count as contiguous
    Coherence, phase, gain and p are NaN as well where K_n < 2 (one segment gives coherence 1 identically) and where the bin carries
    no power on either side - a definition: unless Sxx > 2^-40 R and Syy > 2^-40 Ry, R the summed energy
    sum_j (w_j (x'_j - mu))^2 of the present segments, which by Parseval is the mean of Sxx over all L bins.  That rejects an
    exactly constant grid point and bin 0 of segments de-meaned under the boxcar, whose value is rounding noise.  A 1-D index keeps the trailing axis of
    length 1.  For a tensor X every map is a GPU tensor that the device wrote; 'freqs' and 'bins' are numpy.  The maps of one bin
    depend neither on the other bins of the call nor on their order, and a call repeats its bits.  Every argument error is a
    ValueError raised before the library's device code is reached."""
    what = "spectral_maps"
    weights = welch_window(window, nperseg)
    L = int(nperseg)
    if step is None:
        step = L // 2
    if not _is_int(step) or not -(-L // 4) <= int(step) <= L:
        raise ValueError("%s: step must be an integer in [ceil(nperseg / 4), nperseg] = [%d, %d], got %r" % (what, -(-L // 4), L, step))
    if detrend is not None and not (isinstance(detrend, str) and detrend == 'mean'):
        raise ValueError("%s: detrend must be 'mean' or None, got %r" % (what, detrend))
    if not _is_int(min_segments) or int(min_segments) < 1:
        raise ValueError("%s: min_segments must be an integer of at least 1, got %r" % (what, min_segments))
    if isinstance(fs, (bool, np.bool_)) or not isinstance(fs, (int, float, np.integer, np.floating)) or not (np.isfinite(fs) and fs > 0):
        raise ValueError("%s: fs must be a positive finite number, got %r" % (what, fs))
    bin_list = _check_bins(what, bins, L)
    if _is_tensor(X):
        T = int(X.shape[0]) if X.dim() >= 1 else 0
    else:
        T = int(np.shape(X)[0]) if np.ndim(X) >= 1 else 0
    if T < 1:
        raise ValueError("%s: the field needs time first and at least one spatial dimension" % what)
    if L > T:
        raise ValueError("%s: nperseg = %d exceeds the T = %d time steps of the field" % (what, L, T))
    y = None if index is None else _check_index(what, index, T, MAX_INDICES)
    field, shape, tensor = _check_field(what, X, handle)
    yc = None if y is None else center_index(y)[0]
    h = handle if handle is not None else _hip.default_handle()
    res = h.spectral_maps(field, yc, L, int(step), weights, detrend == 'mean', bin_list, float(fs), int(min_segments),
                          alloc=_tensor_alloc(h.device) if tensor else None)
    S, F = tuple(shape[1:]), bin_list.size
    out = {'power': res['power'].reshape((F,) + S), 'segments': res['segments'].reshape(S),
           'freqs': bin_list.astype(np.float64) * float(fs) / np.float64(L), 'bins': bin_list.copy()}
    if y is not None:
        q = y.shape[1]
        for key in ('index_power', 'cospectrum', 'quadrature', 'coherence', 'phase', 'gain', 'p'):
            out[key] = res[key].reshape((F,) + S + (q,))
    return out
