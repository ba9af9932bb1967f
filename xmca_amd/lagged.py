"""`xmca_amd.lagged` - lead-lag maps on the device: a field regressed on and correlated with index series at a range of lags,
with p-values, grid point by grid point over the present values.

What users of an EOF / MCA package do next with a PC, a box average or a reconstructed component: regress the field on it at
leads and lags and mask what is not significant.  The field may have gaps (NaN) - every lag uses the pairs that exist - and may be a
GPU tensor, read where it lies.

    from xmca_amd.lagged import lead_lag_maps
    model = MCA(full['field']); model.solve()
    maps = lead_lag_maps(prep['field'], model.pcs(2)['left'], range(-12, 13), dof='bretherton')
    significant = maps['p'] < 0.05
"""
import numpy as np

from . import _hip
from .gaps import _is_tensor
from .prepare import _check_field, _tensor_alloc

MAX_INDICES = 8           # most index series (csrc/lead_lag.h LL_MAX_Q)
MAX_ENTRIES = 1024        # most lags x index series of a call (csrc/lead_lag.h LL_MAX_ENTRIES)


def _ascending_sum(v):
    """sum(v) over the first axis in ascending order, in float64, starting from +0.0"""
    s = np.zeros(v.shape[1:], dtype=np.float64)
    for row in v:
        s = s + row
    return s


def _check_index(what, index, T, most=MAX_INDICES):
    """The index as a (T, q) float64 plane with 1 <= q <= `most`, checked."""
    if _is_tensor(index):
        index = index.detach().cpu().numpy()
    y = np.asarray(index)
    if y.dtype.kind not in 'fiu':
        raise ValueError("%s: the index must be real, got %s" % (what, y.dtype))
    if y.ndim == 1:
        y = y[:, None]
    if y.ndim != 2 or y.shape[0] != T:
        raise ValueError("%s: the index must have shape (T,) or (T, q) with T = %d time steps, got %s" % (what, T, np.shape(index)))
    if not 1 <= y.shape[1] <= most:
        raise ValueError("%s: between 1 and %d index series are supported, got %d" % (what, most, y.shape[1]))
    y = np.ascontiguousarray(y, dtype=np.float64)
    if not np.isfinite(y).all():
        raise ValueError("%s: the index holds a NaN or an Inf (an index with gaps is not supported)" % what)
    if (y == y[0]).all(axis=0).any():
        raise ValueError("%s: an index series is constant" % what)
    return y


def _check_lags(what, lags, T, q):
    try:
        seq = list(lags)
    except TypeError:
        raise ValueError("%s: lags must be a sequence of integers, got %r" % (what, lags)) from None
    if not seq:
        raise ValueError("%s: lags must not be empty" % what)
    for v in seq:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s: a lag must be an integer, got %r" % (what, v))
    out = np.array([int(v) for v in seq], dtype=np.int64)
    if len(set(out.tolist())) != out.size:
        raise ValueError("%s: the lags must be distinct, got %s" % (what, out.tolist()))
    if np.abs(out).max() > T - 1:
        raise ValueError("%s: a lag must lie in [-(T - 1), T - 1] with T = %d, got %d" % (what, T, out[np.argmax(np.abs(out))]))
    if out.size * q > MAX_ENTRIES:
        raise ValueError("%s: at most %d lags x index series per call, got %d x %d" % (what, MAX_ENTRIES, out.size, q))
    return out


def center_index(y):
    """(y', means): the (T, q) float64 plane minus its column means, each mean the ascending float64 sum divided by T - what
    `lead_lag_maps` gives the device."""
    mean = _ascending_sum(y) / np.float64(y.shape[0])
    return y - mean, mean


def lag1_index(yc):
    """The lag-1 autocorrelation of every column of the centred gap-free plane `yc`, the expression the device evaluates for the
    columns of a field: [sum_t y'_t y'_{t+1} / (T - 1)] / [sum_t y'_t^2 / T] in ascending float64 sums, 0 where T = 1 or the
    denominator is not positive, clamped to [-1, 1]."""
    T = yc.shape[0]
    rho = np.zeros(yc.shape[1], dtype=np.float64)
    if T < 2:
        return rho
    den = _ascending_sum(yc * yc) / np.float64(T)
    num = _ascending_sum(yc[:-1] * yc[1:]) / np.float64(T - 1)
    ok = den > 0.0
    rho[ok] = num[ok] / den[ok]
    return np.clip(rho, -1.0, 1.0)


def lead_lag_maps(X, index, lags, min_pairs=8, dof='n', handle=None):
    """Regression and correlation maps of the field `X` on the index series `index` at the lags `lags`, with two-sided p-values,
    grid point by grid point over the pairs that are present, on the device.

    X            as in `anomalies` / `time_filter`: time first and any spatial shape S, real float32 or float64, NaN marking a
                 missing value (an Inf is refused): a numpy array, or a `torch.Tensor` on the handle's GPU in any layout
    index        shape (T,) or (T, q), 1 <= q <= 8: real and finite, no column constant.  It is converted to float64 and its column
                 means (ascending float64 sum / T) are subtracted on the host
    lags         a non-empty sequence of distinct integers in any order, |lag| <= T - 1, len(lags) * q <= 1024.  For lag l the
                 pairs are (index[s], X[s + l]) over s in [max(0, -l), min(T, T - l)) with X[s + l, n] present: a positive lag means
                 the index leads the field
    min_pairs    an integer >= 3: an entry with fewer pairs is not live
    dof          'n': the degrees of freedom of the p-value are the pair count n;  'bretherton' (Bretherton et al. 1999): the
                 effective sample size min(n, floor(n (1 - rho) / (1 + rho))) where rho = rho_x rho_y > 0, the product of the
                 lag-1 autocorrelations of the grid point (over its present neighbours; 'lag1' of the result) and of the index
    handle       a `_hip.Handle` (default: the one of the device); its resident fields and results are left as they are

    All sums are float64 chains in ascending time that start from +0.0, whatever the dtype of X, over x' = x - c_n (c_n the mean of
    the present values of the grid point, against cancellation) and the centred index y'.  With n the pair count,
    Cxx = Sxx - Sx^2 / n, Cyy = Syy - Sy^2 / n and Cxy = Sxy - Sx Sy / n, r = Cxy / sqrt(Cxx Cyy) clamped to [-1, 1] and
    slope = Cxy / Cyy (field units per index unit), both rounded once to the dtype of X.  An entry (lag, grid point, series) is
    live exactly when n >= min_pairs, Cxx > 2^-40 Sxx and Cyy > 2^-40 Syy - the second rule, a definition, rejects a series that is
    constant over the pairs of that lag.  An entry that is not live has r, slope and p NaN and dof 0.  p is the two-sided p-value of
    the returned r under the exact null distribution with `dof` samples, NaN where dof < 3.

    Returns a dict; with L = len(lags):
        'r', 'slope'   (L,) + S + (q,), dtype of X
        'p'            (L,) + S + (q,), float64
        'dof'          (L,) + S + (q,), int32
        'pairs'        (L,) + S, int32, for every grid point
        'lags'         (L,) int64, a numpy copy of the argument in the caller's order
        'lag1'         S, float64: rho_x (dof='bretherton' only)
    A 1-D index keeps the trailing axis of length 1.  For a tensor X every map - 'r', 'slope', 'p', 'dof', 'pairs', 'lag1' - is a GPU
    tensor that the device wrote; only 'lags' is numpy.  The maps of one lag depend neither on the other lags of the call nor on
    their order, and a call repeats its bits.  Every argument error is a ValueError raised before the library's device code is
    reached."""
    what = "lead_lag_maps"
    if isinstance(min_pairs, (bool, np.bool_)) or not isinstance(min_pairs, (int, np.integer)) or int(min_pairs) < 3:
        raise ValueError("%s: min_pairs must be an integer of at least 3, got %r" % (what, min_pairs))
    if not isinstance(dof, str) or dof not in ('n', 'bretherton'):
        raise ValueError("%s: dof must be 'n' or 'bretherton', got %r" % (what, dof))
    if _is_tensor(X):
        T = int(X.shape[0]) if X.dim() >= 1 else 0
    else:
        T = int(np.shape(X)[0]) if np.ndim(X) >= 1 else 0
    if T < 1:
        raise ValueError("%s: the field needs time first and at least one spatial dimension" % what)
    if T > _hip.PVALUE_MAX_OBS:
        raise ValueError("%s: at most %d time steps (the range of the p-value), got %d" % (what, _hip.PVALUE_MAX_OBS, T))
    y = _check_index(what, index, T)
    lag_list = _check_lags(what, lags, T, y.shape[1])
    field, shape, tensor = _check_field(what, X, handle)
    yc, _ = center_index(y)
    rho_y = lag1_index(yc) if dof == 'bretherton' else None
    h = handle if handle is not None else _hip.default_handle()
    r, slope, p, d, pairs, lag1 = h.lead_lag_maps(field, yc, lag_list, int(min_pairs), rho_y=rho_y,
                                                  alloc=_tensor_alloc(h.device) if tensor else None)
    S, L, q = tuple(shape[1:]), lag_list.size, y.shape[1]
    out = {'r': r.reshape((L,) + S + (q,)), 'slope': slope.reshape((L,) + S + (q,)), 'p': p.reshape((L,) + S + (q,)),
           'dof': d.reshape((L,) + S + (q,)), 'pairs': pairs.reshape((L,) + S), 'lags': lag_list.copy()}
    if lag1 is not None:
        out['lag1'] = lag1.reshape(S)
    return out
