"""`xmca_amd.gaps.fill_gaps` - DINEOF and M-SSA gap filling of a field on the device.

The model classes drop every grid point that holds a NaN, so a field with scattered gaps (clouds in a satellite record) has to be
completed before it is decomposed.  DINEOF (Beckers & Rixen 2003; Alvera-Azcarate et al. 2005) fills the gaps with the field's own
truncated EOF reconstruction and repeats until the filled values stop moving; the number of modes is chosen by withholding some
present values and comparing the reconstruction with them.  The whole loop runs on the device (xmca_fill_gaps); this module holds
the argument checks, the choice among candidates and the scatter back into the caller's shape.

    from xmca_amd.gaps import fill_gaps
    out = fill_gaps(sst, n_modes=(2, 4, 6, 8), cv_fraction=0.03, seed=0)
    MCA(out['field']).solve()

DINEOF rebuilds a value from the other grid points of its own time step, so a time step with nothing present (a missed overpass,
an outage) comes back as the column means.  `embedding=M, tau=` runs the same iteration on the field embedded with M windows tau
steps apart (M-SSA gap filling, Kondrashov & Ghil 2006): a value is rebuilt from its neighbours in time as well, and such time
steps are bridged.

    out = fill_gaps(sst, n_modes=6, embedding=12)
"""
import sys

import numpy as np

from . import _hip


def _is_tensor(x):
    torch = sys.modules.get('torch')
    return torch is not None and isinstance(x, torch.Tensor)


def _candidates(n_modes):
    """n_modes as a tuple of ints and whether it was given as a sequence."""
    if isinstance(n_modes, (int, np.integer)) and not isinstance(n_modes, bool):
        return (int(n_modes),), False
    try:
        ks = tuple(n_modes)
    except TypeError:
        raise ValueError("fill_gaps: n_modes must be an int or a sequence of ints, got %r" % (n_modes,)) from None
    if not ks or not all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) for k in ks):
        raise ValueError("fill_gaps: n_modes must be an int or a non-empty sequence of ints, got %r" % (n_modes,))
    ks = tuple(int(k) for k in ks)
    if any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError("fill_gaps: the candidates of n_modes must be strictly increasing, got %r" % (ks,))
    return ks, True


def _embedding(T, embedding, tau):
    """(embedding, tau, T') of a field of T time steps, checked; embedding = 1 is DINEOF and gives (1, 1, T)."""
    for name, v in (("embedding", embedding), ("tau", tau)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("fill_gaps: %s must be an int of at least 1, got %r" % (name, v))
    M, tau = int(embedding), int(tau)
    if M == 1:
        return 1, 1, T
    Tp = T - (M - 1) * tau
    if Tp < 2:
        raise ValueError("fill_gaps: T' = T - (embedding - 1) * tau = %d leaves fewer than two windows" % Tp)
    if tau > Tp:
        raise ValueError("fill_gaps: tau = %d above T' = %d leaves time steps outside every window (nothing to fill them from)" % (tau, Tp))
    return M, tau, Tp


def _prepare(X, n_modes, max_iter, tol, cv_fraction, cv_idx, seed, embedding=1, tau=1):
    """Every argument check of `fill_gaps`, without a device: (flat field T x N_full, kept columns, plane of the kept columns,
    candidates, is a sequence, withheld indices into the plane or None)."""
    if _is_tensor(X):
        raise ValueError("fill_gaps: torch tensors are out of scope of gap filling; pass a numpy array (tensor.cpu().numpy())")
    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        raise ValueError("fill_gaps: the field must be real float32 or float64, got %s" % X.dtype)
    if X.ndim < 2:
        raise ValueError("fill_gaps: the field needs time first and at least one spatial dimension, got shape %s" % (X.shape,))
    T = X.shape[0]
    flat = X.reshape(T, -1)
    if np.isinf(flat).any():
        raise ValueError("fill_gaps: the field holds an Inf (NaN marks a missing value)")
    present = np.isfinite(flat)
    keep = np.flatnonzero(present.any(axis=0))
    if keep.size == 0:
        raise ValueError("fill_gaps: the field holds no finite value")
    N = keep.size
    M, tau, Tp = _embedding(T, embedding, tau)
    ks, many = _candidates(n_modes)
    if M == 1 and (ks[0] < 1 or ks[-1] > min(T, N) - 1):
        raise ValueError("fill_gaps: n_modes must lie in [1, min(T, N) - 1] = [1, %d] (N counts the columns with a finite value), got %r"
                         % (min(T, N) - 1, ks if many else ks[0]))
    if M > 1 and (ks[0] < 1 or ks[-1] > min(Tp, M * N) - 1):
        raise ValueError("fill_gaps: n_modes must lie in [1, min(T', embedding * N) - 1] = [1, %d] (T' = %d windows; N counts the columns "
                         "with a finite value), got %r" % (min(Tp, M * N) - 1, Tp, ks if many else ks[0]))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError("fill_gaps: max_iter must be an int of at least 1, got %r" % (max_iter,))
    tol = float(tol)
    if not np.isfinite(tol) or tol < 0:
        raise ValueError("fill_gaps: tol must be finite and not negative, got %r" % (tol,))
    if cv_fraction is not None and cv_idx is not None:
        raise ValueError("fill_gaps: give cv_fraction or cv_idx, not both")
    plane = np.ascontiguousarray(flat[:, keep])
    withheld = None
    if cv_idx is not None:
        idx = np.asarray(cv_idx)
        if idx.ndim != 1 or idx.size == 0 or idx.dtype.kind not in 'iu':
            raise ValueError("fill_gaps: cv_idx must be a non-empty 1-D array of flat integer indices into X.reshape(T, -1)")
        idx = idx.astype(np.int64)
        if idx.min() < 0 or idx.max() >= flat.size:
            raise ValueError("fill_gaps: a cv_idx entry is out of range [0, %d)" % flat.size)
        if np.unique(idx).size != idx.size:
            raise ValueError("fill_gaps: a cv_idx entry is repeated")
        if not present.reshape(-1)[idx].all():
            raise ValueError("fill_gaps: a cv_idx entry points at a missing value")
        # flat index into T x N_full -> flat index into the plane of the kept columns (a present entry lies in a kept column)
        col_of = np.full(flat.shape[1], -1, dtype=np.int64)
        col_of[keep] = np.arange(N)
        withheld = (idx // flat.shape[1]) * N + col_of[idx % flat.shape[1]]
    elif cv_fraction is not None:
        frac = float(cv_fraction)
        if not 0.0 < frac < 1.0:
            raise ValueError("fill_gaps: cv_fraction must lie in (0, 1), got %r" % (cv_fraction,))
        where = np.flatnonzero(np.isfinite(plane).reshape(-1))
        n_cv = int(round(frac * where.size))
        if n_cv < 1:
            raise ValueError("fill_gaps: cv_fraction = %r of %d present entries withholds nothing" % (cv_fraction, where.size))
        withheld = np.sort(np.random.default_rng(seed).choice(where, size=n_cv, replace=False)).astype(np.int64)
    if many and withheld is None:
        raise ValueError("fill_gaps: choosing among candidates of n_modes needs a cross-validation set (cv_fraction or cv_idx)")
    return flat, keep, plane, ks, many, withheld


def fill_gaps(X, n_modes, max_iter=300, tol=1e-5, cv_fraction=None, cv_idx=None, seed=None, handle=None, embedding=1, tau=1):
    """DINEOF (embedding = 1) or M-SSA (embedding > 1) gap filling of `X`, a numpy array with time first and NaN at the missing values.

    n_modes      an int, or a strictly increasing sequence of ints: candidates, each run from a cold start with the
                 cross-validation set withheld; the one with the smallest `cv_rms` wins (the first on a tie), and one final run
                 with that number of modes and nothing withheld gives the field
    max_iter     most iterations of a run;  tol: a run ends when the RMS change of the filled values, relative to the RMS of the
                 present anomalies, falls below it (0: exactly max_iter iterations)
    cv_idx       flat indices into X.reshape(T, -1) of present entries to withhold;  cv_fraction: that share of the present entries
                 instead, drawn with numpy.random.default_rng(seed).  Required with candidates.
    handle       a `_hip.Handle` (default: the one of the device); its resident fields and results are left as they are
    embedding    M >= 1 windows of T' = T - (M - 1) tau time steps, `tau` steps apart: the iteration truncates the embedded field
                 [A_0 | ... | A_{M-1}], A_j = A[j tau : j tau + T'], and averages the M copies of a value (its anti-diagonal), so a
                 time step without any present value is filled from its neighbours in time.  1 (the default) is DINEOF, and `tau`
                 is then not looked at.  Needs T' >= 2, tau <= T' and n_modes in [1, min(T', M N) - 1].

    Returns a dict: 'field' (the shape and dtype of X; present values untouched; NaN only where a grid point has no value at any
    time), 'n_modes', 'iterations', 'converged', 'history' (the relative changes d_i), 'cv_rms' (None without a cross-validation
    set), 'cv_curve' ({k: cv_rms}, candidates only), 'singular_values' (eigenvalues of the last iterate's Gram matrix / (T - 1);
    with embedding > 1: of its lag-summed Gram matrix / (T' - 1)), and, with embedding > 1 only, 'embedding' and 'tau'.
    Every argument error is a ValueError raised before the device is touched."""
    flat, keep, plane, ks, many, withheld = _prepare(X, n_modes, max_iter, tol, cv_fraction, cv_idx, seed, embedding, tau)
    h = handle if handle is not None else _hip.default_handle()
    M, tau, Tp = _embedding(plane.shape[0], embedding, tau)
    max_iter, tol = int(max_iter), float(tol)
    if M == 1:
        def run(k, cv_idx=None):
            return h.fill_gaps(plane, k, max_iter, tol, cv_idx=cv_idx)
    else:
        def run(k, cv_idx=None):
            return h.fill_gaps_lagged(plane, k, M, tau, max_iter, tol, cv_idx=cv_idx)
    out = {}
    if many:
        curve = {}
        for k in ks:
            curve[k] = run(k, cv_idx=withheld)[2]
        best = min(ks, key=lambda k: (curve[k], ks.index(k)))
        out['cv_curve'] = curve
        out['cv_rms'] = curve[best]
        filled, history, _, lam = run(best)
    else:
        best = ks[0]
        filled, history, cv_rms, lam = run(best, cv_idx=withheld)
        out['cv_rms'] = cv_rms
    field = np.full(flat.shape, np.nan, dtype=flat.dtype)
    field[:, keep] = filled
    out['field'] = field.reshape(np.shape(X))
    out['n_modes'] = best
    out['iterations'] = int(history.size)
    out['converged'] = bool(history.size and history[-1] < tol)
    out['history'] = history
    out['singular_values'] = lam / (Tp - 1)
    if M > 1:
        out['embedding'] = M
        out['tau'] = tau
    return out
