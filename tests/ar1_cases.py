"""TEST INFRASTRUCTURE (never imported by the product): numpy twin of the red-noise surrogates of rule_n.

`ar1_filter(e, phi, dtype)` is the sequential recurrence of the definition and `lag1(x)` the centred two-sum estimate, both in
float64.  The normals come from `oracle/philox_numpy.py` without a GPU and from `Handle.surrogate` with one.
"""
import numpy as np

PHI_CYCLE = (0.0, 0.5, -0.5, 0.9, 0.999, -0.999)      # per-column phi of the filter tests, cycled over the columns


def ar1_filter(e, phi, dtype=np.float64):
    """x[0] = e[0], x[t] = phi x[t-1] + sqrt(1 - phi^2) e[t] down the columns of the (T, N) normals `e`, which are rounded to the
    run `dtype` first, as the generator stores them.  The state stays float64; the result holds the values rounded to `dtype`
    (as float64).  phi: a scalar or N values."""
    e = np.asarray(e, dtype=np.float64).astype(dtype).astype(np.float64)
    T, N = e.shape
    phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), (N,))
    a = np.sqrt((1.0 - phi) * (1.0 + phi))          # sqrt(1 - phi^2) without the cancellation near |phi| = 1
    x = np.empty_like(e)
    state = e[0].copy()
    x[0] = state
    for t in range(1, T):
        state = phi * state + a * e[t]
        x[t] = state
    return x.astype(dtype).astype(np.float64)


def lag1(x):
    """phi_c = sum_t (x[t] - m)(x[t+1] - m) / sum_t (x[t] - m)^2 of every column of the (T, N) field, in float64; 0 where the
    denominator is 0."""
    x = np.asarray(x, dtype=np.float64)
    d = x - x.mean(axis=0)
    num = np.sum(d[:-1] * d[1:], axis=0)
    den = np.sum(d * d, axis=0)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def cycled_phi(N):
    return np.array([PHI_CYCLE[c % len(PHI_CYCLE)] for c in range(N)])


def filter_bound(x, phi, T, dtype):
    """Per-column bound on |device - twin| of the filter: 16 eps64 max|x_c| min(T, 1 / (1 - |phi_c|)) - every step adds at most
    2 eps |x|, damped geometrically, the carry term is of the same size, 16 leaves a factor of about four - plus, for float32, one
    float32 ulp of max|x_c| for a rounding that flips on store."""
    amp = np.max(np.abs(x), axis=0)
    bound = 16 * np.finfo(np.float64).eps * amp * np.minimum(T, 1.0 / (1.0 - np.abs(phi)))
    if np.dtype(dtype) == np.float32:
        bound = bound + np.spacing(amp.astype(np.float32)).astype(np.float64)
    return bound
