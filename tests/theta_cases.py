"""The Theta fore/back-cast extension of solve(complexify=True, extend='theta', period=m) restated in numpy, and the columns the
tests fit (tests/test_theta_extension_host.py, tests/test_gpu_theta_extension.py, tests/test_theta_statsmodels_twin.py,
scripts/extend_theta_accuracy.py).  The product does not import this module.

The restatement follows DESIGN.md 2.11, which states `ThetaModel(y, period=m, deseasonalize=True, use_test=False).fit()
.forecast(steps=T, theta=20)` from the published algorithm (it has not been compared with statsmodels on any machine:
tests/test_theta_statsmodels_twin.py does that where statsmodels is installed).  For one centred real column y of length n:

  seasonal   additive; m = 1: s = 0.  m >= 2: centred moving average of length m (weights 1/m, the two ends 1/(2m) for even m),
             defined for t in [h, n - h), h = m // 2; d_t = y_t - trend_t there; a_p the mean of d_t over t = p (mod m);
             s_p = a_p - mean_p(a_p); z_t = y_t - s[t mod m].  n >= 2m.
  drift      b0: least-squares slope of z on t.
  smoothing  l_0 = z_0, e_t = z_t - l_{t-1}, l_t = l_{t-1} + alpha e_t, SSE = sum e_t^2; alpha minimises SSE on [1e-4, 1 - 1e-4] by
             six rounds of 33 candidates a_i = lo + (hi - lo) i / 32, j the first argmin, next round on [a_max(j-1,0), a_min(j+1,32)];
             level = l_{n-1}(alpha).
  forecast   f_h = 0.95 b0 (h + (1 - (1 - alpha)^n) / alpha) + level + s[(n + h) mod m], h = 0 .. n-1; the backcast is the same map
             of the reversed column, reversed.

Every sum is taken in the order of its index, one operation at a time, over all columns at once (arrays n x N)."""
import numpy as np
from scipy.signal import hilbert

ALPHA_LO, ALPHA_HI = 1e-4, 1.0 - 1e-4
ROUNDS, CAND = 6, 33
ALPHA_STEP = 2.0 * 16.0 ** -6          # the bound of the tests on alpha (the last round's candidates are 16^-6 / 2 apart)
MIN_GAP = 1e-6                         # condition on the test columns: see `first_round_gap`


def seasonal_means(Y, m):
    """(m, N) seasonal means s_p of the columns of Y (n x N)."""
    Y = np.asarray(Y, dtype=np.float64)
    n, N = Y.shape
    if m < 1 or n < 2 * m:
        raise ValueError("the Theta extension needs period >= 1 and n >= 2 period")
    if m == 1:
        return np.zeros((1, N))
    h = m // 2
    sums = np.zeros((m, N))
    count = np.zeros(m)
    for t in range(h, n - h):
        if m % 2:
            acc = Y[t - h].copy()
            for k in range(1, m):
                acc = acc + Y[t - h + k]
        else:
            acc = 0.5 * Y[t - h]
            for k in range(1, m):
                acc = acc + Y[t - h + k]
            acc = acc + 0.5 * Y[t + h]
        sums[t % m] = sums[t % m] + (Y[t] - acc / m)
        count[t % m] += 1
    a = sums / count[:, None]
    mean = np.zeros(N)
    for p in range(m):
        mean = mean + a[p]
    return a - mean / m


def deseasonalised(Y, m, s=None):
    Y = np.asarray(Y, dtype=np.float64)
    s = seasonal_means(Y, m) if s is None else s
    return Y - s[np.arange(Y.shape[0]) % m]


def drift(Z):
    """Least-squares slope of every column of Z on t."""
    n = Z.shape[0]
    tbar = 0.5 * (n - 1)
    num = np.zeros(Z.shape[1])
    for t in range(n):
        num = num + (t - tbar) * Z[t]
    return num / (n * (n * n - 1.0) / 12.0)


def smooth(Z, alpha):
    """(SSE, final level) of simple exponential smoothing of the columns of Z; alpha: (..., N) - one value per column, or a stack
    of candidates per column."""
    alpha = np.asarray(alpha, dtype=np.float64)
    level = np.broadcast_to(Z[0], alpha.shape).copy()
    sse = np.zeros(alpha.shape)
    for t in range(1, Z.shape[0]):
        e = Z[t] - level
        level = level + alpha * e
        sse = sse + e * e
    return sse, level


def grid_zoom(Z):
    """alpha of every column by the fixed grid zoom; also the SSE of the first round's candidates (CAND x N)."""
    N = Z.shape[1]
    lo = np.full(N, ALPHA_LO)
    hi = np.full(N, ALPHA_HI)
    frac = (np.arange(CAND) / 32.0)[:, None]
    first = None
    cols = np.arange(N)
    for _ in range(ROUNDS):
        a = lo + (hi - lo) * frac
        sse, _level = smooth(Z, a)
        if first is None:
            first = sse
        j = np.argmin(sse, axis=0)                   # the lowest index on ties
        alpha = a[j, cols]
        lo, hi = a[np.maximum(j - 1, 0), cols], a[np.minimum(j + 1, CAND - 1), cols]
    return alpha, first


def first_round_gap(sse):
    """Smallest relative SSE gap between the first round's argmin and any local minimum of that round that is not next to it, over the
    columns of sse (CAND x N); inf where there is none.  The candidate choice of a test column must not hinge on rounding."""
    worst = np.inf
    for c in range(sse.shape[1]):
        v = sse[:, c]
        j = int(np.argmin(v))
        if not v[j] > 0:
            continue                                  # (the all-zero column: every candidate ties, the lowest index wins)
        for i in range(CAND):
            left = v[i - 1] if i > 0 else np.inf
            right = v[i + 1] if i < CAND - 1 else np.inf
            if abs(i - j) > 1 and v[i] < left and v[i] < right:
                worst = min(worst, (v[i] - v[j]) / v[j])
    return worst


def fit(Y, m, alpha=None):
    """The fit of every column of Y (n x N): dict of alpha (N), b0 (N), level (N), s (m x N) and the first round's SSE.  With `alpha`
    given (N values) the search is skipped."""
    Y = np.asarray(Y, dtype=np.float64)
    s = seasonal_means(Y, m)
    Z = deseasonalised(Y, m, s)
    b0 = drift(Z)
    first = None
    if alpha is None:
        alpha, first = grid_zoom(Z)
    alpha = np.asarray(alpha, dtype=np.float64)
    sse, level = smooth(Z, alpha)
    return {"alpha": alpha, "b0": b0, "level": level, "s": s, "sse": sse, "first_round": first}


def forecast(f, n, m):
    """(n x N) forecast of a fit."""
    alpha = f["alpha"]
    pw = np.ones_like(alpha)
    for _ in range(n):
        pw = pw * (1.0 - alpha)
    A = (1.0 - pw) / alpha
    h = np.arange(n)
    return 0.95 * f["b0"] * (h[:, None] + A) + f["level"] + f["s"][(n + h) % m]


def coefficients(f, n, m):
    """(2 + m, N): the forecast in the basis of `_hip.theta_forecast_basis` - 1, h, the phases of (n + h) mod m."""
    alpha = f["alpha"]
    pw = np.ones_like(alpha)
    for _ in range(n):
        pw = pw * (1.0 - alpha)
    slope = 0.95 * f["b0"]
    return np.concatenate([(f["level"] + slope * ((1.0 - pw) / alpha))[None], slope[None], f["s"]])


def fits(Y, m, alpha=None):
    """Forecast and backcast fits of the columns of Y; alpha: None or the pair of (N,) arrays to evaluate at."""
    Y = np.asarray(Y, dtype=np.float64)
    return (fit(Y, m, None if alpha is None else alpha[0]), fit(Y[::-1], m, None if alpha is None else alpha[1]))


def packed(pair):
    """The layout of xmca_theta_fit: (2, 3 + m, N) - rows alpha, b0, level, s_0 .. s_{m-1}."""
    return np.stack([np.concatenate([f["alpha"][None], f["b0"][None], f["level"][None], f["s"]]) for f in pair])


def remove_mean(a):
    return a - a.mean(axis=0)


def analytic_signal(Y, m, pair=None):
    """The reference's `_complexify` (xmca/array.py:429-472) on the restated forecasts: [pre; y; post], hilbert at 3n, the trim to
    [n, 2n), remove_mean.  complex128, n x N."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[0]
    pair = fits(Y, m) if pair is None else pair
    post = forecast(pair[0], n, m)
    pre = forecast(pair[1], n, m)[::-1]
    return remove_mean(hilbert(np.concatenate([pre, Y, post]), axis=0)[n:2 * n])


def shifted(pair, Y, m, step):
    """The fits re-evaluated with every alpha moved by `step` (clipped to the search interval)."""
    alphas = [np.clip(f["alpha"] + step, ALPHA_LO, ALPHA_HI) for f in pair]
    return fits(Y, m, alphas)


def tolerances(Y, m, pair=None):
    """Bounds of the device tests, derived from the restatement alone: a device alpha may differ by ALPHA_STEP, so every quantity may
    differ by 4 x the change of the restatement's own value when its alpha moves by that step (either way), plus a rounding floor of
    64 eps n max |Y|.  Returns dict: 'fit' (2, 3 + m, N) with ALPHA_STEP in the alpha rows, 'planes' (scalar, for max |X_im|)."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[0]
    pair = fits(Y, m) if pair is None else pair
    floor = 64 * np.finfo(np.float64).eps * n * max(np.abs(Y).max(), np.finfo(np.float64).tiny)
    base = packed(pair)
    im = analytic_signal(Y, m, pair).imag
    d_fit = np.zeros_like(base)
    d_im = 0.0
    for step in (-ALPHA_STEP, ALPHA_STEP):
        moved = shifted(pair, Y, m, step)
        d_fit = np.maximum(d_fit, np.abs(packed(moved) - base))
        d_im = max(d_im, np.abs(analytic_signal(Y, m, moved).imag - im).max())
    tol = 4 * d_fit + floor
    tol[:, 0] = ALPHA_STEP
    return {"fit": tol, "planes": 4 * d_im + floor}


# ---- the columns of the tests ---------------------------------------------------------------------------------------------------
def columns(T, N, m, seed):
    """T x N centred float64 test field: column c mod 6 is 0: trend + season + random walk + noise (alpha interior), 1: white noise
    (alpha at the lower bound), 2: a random walk (alpha at the upper bound), 3: season + noise, 4: all zeros (a constant grid point
    after centring), 5: trend + smoothed random walk."""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)
    X = np.zeros((T, N))
    for c in range(N):
        kind = c % 6
        season = rng.standard_normal(m)[np.arange(T) % m] if m > 1 else np.zeros(T)
        walk = np.cumsum(rng.standard_normal(T))
        noise = rng.standard_normal(T)
        if kind == 0:
            X[:, c] = 0.3 * rng.standard_normal() * t + 2.0 * season + walk + 0.7 * noise
        elif kind == 1:
            X[:, c] = noise
        elif kind == 2:
            X[:, c] = walk * (1.0 + rng.random())
        elif kind == 3:
            X[:, c] = 3.0 * season + 0.5 * noise
        elif kind == 4:
            X[:, c] = 5.0
        else:
            X[:, c] = 0.1 * t + 0.5 * walk + 0.5 * np.concatenate([walk[:1], walk[:-1]])
    return X - X.mean(axis=0)


def checked_fits(X, m):
    """Forecast and backcast fits of the field, after asserting the condition on the inputs: no column's first-round choice hinges
    on rounding."""
    pair = fits(X, m)
    for f in pair:
        gap = first_round_gap(f["first_round"])
        assert gap >= MIN_GAP, "a test column has a second SSE minimum within %g of the first round's argmin: %g" % (MIN_GAP, gap)
    return pair


M_VALUES = (1, 2, 3, 4, 12)
N_VALUES = (1, 63, 65, 130)


def lengths(m):
    """T = 2m (one defined detrended value per phase for even m), 2m + 1, and a T with T mod m outside {0, 1} (m >= 3; for m = 1, 2
    there is none and a longer odd series stands in)."""
    return (2 * m, 2 * m + 1, 3 * m + 2 if m >= 3 else 9)
