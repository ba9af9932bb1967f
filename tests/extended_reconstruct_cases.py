"""The numpy truth of `MCA.extended_reconstruct` and the cases shared by tests/test_extended_reconstruct_host.py
and tests/test_gpu_extended_reconstruct.py.  Notation as in tests/extended_eofs_cases.py.

Definition.  X: the T x N field as solve() sees it; M = embedding, T' = T - (M - 1) tau; Y = [X_0 | ... | X_{M-1}] with
X_j = X[j tau : j tau + T']; mu the row of column means of Y; Y - 1 mu^T = U S V^T.  For a set of modes the truncation is
Y^ = sum_k s_k u_k v_k^T, and with J(t) = {j : 0 <= j < M, 0 <= t - j tau < T'}, c_t = |J(t)|

    R[t, n] = (1 / c_t) sum_{j in J(t)} Y^[t - j tau, j N + n]          the reconstructed component (T x N)
    m[t, n] = (1 / c_t) sum_{j in J(t)} mu[j N + n]                     the window means, averaged the same way.

`truth` is this from the explicit SVD.  `route` restates what the device does: the eigenvectors Z of the doubly centred lag sum,
P = the products Z_sel^T X_j of the UNCENTRED windows (the vectors sum to zero) with the M rows of window means below them,
A~ = the lag-placed vectors with the M indicator columns beside them, R + m = diag(1 / c) A~ P.  `route(means=False)` and
`route(divide='M')` are the two mistakes the tests must see: the window means left out, and a division by M instead of c_t."""
import numpy as np

import extended_eofs_cases as E

# the mode groups of every mode-group case, as `mode` arguments (1-based; a slice has an inclusive stop): the modes 1, 2 and 3 alone
# as slices, the leading three as an int, the pair 2-3
MODE_GROUPS = [slice(1, 1), slice(2, 2), slice(3, 3), 3, slice(2, 3)]
# (name, T, N, M, tau, seed): the seeds of extended_eofs_cases guarantee MIN_RELGAP behind the modes 1-3
GROUP_CASES = [(name, T, N, M, tau, seed) for name, T, N, M, tau, k, seed in E.E2E_CASES]
LARGE_CASE = E.LARGE_CASE[:5] + (E.LARGE_CASE[6],)
MASKED_CASE = E.MASKED_CASE
# (T, N, M, tau): fields of `full_field`, whose centred embedded matrix has numerical rank T' - 1.  (34, 130, 2, 17): the windows
# abut and every c_t is 1; (12, 40, 1, 1): no embedding
COMPLETE_CASES = [(40, 96, 4, 3), (40, 96, 4, 1), (33, 257, 2, 16), (34, 130, 2, 17), (37, 130, 5, 2), (64, 200, 6, 1), (12, 40, 1, 1)]
MIN_TAIL_RATIO = 1e-3                 # lam_{T'-1} / lam_1 of every completeness case


def full_field(T, N, seed=0):
    """A T x N float64 field of full numerical rank: standard normal noise plus a linear trend along a random pattern (so that the
    window means differ from lag to lag), centred over T"""
    rng = np.random.default_rng([seed, T, N])
    X = rng.standard_normal((T, N)) + np.outer(np.linspace(-1.0, 1.0, T), rng.standard_normal(N))
    return X - X.mean(axis=0)


def mode_indices(mode, most):
    """0-based indices of the `mode` argument (None, int n: modes 1..n, 1-based slice with an inclusive stop) among `most` modes"""
    if mode is None:
        return np.arange(most)
    if isinstance(mode, slice):
        return np.arange(0 if mode.start is None else mode.start - 1, most if mode.stop is None else mode.stop, mode.step or 1)
    return np.arange(int(mode))


def n_modes(X, M, tau):
    """min(T' - 1, M N)"""
    return min(X.shape[0] - (M - 1) * tau - 1, M * X.shape[1])


def counts(T, M, tau):
    """c_t: the number of windows j with 0 <= t - j tau < T'"""
    Tp = T - (M - 1) * tau
    c = np.zeros(T, dtype=np.int64)
    for j in range(M):
        c[j * tau:j * tau + Tp] += 1
    return c


def diagonal_average(Yhat, M, tau, c=None):
    """R[t, n] = (1 / c_t) sum_{j in J(t)} Yhat[t - j tau, j N + n] for the T' x (M N) matrix Yhat; `c`: another divisor"""
    Tp, MN = Yhat.shape
    N = MN // M
    T = Tp + (M - 1) * tau
    R = np.zeros((T, N))
    for j in range(M):
        R[j * tau:j * tau + Tp] += Yhat[:, j * N:(j + 1) * N]
    return R / (counts(T, M, tau) if c is None else c)[:, None]


def truth(X, M, tau, modes, means=False):
    """The definition: R (means=True: R + m) of the 0-based `modes` from the SVD of the explicitly embedded, centred matrix"""
    X = np.asarray(X, dtype=np.float64)
    Y = E.embed(X, M, tau)
    mu = Y.mean(axis=0)
    u, s, vt = np.linalg.svd(Y - mu, full_matrices=False)
    modes = np.asarray(modes)
    Yhat = (u[:, modes] * s[modes]) @ vt[modes]
    if means:
        Yhat = Yhat + mu
    return diagonal_average(Yhat, M, tau)


def expand(Z, M, tau, with_indicators):
    """A~ (T x M (q + 1), or T x M q) of the q x T' matrix Z: A~[t, j q + c] = Z[c, t - j tau] inside window j, else 0;
    A~[t, M q + j] = 1 inside window j, else 0"""
    q, Tp = Z.shape
    T = Tp + (M - 1) * tau
    A = np.zeros((T, M * (q + (1 if with_indicators else 0))))
    for j in range(M):
        A[j * tau:j * tau + Tp, j * q:(j + 1) * q] = Z.T
        if with_indicators:
            A[j * tau:j * tau + Tp, M * q + j] = 1.0
    return A


def window_means(X, M, tau):
    """(M, N): the means of the windows X[j tau : j tau + T'] of every column, in float64"""
    X = np.asarray(X, dtype=np.float64)
    Tp = X.shape[0] - (M - 1) * tau
    return np.stack([X[j * tau:j * tau + Tp].sum(axis=0) / Tp for j in range(M)])


def route(X, M, tau, modes, means=True, divide='count'):
    """The device's route in numpy.  means=False leaves the window means out (the result is then R); divide='M' is the mistake of
    dividing by the number of lags instead of c_t"""
    X = np.asarray(X, dtype=np.float64)
    T = X.shape[0]
    Tp = T - (M - 1) * tau
    lam, Z = np.linalg.eigh(E.double_center(E.lag_sum(X @ X.T, M, tau)))
    Zsel = np.ascontiguousarray(Z[:, ::-1][:, np.asarray(modes)].T)
    P = [Zsel @ X[j * tau:j * tau + Tp] for j in range(M)]
    if means:
        P.append(window_means(X, M, tau))
    A = expand(Zsel, M, tau, means)
    c = counts(T, M, tau) if divide == 'count' else np.full(T, M)
    return (A @ np.concatenate(P, axis=0)) / c[:, None]


def tail_ratio(X, M, tau):
    """lam_{T'-1} / lam_1 of the centred embedded matrix"""
    Y = E.embed(np.asarray(X, dtype=np.float64), M, tau)
    s = np.linalg.svd(Y - Y.mean(axis=0), compute_uv=False)
    Tp = Y.shape[0]
    return (s[Tp - 2] / s[0]) ** 2


def masked_full_field(T, shape, masked, seed=0):
    """(field (T,) + shape with NaN at the masked points, its kept columns T x N' from `full_field`, the keep mask)"""
    n = int(np.prod(shape))
    keep = np.ones(n, dtype=bool)
    keep[list(masked)] = False
    X = full_field(T, int(keep.sum()), seed)
    full = np.full((T, n), np.nan)
    full[:, keep] = X
    return full.reshape((T,) + tuple(shape)), X, keep
