"""The numpy truth of `MCA.extended_rule_n` and the cases shared by tests/test_extended_rule_n_host.py and
tests/test_gpu_extended_rule_n.py.

Definition.  Notation of tests/extended_eofs_cases.py: Y = embed(X), H centres every column over the T' rows, H Y = U S V^T,
lambda_k = s_k^2.  For a surrogate field R with the embedded matrix Y_R the statistic of mode k is Lambda_k(R) = ||H Y_R v_k||^2.
`truth` forms Y and Y_R explicitly and takes V from an SVD of H Y; `shift_sum` restates what the device does - W = R [V_0 | ... |
V_{M-1}], Q[t, c] = sum_j W[t + j tau, j k + c], the centred columns of Q squared and summed.

A projection on a single vector of a close pair is ill-conditioned: an error eps in the decomposition turns v_k by about
eps lambda_1 / (lambda_k - lambda_{k+1}).  Every field here therefore has a prescribed, well-separated leading spectrum
(`separated_field`), and tests/test_extended_rule_n_host.py asserts MIN_RELGAP behind every tested mode of every case."""
import numpy as np

import ar1_cases as A
from extended_eofs_cases import embed, masked_field, relgaps, svd_truth      # noqa: F401  (re-exported to the tests)

MIN_RELGAP = 0.2
# (name, T, N, M, tau, n_modes, seed): M = 1, 3 and 12; T' on and off the projection kernel's row tile; tau below and above it
CASES = [
    ("40x23_M1", 40, 23, 1, 1, 3, 1),
    ("41x17_M3_t2", 41, 17, 3, 2, 3, 2),
    ("130x65_M12_t1", 130, 65, 12, 1, 4, 3),
    ("64x300_M3_t5", 64, 300, 3, 5, 3, 4),
    ("107x33_M2_t40", 107, 33, 2, 40, 3, 5),
]
# the 3-d field with masked grid points: (name, T, spatial shape, masked flat indices, M, tau, n_modes, seed)
MASKED_CASE = ("48x5x6_masked_M3_t2", 48, (5, 6), (0, 7, 8, 19, 29), 3, 2, 3, 6)
# the cases of the full test (all of them have more than one segment of the AR(1) filter but the first)
RULE_N_CASES = [CASES[0], CASES[2], CASES[3]]
N_RUNS = 4
SEED = 20261020


def separated_field(T, N, seed=0, ratio=0.5, n_signals=6, noise=1e-3):
    """A T x N float64 field with a prescribed leading spectrum: signal i is the half-wave cos(pi (i + 1) (t + 1/2) / T) (the
    DCT-II basis: orthogonal over T, and so slow that its lagged copies are nearly the same vector, which keeps one leading
    eigenvalue per signal in the embedded matrix instead of a cluster of M) along a random orthonormal pattern with the
    amplitude ratio^i, plus white noise of the relative size `noise`; every column has its own scale in [0.5, 2], so that the
    column standard deviations of the null differ; centred over T."""
    rng = np.random.default_rng([seed, T, N])
    t = np.arange(T) + 0.5
    U = np.stack([np.cos(np.pi * (i + 1) * t / T) for i in range(n_signals)], axis=1) * np.sqrt(2.0 / T)
    V = np.linalg.qr(rng.standard_normal((N, n_signals)))[0]
    s = ratio ** np.arange(n_signals)
    X = (U * s) @ V.T + noise * rng.standard_normal((T, N)) / np.sqrt(T)
    X = X * np.linspace(0.5, 2.0, N)
    return X - X.mean(axis=0)


def masked_separated_field(T, shape, masked, seed=0):
    """(field of shape (T,) + shape with NaN at the masked points, its kept columns T x N' as solve() sees them, the kept mask)"""
    n = int(np.prod(shape))
    keep = np.ones(n, dtype=bool)
    keep[list(masked)] = False
    X = separated_field(T, int(keep.sum()), seed)
    full = np.full((T, n), np.nan)
    full[:, keep] = X
    return full.reshape((T,) + tuple(shape)), X, keep


def patterns(X, M, tau, k):
    """(lam: all T' eigenvalues, V: M N x k unit-norm patterns) from the SVD of the explicitly embedded, centred matrix"""
    ref = svd_truth(X, M, tau, k)
    return ref["lam"], ref["eofs"].reshape(-1, k)            # ((M, N, k) -> rows j N + n)


def truth(V, R, M, tau):
    """Lambda_c(R) = ||H Y_R v_c||^2 with Y_R formed explicitly"""
    Y = embed(np.asarray(R, dtype=np.float64), M, tau)
    Q = (Y - Y.mean(axis=0)) @ V
    return np.sum(Q * Q, axis=0)


def lag_project(W, M, tau, k):
    """the projection kernel in numpy: Q[t, c] = sum_j W[t + j tau, j k + c] (j = 0 first), then the sums of the squared, centred columns"""
    Tp = W.shape[0] - (M - 1) * tau
    Q = W[:Tp, :k].copy()
    for j in range(1, M):
        Q += W[j * tau:j * tau + Tp, j * k:(j + 1) * k]
    Q -= Q.mean(axis=0)
    return np.sum(Q * Q, axis=0)


def shift_sum(V, R, M, tau):
    """the device's route in numpy: one product over the whole surrogate, then the shift sum"""
    N, k = R.shape[1], V.shape[1]
    B = np.concatenate([V[j * N:(j + 1) * N] for j in range(M)], axis=1)          # N x M k
    return lag_project(np.asarray(R, dtype=np.float64) @ B, M, tau, k)


def red_surrogate(T, N, phi, seed, run, dtype=np.float64):
    """the unit-variance AR(1) surrogate of (seed, run, side 0) without a GPU: the Philox normals of oracle/philox_numpy.py through
    the sequential filter of tests/ar1_cases.py"""
    from oracle.philox_numpy import surrogate
    return A.ar1_filter(surrogate(T * N, seed, run, 0).reshape(T, N), phi, dtype)


# ---- planted signal ---------------------------------------------------------------------------------------------------------
PLANTED = {"T": 120, "N": 24, "M": 10, "tau": 1, "k": 6, "n_runs": 40, "field_seed": 11, "seed": 5, "period": 12.0, "amplitude": 1.5,
           "phi": 0.5}


def planted_field():
    """One oscillatory pair (a standing pattern times cos, another times sin, period 12 steps) in AR(1) noise of phi = 0.5 made
    with the library's own generator key (field_seed, run 0)"""
    p = PLANTED
    T, N = p["T"], p["N"]
    noise = red_surrogate(T, N, p["phi"], p["field_seed"], 0)
    rng = np.random.default_rng(p["field_seed"])
    a, b = np.linalg.qr(rng.standard_normal((N, 2)))[0].T
    w = 2.0 * np.pi * np.arange(T) / p["period"]
    X = noise + p["amplitude"] * np.sqrt(N) * (np.outer(np.cos(w), a) + np.outer(np.sin(w), b))
    return X - X.mean(axis=0)


def planted_truth():
    """(lam[:k], Lambda (n_runs x k)) of the planted case on the CPU, with the estimated phi and the column scale of the field"""
    p = PLANTED
    X = planted_field()
    lam, V = patterns(X, p["M"], p["tau"], p["k"])
    phi, d = A.lag1(X), X.std(axis=0, ddof=1)
    runs = np.array([truth(V, red_surrogate(p["T"], p["N"], phi, p["seed"], r) * d, p["M"], p["tau"]) for r in range(p["n_runs"])])
    return lam[:p["k"]], runs
