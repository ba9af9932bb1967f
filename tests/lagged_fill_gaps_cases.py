"""The numpy restatement of `xmca_amd.gaps.fill_gaps(embedding=M, tau=)` (M-SSA gap filling) and the cases shared
by tests/test_lagged_fill_gaps_host.py and tests/test_gpu_lagged_fill_gaps.py.

Algorithm, as the device runs it.  Plane A, mask, column means and scale are those of DINEOF (tests/fill_gaps_cases.py `center`),
formed once.  With T' = T - (M - 1) tau, A_j = A[j tau : j tau + T'], J(t) = { j < M : 0 <= t - j tau < T' } and c_t = |J(t)|,
iteration i replaces A at the masked entries by the diagonally averaged rank-k truncation of Y = [A_0 | ... | A_{M-1}]:
    R[t] = (1 / c_t) sum_{j in J(t)} Y_k[t - j tau, block j]
and d_i = sqrt(sum of the squared changes / masked entries) / scale.  Two float64 routes to R that differ only in rounding: `gram`
(G = A A^T, K = sum_j G[j tau : j tau + T', j tau : j tau + T'], Z the k leading eigenvectors of K, P_j = Z A_j,
R[t] = (1 / c_t) sum_j Z[:, t - j tau] . P_j - the device's route) and `svd` (Y itself, numpy.linalg.svd, truncation, averaging).
`arithmetic='float32'` is the gram route with the plane stored in float32 and the Gram and projection products in float32
arithmetic (eigenvectors and the fill's sums stay float64, as on the device): its distance from the float64 restatement on the
same float32 input is eps32, the measure of the float32 tests' tolerance."""
import numpy as np

import fill_gaps_cases as D

TILE_ROWS, TILE_COLS, MODE_CHUNK = D.TILE_ROWS, D.TILE_COLS, D.MODE_CHUNK

# (T, N, k, M, tau, frac, dead): k modes, M windows tau steps apart, a share frac of the entries removed at random and `dead` whole
# time steps removed
CASES = [
    (120, 40, 4, 12, 1, 0.3, 8),
    (63, 255, 4, 2, 1, 0.3, 3),
    (64, 256, 4, 3, 1, 0.2, 3),
    (65, 257, 4, 5, 3, 0.4, 3),          # both sides of the 64 x 256 tile
    (97, 65, 4, 6, 2, 0.3, 5),
    (150, 30, 4, 24, 3, 0.3, 10),        # the lag span 69 exceeds a row tile; T' = 81
    (80, 33, 2, 2, 40, 0.3, 0),          # tau = T': every c_t = 1
]
DEAD_CASES = [c for c in CASES if c[6] > 0]
STATE_ITERATIONS = 25
# T' = 798 >= 768: the eigensolver reduces to tridiagonal form and gives the k leading vectors alone (no polish)
LARGE_CASE = (800, 900, 4, 3, 1, 0.3, 8)
# T' = 764 < 768 <= T = 780: the block Jacobi sweeps and the polish - the route is chosen at T', not at T
EDGE_CASE = (780, 64, 4, 5, 4, 0.3, 8)
BIG_ITERATIONS = 5
CV_CASE, CV_SHARE, CV_SEED, CV_CANDIDATES = CASES[0], 0.05, 3, (1, 2, 4)
CONVERGENCE_CASE, CONVERGENCE_TOL = (40, 30, 4, 4, 1, 0.2, 2), 1e-8
DEVICE_DEAD_CASES = [CASES[0], CASES[3]]
DEAD_RATIO, DINEOF_DEAD_RATIO = 0.5, 0.99
# the kernel alone: (T, N) x k x (M, tau)
KERNEL_PLANES = [(63, 255), (64, 256), (65, 257), (150, 30)]
KERNEL_MODES = [1, 16, 17]


def kernel_embeddings(T):
    """(M, tau) of the kernel tests on a plane of T rows: no lag, neighbours, a stride, a span above a row tile (T = 150), and
    tau = T' with two windows where T is even"""
    out = [(1, 1), (2, 1), (5, 3)]
    if T == 150:
        out.append((24, 3))
    if T % 2 == 0:
        out.append((2, T // 2))
    return out


def case_name(case):
    return "%dx%d_k%d_M%d_tau%d_f%g_dead%d" % case


def case_field(case, dtype=np.float64, seed=0):
    """(X with NaN gaps, truth, dead rows): a travelling wave with a modulated amplitude, a second wave against it, AR(1) noise
    (coefficient 0.5, unit variance, x 0.3) and an offset that grows along x"""
    T, N, k, M, tau, frac, dead = case
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)[:, None]
    x = np.arange(N, dtype=np.float64)[None, :]
    e = np.empty((T, N))
    e[0] = rng.standard_normal(N)
    w = rng.standard_normal((T, N)) * np.sqrt(1 - 0.25)
    for i in range(1, T):
        e[i] = 0.5 * e[i - 1] + w[i]
    truth = (np.cos(2 * np.pi * (t / 12 - x / N)) * (1 + 0.3 * np.sin(2 * np.pi * x / N)) + 0.5 * np.cos(2 * np.pi * (t / 7.3 + 2 * x / N))
             + 0.3 * e + 3 + 0.01 * x).astype(dtype)
    X = truth.copy()
    X[rng.random((T, N)) < frac] = np.nan
    rows = np.sort(rng.choice(np.arange(2, T - 2), size=dead, replace=False)) if dead else np.zeros(0, dtype=np.int64)
    X[rows, :] = np.nan
    return X, truth, rows


def windows(T, M, tau):
    """(T', c_t for every t)"""
    Tp = T - (M - 1) * tau
    count = np.zeros(T)
    for j in range(M):
        count[j * tau:j * tau + Tp] += 1
    return Tp, count


def averaged(Z, P, T, M, tau, mistake=None):
    """diag(1 / c) A~ P: R[t] = (1 / c_t) sum_{j in J(t)} Z[:, t - j tau] . P[j k : (j + 1) k].  Z k x T', P M k x N.  The planted
    mistakes of the host tests: 'by_M' divides by M instead of c_t, 'no_shift' takes Z[:, t] (the last window row past T') for
    every lag."""
    k = Z.shape[0]
    Tp, count = windows(T, M, tau)
    R = np.zeros((T, P.shape[1]))
    for j in range(M):
        lo = j * tau
        if mistake == "no_shift":
            R[lo:lo + Tp] += Z[:, np.minimum(np.arange(lo, lo + Tp), Tp - 1)].T @ P[j * k:(j + 1) * k]
        else:
            R[lo:lo + Tp] += Z.T @ P[j * k:(j + 1) * k]
    return R / (M if mistake == "by_M" else count[:, None])


def truncation(A, k, M, tau, route, mistake=None, arithmetic="float64"):
    """(the diagonally averaged rank-k truncation of the embedded A, the k leading eigenvalues of the lag-summed Gram matrix)"""
    T, N = A.shape
    Tp, count = windows(T, M, tau)
    if route == "svd":
        Y = np.hstack([A[j * tau:j * tau + Tp] for j in range(M)])
        U, s, Vt = np.linalg.svd(Y, full_matrices=False)
        Yk = (U[:, :k] * s[:k]) @ Vt[:k]
        R = np.zeros((T, N))
        for j in range(M):
            R[j * tau:j * tau + Tp] += Yk[:, j * N:(j + 1) * N]
        return R / count[:, None], s[:k] ** 2
    low = arithmetic == "float32"
    A_ = A.astype(np.float32) if low else A
    G = (A_ @ A_.T).astype(np.float64)
    K = np.zeros((Tp, Tp))
    for j in range(M):
        K += G[j * tau:j * tau + Tp, j * tau:j * tau + Tp]
    lam, V = np.linalg.eigh(K)
    Z = V[:, ::-1][:, :k].T
    Z_ = Z.astype(np.float32) if low else Z
    P = np.vstack([(Z_ @ A_[j * tau:j * tau + Tp]).astype(np.float64) for j in range(M)])
    return averaged(Z, P, T, M, tau, mistake), lam[::-1][:k]


def mssa_fill(X, k, M, tau, max_iter, tol, cv_idx=None, route="gram", mistake=None, arithmetic="float64"):
    """The restatement (of a float32 field too; in float64 unless arithmetic = 'float32').  Returns what `fill_gaps_cases.dineof`
    returns; 'lam' are the k leading eigenvalues of the last iterate's lag-summed Gram matrix."""
    X = np.asarray(X, dtype=np.float64)
    mean, A, mask, scale = D.center(X)
    low = arithmetic == "float32"
    if low:
        A = A.astype(np.float32).astype(np.float64)
    saved = None
    if cv_idx is not None:
        saved = A.reshape(-1)[cv_idx].copy()
        A.reshape(-1)[cv_idx] = 0.0
        mask = mask.copy()
        mask.reshape(-1)[cv_idx] = True
    n_masked = int(mask.sum())
    history, lam = [], None
    for _ in range(max_iter):
        R, lam = truncation(A, k, M, tau, route, mistake, arithmetic)
        new = R[mask].astype(np.float32).astype(np.float64) if low else R[mask]
        d = np.sqrt(np.sum((new - A[mask]) ** 2) / n_masked) / scale
        A[mask] = new
        history.append(float(d))
        if d < tol:
            break
    cv_rms = None if saved is None else float(np.sqrt(np.mean((A.reshape(-1)[cv_idx] - saved) ** 2)))
    field = np.where(np.isfinite(X), X, A + mean)
    if low:
        field = np.where(np.isfinite(X), X, (A + mean).astype(np.float32).astype(np.float64))
    return {"field": field, "history": np.array(history), "iterations": len(history), "converged": bool(history[-1] < tol),
            "cv_rms": cv_rms, "lam": lam}


def dead_step_ratio(field, X, truth, rows):
    """RMS error of `field` at the wholly missing time steps against the truth, over that of filling with the column means"""
    mean = D.center(X)[0]
    field = np.asarray(field, dtype=np.float64)
    by_mean = np.broadcast_to(mean, X.shape)[rows] - truth[rows]
    return float(np.sqrt(np.mean((field[rows] - truth[rows]) ** 2)) / np.sqrt(np.mean(by_mean ** 2)))


_cache = {}


def iterations_of(case):
    return BIG_ITERATIONS if case in (LARGE_CASE, EDGE_CASE) else STATE_ITERATIONS


def reference(case, dtype=np.float64, route="gram", cv=False, k=None, mistake=None, arithmetic="float64", embedded=True):
    """The restatement after the case's iterations (tol = 0) on its field of `dtype`, computed once per process; embedded = False:
    the same with M = 1 (DINEOF)"""
    key = (case, np.dtype(dtype).name, route, cv, k, mistake, arithmetic, embedded)
    if key not in _cache:
        T, N, kk, M, tau, frac, dead = case
        X = case_field(case, dtype)[0]
        idx = D.cv_indices(X, CV_SHARE, CV_SEED) if cv else None
        out = mssa_fill(X, kk if k is None else k, M if embedded else 1, tau if embedded else 1, iterations_of(case), 0.0, cv_idx=idx,
                        route=route, mistake=mistake, arithmetic=arithmetic)
        out["field"].setflags(write=False)
        _cache[key] = out
    return _cache[key]


def route_delta(case, dtype=np.float64, cv=False, k=None):
    """delta of the state-for-state comparison: the larger of the difference between the two float64 routes on the case and
    2^-52 max|X|"""
    a = reference(case, dtype, route="gram", cv=cv, k=k)["field"]
    b = reference(case, dtype, route="svd", cv=cv, k=k)["field"]
    return max(float(np.max(np.abs(a - b))), 2.0 ** -52 * float(np.max(np.abs(a))))


def eps32(case):
    """max |float32-arithmetic restatement - float64 restatement| on the case's float32 field"""
    a = reference(case, np.float32, arithmetic="float32")["field"]
    b = reference(case, np.float32)["field"]
    return float(np.max(np.abs(a - b)))
