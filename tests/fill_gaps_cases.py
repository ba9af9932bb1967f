"""The numpy restatement of `xmca_amd.gaps.fill_gaps` (DINEOF) and the cases shared by
tests/test_fill_gaps_host.py and tests/test_gpu_fill_gaps.py.

Algorithm, as the device runs it.  X is T x N with NaN at the missing values.  Every column is centred over its present values;
missing entries of the anomaly plane A start at 0; `scale` is the RMS of the present anomalies.  Withheld entries (cross-validation)
are saved, zeroed and treated as missing.  Iteration i: the rank-k truncation R of A replaces A at the masked entries, d_i =
sqrt(sum of the squared changes / masked entries) / scale; the loop ends with d_i < tol or after max_iter iterations.  The field is
X with A + mean at its missing entries.  Two float64 routes to R that differ only in rounding: `gram` (eigenvectors Z of A A^T,
P = Z A, R = Z^T P - the device's route) and `svd` (U_k S_k V_k^T)."""
import numpy as np

TILE_ROWS, TILE_COLS, MODE_CHUNK = 64, 256, 16       # of the fill kernel; the GPU tests check them against xmca_gap_fill_tile

# (T, N, r, k, frac): r separable modes in the field, k modes in the reconstruction, frac of the entries removed at random
MAIN_CASES = [
    (40, 30, 2, 2, 0.2),
    (60, 150, 3, 3, 0.3),
    (97, 333, 4, 4, 0.5),
]
# both sides of the tile edges of the fill kernel, in rows and in columns
EDGE_CASES = [
    (TILE_ROWS - 1, TILE_COLS - 1, 3, 3, 0.3),
    (TILE_ROWS + 1, TILE_COLS + 1, 3, 3, 0.3),
    (TILE_ROWS - 1, TILE_COLS + 1, 3, 3, 0.3),
    (TILE_ROWS + 1, TILE_COLS - 1, 3, 3, 0.3),
]
ONE_MODE_CASE = (40, 30, 1, 1, 0.2)
STATE_CASES = MAIN_CASES + EDGE_CASES + [ONE_MODE_CASE]          # every one has k = r
ILL_CONDITIONED_CASE = (60, 150, 3, 5, 0.3)                      # k > r: kept out of the state-for-state comparisons
# T = 800 is past the order (768) from which the eigensolver reduces to tridiagonal form and forms the k leading vectors only:
# the other side of the loop's one branch.  Five iterations keep the numpy restatement (an 800 x 800 eigh each) to seconds.
LARGE_CASE, LARGE_ITERATIONS = (800, 900, 3, 3, 0.3), 5
# shapes (T, N, k) of the kernel tests: the edges, one mode, one k above the chunk of modes a lane holds, two chunks and a bit
KERNEL_SHAPES = [(c[0], c[1], c[3]) for c in EDGE_CASES] + [(40, 30, 1), (70, 300, MODE_CHUNK + 1), (33, 65, 2 * MODE_CHUNK + 3)]
STATE_ITERATIONS = 25
CONVERGENCE_CASE, CONVERGENCE_TOL, CONVERGENCE_ITERATIONS = MAIN_CASES[0], 1e-8, 27
RECOVERY_RATIO = 0.25
CV_CASE, CV_SEED, CV_SHARE, CV_CANDIDATES = MAIN_CASES[0], 3, 0.05, (1, 2, 3)


def case_name(case):
    return "%dx%d_r%d_k%d_f%g" % case


def case_field(T, N, r, frac, dtype=np.float64):
    """(X with NaN gaps, truth): r separable modes, an offset that grows along x, noise; a share `frac` of the entries removed at
    random and the rows 5..8 removed over the columns 20 .. N/2 (a block gap)."""
    rng = np.random.default_rng(1)
    t = np.arange(T, dtype=np.float64)[:, None]
    x = np.arange(N, dtype=np.float64)[None, :]
    truth = 5.0 + 2.0 * x / N + np.zeros((T, 1))
    for c in range(r):
        truth = truth + (r - c) * np.sin(2 * np.pi * ((c + 1) * 3 * t / T + 0.37 * c)) * np.cos(2 * np.pi * ((c + 1) * x / N + 0.11 * c))
    truth = (truth + 0.1 * rng.standard_normal((T, N))).astype(dtype)
    X = truth.copy()
    X[rng.random((T, N)) < frac] = np.nan
    X[5:9, 20:N // 2] = np.nan
    return X, truth


def cv_indices(X, share, seed):
    """Flat indices of a share of the present entries of X, sorted"""
    where = np.flatnonzero(np.isfinite(X).reshape(-1))
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(where, size=max(1, int(round(share * where.size))), replace=False)).astype(np.int64)


def center(X):
    """(mean over the present entries per column, anomaly plane with 0 at the missing entries, mask of the missing, scale)"""
    X = np.asarray(X, dtype=np.float64)
    present = np.isfinite(X)
    mean = np.where(present, X, 0.0).sum(axis=0) / present.sum(axis=0)
    A = np.where(present, X - mean, 0.0)
    scale = np.sqrt(np.sum(A[present] ** 2) / present.sum())
    return mean, A, ~present, scale


def truncation(A, k, route):
    """(rank-k truncation of A, the k leading eigenvalues of A A^T) by either route"""
    if route == "gram":
        lam, Z = np.linalg.eigh(A @ A.T)
        Z = Z[:, ::-1][:, :k].T
        return Z.T @ (Z @ A), lam[::-1][:k]
    U, s, Vt = np.linalg.svd(A, full_matrices=False)
    return (U[:, :k] * s[:k]) @ Vt[:k], s[:k] ** 2


def dineof(X, k, max_iter, tol, cv_idx=None, route="gram"):
    """The restatement in float64 (of a float32 field too).  Returns 'field' (float64), 'history', 'iterations', 'converged',
    'cv_rms' (None without cv_idx) and 'lam', the k leading eigenvalues of the last iterate's Gram matrix."""
    X = np.asarray(X, dtype=np.float64)
    mean, A, mask, scale = center(X)
    saved = None
    if cv_idx is not None:
        saved = A.reshape(-1)[cv_idx].copy()
        A.reshape(-1)[cv_idx] = 0.0
        mask = mask.copy()
        mask.reshape(-1)[cv_idx] = True
    n_masked = int(mask.sum())
    history, lam = [], None
    for _ in range(max_iter):
        R, lam = truncation(A, k, route)
        d = np.sqrt(np.sum((R[mask] - A[mask]) ** 2) / n_masked) / scale
        A[mask] = R[mask]
        history.append(float(d))
        if d < tol:
            break
    cv_rms = None if saved is None else float(np.sqrt(np.mean((A.reshape(-1)[cv_idx] - saved) ** 2)))
    field = np.where(np.isfinite(X), X, A + mean)
    return {"field": field, "history": np.array(history), "iterations": len(history), "converged": bool(history[-1] < tol),
            "cv_rms": cv_rms, "lam": lam}


def recovery_ratio(field, X, truth):
    """RMS error of `field` at the removed entries of X against the truth, over that of filling with the column means"""
    gone = ~np.isfinite(X)
    mean = center(X)[0]
    by_mean = np.broadcast_to(mean, X.shape)[gone] - truth[gone]
    return float(np.sqrt(np.mean((np.asarray(field, dtype=np.float64)[gone] - truth[gone]) ** 2)) / np.sqrt(np.mean(by_mean ** 2)))


_cache = {}


def reference(case, dtype=np.float64, iterations=STATE_ITERATIONS, route="gram", cv=False):
    """The restatement after `iterations` iterations (tol = 0) on a case's field of `dtype`, computed once per process"""
    key = (case, np.dtype(dtype).name, iterations, route, cv)
    if key not in _cache:
        T, N, r, k, frac = case
        X = case_field(T, N, r, frac, dtype)[0]
        idx = cv_indices(X, CV_SHARE, CV_SEED) if cv else None
        out = dineof(X, k, iterations, 0.0, cv_idx=idx, route=route)
        out["field"].setflags(write=False)
        _cache[key] = out
    return _cache[key]


def route_delta(case, dtype=np.float64, cv=False, iterations=STATE_ITERATIONS):
    """delta of the state-for-state comparison: the larger of the difference between the two float64 routes on the case and
    2^-52 max|X|"""
    a = reference(case, dtype, iterations, route="gram", cv=cv)["field"]
    b = reference(case, dtype, iterations, route="svd", cv=cv)["field"]
    return max(float(np.max(np.abs(a - b))), 2.0 ** -52 * float(np.max(np.abs(a))))
