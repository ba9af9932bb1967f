"""The numpy truth of `MCA.extended_eofs` and the cases shared by tests/test_extended_eofs_host.py and
tests/test_gpu_extended_eofs.py.

Definition.  X: the T x N field as solve() sees it; M = embedding, T' = T - (M - 1) tau, X_j = X[j tau : j tau + T', :];
Y = [X_0 | ... | X_{M-1}] with every column centred over its T' rows; Y_c = U S V^H.  singular_values = S^2 / (T' - 1), PCs =
U sqrt(T' - 1), patterns = the unit-norm rows of V^H as (M, N, modes).  The truth is the SVD of the explicit Y_c in float64.
`gram_route` restates what the device does - lag-summed Gram matrix, double centring, eigenvectors, back-projection of the
UNCENTRED windows - and `gram_route(center=False)` the mistake of leaving the centring out."""
import numpy as np

# (name, T, N, M, tau, n_modes, seed): the seeds are chosen so that every case meets MIN_RELGAP (test_extended_eofs_host.py)
E2E_CASES = [
    ("40x23_M4_t1", 40, 23, 4, 1, 3, 9),
    ("40x23_M4_t3", 40, 23, 4, 3, 3, 2),
    ("37x130_M5_t2", 37, 130, 5, 2, 3, 7),
    ("33x257_M2_t16", 33, 257, 2, 16, 3, 8),
    ("130x65_M3_t7", 130, 65, 3, 7, 3, 10),
]
# ... and two more for the identity on the host: a narrow field with a long window, and the largest shape of the derivation
IDENTITY_CASES = E2E_CASES + [
    ("64x9_M6_t1", 64, 9, 6, 1, 3, 8),
    ("200x300_M12_t1", 200, 300, 12, 1, 3, 1),
]
# T' = 799 is past the order from which the eigensolver reduces to tridiagonal form and forms the leading vectors only
LARGE_CASE = ("800x900_M2_t1", 800, 900, 2, 1, 3, 0)
# the 3-d field with masked grid points: (name, T, spatial shape, masked flat indices, M, tau, n_modes, seed)
MASKED_CASE = ("40x5x6_masked_M3_t2", 40, (5, 6), (0, 7, 8, 19, 29), 3, 2, 3, 2)
MIN_RELGAP = 0.02


def case_field(T, N, seed=0):
    """A T x N float64 field: a geometric spectrum 0.8^i between orthonormal factors, plus a linear trend of the leading mode's
    amplitude along a random unit pattern, centred over T.  The trend makes the window means differ from lag to lag."""
    rng = np.random.default_rng([seed, T, N])
    r = min(T, N)
    U = np.linalg.qr(rng.standard_normal((T, r)))[0]
    V = np.linalg.qr(rng.standard_normal((N, r)))[0]
    s = 0.8 ** np.arange(r)
    t = np.linspace(-1.0, 1.0, T)
    w = rng.standard_normal(N)
    X = (U * s) @ V.T + s[0] * np.outer(t / np.linalg.norm(t), w / np.linalg.norm(w))
    return X - X.mean(axis=0)


def embed(X, M, tau):
    """Y = [X_0 | ... | X_{M-1}], (T', M N), uncentred"""
    Tp = X.shape[0] - (M - 1) * tau
    return np.concatenate([X[j * tau:j * tau + Tp] for j in range(M)], axis=1)


def _result(lam, u, vt, M, k):
    """lam: all eigenvalues (descending); u: T' x k unit vectors; vt: k x (M N) unit-norm patterns"""
    Tp = u.shape[0]
    return {"lam": lam,
            "singular_values": lam[:k] / (Tp - 1),
            "explained_variance": lam[:k] / np.maximum(lam, 0.0).sum() * 100.0,
            "pcs": u * np.sqrt(Tp - 1),
            "eofs": vt.reshape(k, M, -1).transpose(1, 2, 0)}


def svd_truth(X, M, tau, k):
    """The definition: SVD of the explicitly embedded, column-centred matrix, in float64"""
    Y = embed(np.asarray(X, dtype=np.float64), M, tau)
    Yc = Y - Y.mean(axis=0)
    u, s, vt = np.linalg.svd(Yc, full_matrices=False)
    lam = np.zeros(Y.shape[0])
    lam[:len(s)] = s ** 2
    return _result(lam, u[:, :k], vt[:k], M, k)


def lag_sum(G, M, tau):
    """K[t, s] = sum_j G[t + j tau, s + j tau], the terms added in the order j = 0 .. M-1"""
    Tp = G.shape[0] - (M - 1) * tau
    K = G[:Tp, :Tp].copy()
    for j in range(1, M):
        K += G[j * tau:j * tau + Tp, j * tau:j * tau + Tp]
    return K


def double_center(K):
    """H K H with H = I - 1 1^T / n"""
    r = K.mean(axis=0)
    return K - r[:, None] - r[None, :] + r.mean()


def gram_route(X, M, tau, k, center=True):
    """The device's route in numpy; center=False leaves H K H out"""
    X = np.asarray(X, dtype=np.float64)
    K = lag_sum(X @ X.T, M, tau)
    if center:
        K = double_center(K)
    lam, Z = np.linalg.eigh(K)
    lam, Z = lam[::-1], Z[:, ::-1]
    u = Z[:, :k]
    vt = (embed(X, M, tau).T @ u / np.sqrt(lam[:k])).T
    return _result(lam, u, vt, M, k)


def relgaps(lam, k):
    """(lam_i - lam_{i+1}) / lam_i behind each of the k leading eigenvalues"""
    lam = np.asarray(lam)
    return (lam[:k] - lam[1:k + 1]) / lam[:k]


def aligned(res, ref):
    """(pcs, eofs) of `res` with one sign per mode so that the patterns point along those of `ref`"""
    k = ref["pcs"].shape[1]
    a, b = np.nan_to_num(res["eofs"]).reshape(-1, k), np.nan_to_num(ref["eofs"]).reshape(-1, k)
    sign = np.where(np.sum(a * b, axis=0) < 0, -1.0, 1.0)
    return res["pcs"] * sign, res["eofs"] * sign


def errors(res, ref):
    """worst absolute error of aligned patterns and PCs, worst relative error of singular values and explained variance"""
    pcs, eofs = aligned(res, ref)
    return {"eofs": float(np.nanmax(np.abs(eofs - ref["eofs"]))),
            "pcs": float(np.max(np.abs(pcs - ref["pcs"]))),
            "singular_values": float(np.max(np.abs(res["singular_values"] / ref["singular_values"] - 1))),
            "explained_variance": float(np.max(np.abs(res["explained_variance"] / ref["explained_variance"] - 1)))}


def masked_field(T, shape, masked, seed=0):
    """(field of shape (T,) + shape with NaN at the masked points, its kept columns T x N' as solve() sees them)"""
    n = int(np.prod(shape))
    keep = np.ones(n, dtype=bool)
    keep[list(masked)] = False
    X = case_field(T, int(keep.sum()), seed)
    full = np.full((T, n), np.nan)
    full[:, keep] = X
    return full.reshape((T,) + tuple(shape)), X, keep
