"""CPU check of the fourth-moment form of the Varimax gradient (rotate.h, rot_moment_kernel / varimax_moment_kernel).

With Z = A R and M'_uv = sum_n Q_nu Q_nv over the unordered pairs u = (l <= m), Q_nu = a_nl a_nm:
    G = sum_k R_kj (M' S)_(ik),j - (gamma / N) (A^T A R) diag(c),   S_uj = w_u R_lj R_mj,
which is A^T (Z^3 - gamma / N Z diag(c)) of rotation.py:56-57.  The test restates the kernels' index arithmetic (pair order,
upper-triangle 4 x 4 block layout of M', the per-thread M' slices) and runs the whole loop against oracle.ref_numpy.varimax.
"""
import numpy as np
import pytest

from oracle import ref_numpy as O


def _pairs(p):
    return [(l, m) for l in range(p) for m in range(l, p)]


def _moment_blocks(A):
    """M' in the layout of rot_moment_kernel: upper-triangle 4 x 4 blocks, 16 entries each."""
    n, p = A.shape
    pr = _pairs(p)
    P = len(pr)
    nb = (P + 3) // 4
    Q = np.zeros((n, 4 * nb))
    for u, (l, m) in enumerate(pr):
        Q[:, u] = A[:, l] * A[:, m]
    out = []
    for bu in range(nb):
        for bv in range(bu, nb):
            out.append((Q[:, 4 * bu:4 * bu + 4].T @ Q[:, 4 * bv:4 * bv + 4]).ravel())
    return np.concatenate(out), nb


def _moment_at(mom, nb, u, v):
    if u // 4 > v // 4:
        u, v = v, u
    bu, bv = u // 4, v // 4
    return mom[(bu * nb - bu * (bu - 1) // 2 + bv - bu) * 16 + (u % 4) * 4 + v % 4]


def _gradient(mom, nb, A0, R, c, n, gamma):
    p = R.shape[0]
    pr = _pairs(p)
    P = len(pr)
    nch = min(256 // P, 8)
    ck = -(-P // nch)
    S = np.zeros((nch * ck, p))
    for u, (l, m) in enumerate(pr):
        S[u] = (1.0 if l == m else 2.0) * R[l] * R[m]
    Yp = np.zeros((nch, P, p))
    for ch in range(nch):
        for u in range(P):
            M = np.array([_moment_at(mom, nb, u, ch * ck + vv) if ch * ck + vv < P else 0.0 for vv in range(ck)])
            Yp[ch, u] = M @ S[ch * ck:ch * ck + ck]
    Y = Yp.sum(axis=0)
    pidx = np.zeros((p, p), dtype=int)
    for u, (l, m) in enumerate(pr):
        pidx[l, m] = pidx[m, l] = u
    G1 = np.array([[R[:, j] @ Y[pidx[i], j] for j in range(p)] for i in range(p)])
    return G1 - (gamma / n) * (A0 @ R) * c[None, :]


def _loadings(n, p, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, p)) @ np.diag(0.6 ** np.arange(p)) + 0.1 * rng.standard_normal((n, p))
    return A / np.linalg.norm(A, axis=1)[:, None]


@pytest.mark.parametrize("p", [2, 3, 5, 8, 10, 11, 12])
def test_moment_gradient_equals_direct_sum(p):
    n = 300
    A = _loadings(n, p, 100 + p)
    R, _ = np.linalg.qr(np.random.default_rng(p).standard_normal((p, p)))
    mom, nb = _moment_blocks(A)
    A0 = A.T @ A
    Z = A @ R
    c = np.sum(Z * Z, axis=0)
    for gamma in (1.0, 0.0, 0.5):
        direct = A.T @ (Z ** 3 - (gamma / n) * Z * c[None, :])
        got = _gradient(mom, nb, A0, R, c, n, gamma)
        assert np.max(np.abs(got - direct)) < 1e-12 * np.max(np.abs(direct))


@pytest.mark.parametrize("p", [3, 10])
def test_moment_loop_matches_oracle(p):
    """The loop on M' alone (the SVD polar factor of the reference) stops at the same iteration with the same R."""
    A = _loadings(2000, p, 7 + p)
    n = A.shape[0]
    _, R_ref, it_ref = O.varimax(A)
    mom, nb = _moment_blocks(A)
    A0 = A.T @ A
    R = np.eye(p)
    d = 0.0
    for it in range(1000):
        c = np.diag(R.T @ A0 @ R)
        u, s, vh = np.linalg.svd(_gradient(mom, nb, A0, R, c, n, 1.0))
        R = u @ vh
        d, d_old = np.sum(s), d
        if abs(d - d_old) / d < 1e-8:
            break
    assert it + 1 == it_ref
    assert np.max(np.abs(R - R_ref)) < 1e-10
