"""Kernel-level parity (through the C ABI) against numpy: MFMA GEMM, block-Jacobi eigensolver,
Philox generator.  Bars: GEMM f64 1e-13 / f32-wide 2e-6 relative to |A||B|; eigenvalues 1e-11 * lam_max."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-13), (np.float32, 2e-6)])
@pytest.mark.parametrize("a_kfast,b_nfast", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("M,N,K", [(37, 53, 29), (128, 128, 64), (200, 130, 517), (1, 300, 70)])
def test_gemm_orientations(hip, dtype, tol, a_kfast, b_nfast, M, N, K):
    rng = np.random.default_rng(M * 1000 + N + K)
    A = rng.standard_normal((M, K)).astype(dtype)
    B = rng.standard_normal((K, N)).astype(dtype)
    As = A if a_kfast else np.ascontiguousarray(A.T)
    Bs = B if b_nfast else np.ascontiguousarray(B.T)
    C = hip.gemm(As, Bs, a_kfast=a_kfast, b_nfast=b_nfast, alpha=0.5)
    ref = 0.5 * (A.astype(np.float64) @ B.astype(np.float64))
    scale = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
    assert np.max(np.abs(C - ref) / scale.max()) < tol


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-13), (np.float32, 2e-6)])
@pytest.mark.parametrize("T,N,splits", [(300, 1000, 0), (300, 5000, 4), (129, 777, 3), (64, 40000, 0)])
def test_gram_upper_mirror_splitk(hip, dtype, tol, T, N, splits):
    rng = np.random.default_rng(T + N)
    X = rng.standard_normal((T, N)).astype(dtype)
    G = hip.gemm(X, X, a_kfast=True, b_nfast=False, upper_only=True, mirror=1, splits=splits)
    ref = X.astype(np.float64) @ X.astype(np.float64).T
    assert _rel(G, ref) < tol
    assert np.array_equal(G, G.T)
    # antisymmetric mirror: Xi Xr^T - Xr Xi^T pattern is tested through the complex solve; here mirror=-1 only
    Y = rng.standard_normal((T, N)).astype(dtype)
    H = hip.gemm(X, Y, a_kfast=True, b_nfast=False, upper_only=True, mirror=-1, splits=splits)
    ref2 = X.astype(np.float64) @ Y.astype(np.float64).T
    iu = np.triu_indices(T, 1)
    bm = iu[0] // 128 != iu[1] // 128         # strictly upper BLOCK tiles are mirrored with the sign
    assert _rel(H[iu], ref2[iu]) < tol
    assert np.allclose(H.T[iu][bm], -H[iu][bm], rtol=0, atol=0)


def test_gemm_f32_wide_accumulation(hip):
    """long contraction with a large common offset: plain f32 accumulation would lose ~1e-4; the f64 flush keeps 1e-6."""
    rng = np.random.default_rng(5)
    K = 200_000
    A = (rng.standard_normal((16, K)) + 3.0).astype(np.float32)
    B = (rng.standard_normal((K, 16)) + 3.0).astype(np.float32)
    C = hip.gemm(A, B, splits=1)
    ref = A.astype(np.float64) @ B.astype(np.float64)
    assert _rel(C, ref) < 5e-7


def _herm(rng, n, N, cplx, centered=True):
    X = (rng.standard_normal((n, 6)) * 10 * 0.7 ** np.arange(6)) @ rng.standard_normal((6, N)) + rng.standard_normal((n, N))
    if cplx:
        X = X + 1j * ((rng.standard_normal((n, 6)) * 5 * 0.7 ** np.arange(6)) @ rng.standard_normal((6, N)) + rng.standard_normal((n, N)))
    if centered:
        X = X - X.mean(axis=0)
    return X @ X.conj().T


@pytest.mark.parametrize("n,cplx", [(5, False), (32, False), (33, False), (64, False), (100, False), (257, False), (600, False),
                                     (7, True), (32, True), (50, True), (130, True), (300, True)])
def test_eigh_matches_lapack(hip, n, cplx):
    rng = np.random.default_rng(n)
    G = _herm(rng, n, 3 * n + 10, cplx)
    lam, U = hip.eigh(G)
    ref = np.linalg.eigvalsh(G)[::-1]
    # measured on MI355X: <= 1.2e-12 * lam_max at n = 600 (accumulated rounding of ~200 two-sided block updates)
    assert np.max(np.abs(lam - ref)) < 1e-11 * ref[0], hip.last_eigh_info
    # reconstruction + orthonormality
    assert np.max(np.abs(U.conj().T @ U - np.eye(n))) < 1e-11
    R = U.conj().T @ G @ U
    assert np.max(np.abs(R - np.diag(lam))) < 1e-10 * ref[0]
    assert hip.last_eigh_info["sweeps"] <= 25


@pytest.mark.parametrize("n,cplx,tile,slots", [(20, False, 32, 1), (100, False, 64, 2), (150, False, 64, 3), (128, False, 64, 2),
                                                (50, True, 32, 2), (130, True, 32, 5)])
def test_eigh_values_only_takes_the_jacobi_sweeps(hip, n, cplx, tile, slots):
    """Below 192 rows `vectors=False` stays on the block Jacobi sweeps, launched without eigenvector planes: one tile,
    the unfused pair (2 slots; n = 128 has no padding, so no Frobenius pass) and the fused rounds (3 and 5 slots)."""
    rng = np.random.default_rng(n)
    G = _herm(rng, n, 3 * n + 10, cplx)
    lam, U = hip.eigh(G, vectors=False)
    assert U is None
    info = hip.last_eigh_info
    assert info["tridiag"] == 0 and info["tile"] == tile and info["slots"] == slots, info
    assert np.all(np.diff(lam) <= 0)
    ref = np.linalg.eigvalsh(G)[::-1]
    err = float(np.max(np.abs(lam - ref)))
    print("values-only Jacobi n=%d cplx=%d: max |lam - eigvalsh| / lam_max = %.3e" % (n, cplx, err / ref[0]))
    assert err < 1e-11 * ref[0], info


def test_eigh_rank_deficient_complex(hip):
    """analytic signals have rank T/2: the null space must not stall the sweeps."""
    from scipy.signal import hilbert
    rng = np.random.default_rng(3)
    T = 200
    X = hilbert(rng.standard_normal((T, 700)), axis=0)
    X = X - X.mean(axis=0)
    G = X @ X.conj().T
    lam, U = hip.eigh(G)
    ref = np.linalg.eigvalsh(G)[::-1]
    assert np.max(np.abs(lam - ref)) < 1e-11 * ref[0]
    assert hip.last_eigh_info["sweeps"] <= 25


@pytest.mark.parametrize("n,cplx,decades", [(700, False, 10), (500, True, 8), (1000, False, 6)])
def test_eigh_graded_spectrum_takes_the_cholesky_lr_step(hip, n, cplx, decades, monkeypatch):
    """Eigenvalues spread evenly over many decades: the solver inserts one Cholesky LR step (jacobi.h) and
    must still return orthonormal vectors - also for the small eigenvalues, which the back-transformation R^H v
    only gives if the sweeps converge relative to sqrt(m_ii m_jj)."""
    rng = np.random.default_rng(n)
    Q = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx else 0)
    Q, _ = np.linalg.qr(Q)
    lam_true = np.logspace(0, -decades, n)
    G = (Q * lam_true) @ Q.conj().T
    G = (G + G.conj().T) / 2
    monkeypatch.setenv("XMCA_TRIDIAG", "0")            # (the Jacobi solver; the tridiagonal route: tests/test_gpu_tridiag.py)
    lam, U = hip.eigh(G)
    assert hip.last_eigh_info["lr_step"] == 1, hip.last_eigh_info
    ref = np.linalg.eigvalsh(G)[::-1]
    assert np.max(np.abs(lam - ref)) < 1e-11 * ref[0]
    assert np.max(np.abs(U.conj().T @ U - np.eye(n))) < 1e-10
    # every eigenpair above the shift of the factorisation (1e-13 lam_max), judged at its own scale
    big = lam_true > 1e-9
    res = np.linalg.norm(G @ U[:, big] - U[:, big] * lam[big], axis=0)
    assert np.max(res / ref[0]) < 1e-11
    # the plain path agrees on the vectors of well separated (leading) eigenvalues up to phase
    ov = np.abs(np.sum(U[:, :5].conj() * Q[:, :5], axis=0))
    assert np.all(np.abs(ov - 1) < 1e-8)


def test_eigh_flat_spectrum_stays_on_the_plain_path(hip):
    rng = np.random.default_rng(5)
    G = _herm(rng, 600, 2000, False)
    hip.eigh(G)
    assert hip.last_eigh_info["lr_step"] == 0


def test_eigh_indefinite_graded_matrix(hip):
    """Not a Gram matrix: the LR step must be skipped (or fail cleanly) and the plain sweeps finish the job."""
    rng = np.random.default_rng(9)
    n = 400
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam_true = np.logspace(0, -9, n) * np.where(np.arange(n) % 2, 1.0, -1.0)
    G = (Q * lam_true) @ Q.T
    G = (G + G.T) / 2
    lam, U = hip.eigh(G)
    ref = np.linalg.eigvalsh(G)[::-1]
    assert np.max(np.abs(lam - ref)) < 1e-11 * np.abs(ref).max()
    assert np.max(np.abs(U.T @ U - np.eye(n))) < 1e-10




@pytest.mark.parametrize("seed", [0, 1, 2])
def test_eigh_randomised_shapes_and_spectra(hip, seed):
    """sizes around the tile boundaries, real / complex, flat / graded / rank-deficient / indefinite / spiked spectra and
    scales from 1e-6 to 1e6 (the generator of scripts/eigh_stress.py, fewer trials)."""
    rng = np.random.default_rng(seed)
    sizes = [1, 2, 31, 33, 63, 64, 65, 127, 129, 191, 193, 257, 320, 385, 500]
    for trial in range(14):
        n = int(rng.choice(sizes))
        cplx = bool(rng.integers(2))
        kind = rng.choice(["flat", "graded", "deficient", "indefinite", "spiked"])
        Q = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx else 0)
        Q, _ = np.linalg.qr(Q)
        if kind == "flat":
            lam = rng.uniform(0.1, 1.0, n)
        elif kind == "graded":
            lam = np.logspace(0, -rng.uniform(3, 13), n)
        elif kind == "deficient":
            lam = np.where(np.arange(n) < max(1, n // 3), rng.uniform(0.1, 1, n), 0.0)
        elif kind == "indefinite":
            lam = rng.standard_normal(n) * np.logspace(0, -rng.uniform(0, 8), n)
        else:
            lam = np.concatenate([rng.uniform(1e4, 1e6, min(5, n)), rng.uniform(0.5, 1.0, max(n - 5, 0))])[:n]
        A = (Q * lam) @ Q.conj().T
        A = (A + A.conj().T) / 2 * 10.0 ** rng.integers(-6, 7)
        w, U = hip.eigh(A)
        ref = np.linalg.eigvalsh(A)[::-1]
        scale = np.abs(ref).max()
        ctx = (n, cplx, str(kind), hip.last_eigh_info)
        assert np.all(np.diff(w) <= 0), ctx
        assert np.max(np.abs(w - ref)) < 2e-11 * scale, ctx
        assert np.max(np.abs(U.conj().T @ U - np.eye(n))) < 2e-10, ctx
        assert np.max(np.abs(A @ U - U * w)) < 2e-10 * scale, ctx


def test_eigh_nan_is_an_error(hip):
    G = np.eye(40)
    G[3, 5] = G[5, 3] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        hip.eigh(G)


def test_philox_normals(hip):
    n = 2_000_001
    x = hip.surrogate(n, seed=42, run=3, side=1)
    assert abs(x.mean()) < 4 / np.sqrt(n)
    assert abs(x.std() - 1) < 4 / np.sqrt(2 * n)
    assert abs(np.mean(x ** 3)) < 0.02 and abs(np.mean(x ** 4) - 3) < 0.05
    y = hip.surrogate(n, seed=42, run=3, side=1)
    assert np.array_equal(x, y)                               # counter based: bitwise repeatable
    z = hip.surrogate(n, seed=42, run=4, side=1)
    assert abs(np.corrcoef(x, z)[0, 1]) < 5 / np.sqrt(n)      # independent across runs
    w = hip.surrogate(1000, seed=42, run=3, side=1)
    assert np.array_equal(w, x[:1000])                        # prefix property (length independent)


# ----------------------------------------------------------------------------------------------
# blocked Cholesky (values-only two-field solves)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cplx", [(1, False), (5, False), (64, False), (65, True), (200, True), (333, False), (700, True)])
def test_cholesky_matches_numpy(hip, n, cplx):
    rng = np.random.default_rng(100 + n)
    X = rng.standard_normal((n, 2 * n + 3))
    if cplx:
        X = X + 1j * rng.standard_normal(X.shape)
    A = X @ X.conj().T
    R, ok = hip.cholesky(A)
    assert ok
    ref = np.linalg.cholesky(A).conj().T                 # upper factor
    assert np.allclose(np.tril(R, -1), 0.0)
    assert np.max(np.abs(R - ref)) / np.max(np.abs(ref)) < 1e-11
    assert np.max(np.abs(R.conj().T @ R - A)) / np.max(np.abs(A)) < 1e-13


def test_cholesky_semidefinite_needs_the_shift(hip):
    rng = np.random.default_rng(7)
    X = rng.standard_normal((90, 300))
    X -= X.mean(axis=0)                                   # centered in time: the Gram matrix is singular
    A = X @ X.T
    R, ok = hip.cholesky(A, rel_shift=1e-13)
    assert ok
    assert np.max(np.abs(R.T @ R - A)) / np.max(np.abs(A)) < 1e-12
    _, ok = hip.cholesky(-A)                              # not positive: reported, no exception
    assert not ok


@pytest.mark.parametrize("n", [2, 3, 4, 5, 7, 8, 12, 60, 150, 343, 1000, 2501 - 1, 4200, 5000, 5120])
def test_fft_matches_numpy(hip, n):
    """csrc/fft.h (Stockham, radices 4/2/3/5/7, one workgroup per transform in LDS) against numpy.fft in both directions,
    complex and real input; the analytic-signal path uses it for the Fourier reduction of the Gram matrix (T = 5000: 2^3 5^4)."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal((5, n)) + 1j * rng.standard_normal((5, n))
    scale = np.sqrt(n)
    assert np.max(np.abs(hip.fft(x, -1) - np.fft.fft(x, axis=1))) < 1e-13 * scale * np.abs(x).max() * np.log2(n + 1)
    assert np.max(np.abs(hip.fft(x, +1) - np.fft.ifft(x, axis=1) * n)) < 1e-13 * scale * np.abs(x).max() * np.log2(n + 1)
    assert np.max(np.abs(hip.fft(x.real, -1) - np.fft.fft(x.real, axis=1))) < 1e-13 * scale * np.log2(n + 1) * 5


def test_fft_refuses_lengths_it_cannot_factor(hip):
    for n in (11, 2 * 31, 2920, 5121 * 2):
        with pytest.raises(Exception):
            hip.fft(np.ones((1, n)))
