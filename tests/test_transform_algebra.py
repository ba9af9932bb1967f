"""The small mixes of the device transforms (xmca_amd/array.py `_predict_mix`, `_rotated_mix`, `_reconstruct_coefficients`) against
the reference's formulas on random matrices: predict's `(x @ V[:, :n_rot] / sqrt(s)) @ R^-H` then `[:, var_idx][:, :n]`
(xmca/array.py:1299-1428) and the reconstruction's `(U_eigen @ V_rot^H).real` (:1263-1292).  No GPU."""
import numpy as np
import pytest

from xmca_amd.array import _predict_mix, _reconstruct_coefficients, _rotated_mix

TOL = 1e-13


def _case(rng, cplx, N=37, T=23, rank=9):
    def draw(*shape):
        a = rng.standard_normal(shape)
        return a + 1j * rng.standard_normal(shape) if cplx else a
    V, _ = np.linalg.qr(draw(N, rank))
    s = np.sort(rng.uniform(0.5, 4.0, rank))[::-1]
    x = draw(T, N).real if cplx else draw(T, N)          # new data is real; a complex model's PCs of it are not Hilbert-transformed
    return V, s, x


def _promax_like(rng, p, cplx):
    """a non-orthogonal, well-conditioned p x p rotation (what Promax leaves)"""
    R = np.eye(p) + 0.3 * rng.standard_normal((p, p))
    if cplx:
        R = R + 0.2j * rng.standard_normal((p, p))
    return R


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("n", [None, 1, 4])
def test_predict_mix_matches_reference_formula(cplx, rotated, n):
    rng = np.random.default_rng(3 + 2 * cplx + rotated)
    V, s, x = _case(rng, cplx)
    if rotated:
        n_rot = 6
        R = _promax_like(rng, n_rot, cplx)
        R_it = np.linalg.pinv(R).conjugate().T
        var_idx = rng.permutation(n_rot)
    else:
        n_rot = len(s)
        R_it = np.eye(n_rot)
        var_idx = np.argsort(s)[::-1]
    nn = n_rot if n is None else n
    ref = ((x @ V[:, :n_rot] / np.sqrt(s[:n_rot])) @ R_it)[:, var_idx][:, :nn]
    W = _predict_mix(s, R_it, var_idx, n_rot, nn)
    m = W.shape[0]
    assert W.shape[1] == ref.shape[1] and 1 <= m <= n_rot
    got = (x @ V[:, :m]) @ W
    assert np.max(np.abs(got - ref)) <= TOL * np.max(np.abs(ref))
    if not rotated:
        assert m == nn                  # unrotated: only the selected modes' vectors enter the product


def test_predict_mix_keeps_permuted_modes_and_nan_rows():
    var_idx = np.array([0, 2, 1, 3])                     # tied modes swapped by argsort
    W = _predict_mix(np.array([3.0, 2.0, 2.0, 1.0]), np.eye(4), var_idx, 4, 2)
    assert W.shape == (3, 2)                             # column 2 selects mode 2: three vectors needed
    W = _predict_mix(np.array([3.0, 2.0, 2.0, 0.0]), np.eye(4), var_idx, 4, 2)
    assert W.shape == (4, 2) and np.isnan(W[3]).all()    # a null mode: 0 / 0 reaches the product as the reference's does


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("mode", [None, 3, slice(2, 6)])
@pytest.mark.parametrize("rotated", [False, True])
def test_reconstruct_coefficients_match_reference_formula(cplx, mode, rotated):
    rng = np.random.default_rng(11 + 2 * cplx + rotated)
    V, s, _ = _case(rng, cplx)
    T, rank = 23, len(s)
    U = rng.standard_normal((T, rank)) + (1j * rng.standard_normal((T, rank)) if cplx else 0)
    # 0-based selection as MCA._get_slice makes it, and the largest mode `_max_mode` asks for
    if mode is None:
        keep, max_mode = slice(0, rank), rank
    elif isinstance(mode, slice):
        keep, max_mode = slice(mode.start - 1, mode.stop), mode.stop
    else:
        keep, max_mode = slice(0, mode), mode
    if rotated:
        max_mode = 6
        R = _promax_like(rng, max_mode, cplx)
        norm = rng.uniform(0.5, 2.0, max_mode)
        var_idx = rng.permutation(max_mode)
        A = _rotated_mix(s[:max_mode], R, norm, var_idx, keep)
        V_rot = (V[:, :max_mode] * np.sqrt(s[:max_mode]) @ R / norm)[:, var_idx][:, keep]      # `_get_V`
    else:
        A = np.eye(max_mode)[:, keep]
        V_rot = V[:, :max_mode][:, keep]
    P = U[:, :V_rot.shape[1]]                                                               # pcs(mode, 'eigen')
    ref = (P @ V_rot.conj().T).real
    B = _reconstruct_coefficients(P, A)
    assert B.shape == (T, max_mode)
    got = (B @ V[:, :max_mode].conj().T).real
    assert np.max(np.abs(got - ref)) <= TOL * np.max(np.abs(ref))
