"""Varimax of real loadings with p <= 12 modes on the fourth-moment route (rotate.h rot_moment_kernel +
varimax_moment_kernel), against the numpy restatement of rotation.py: same iteration count, R and B within the tolerance of
test_gpu_rotation.py, on grids shorter than one 64-point tile, not a multiple of 64, C2-sized and longer than 65 536 points.
p = 13 and 16 stay on the persistent kernel and are checked the same way."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-7


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _loadings(n, p, seed):
    rng = np.random.default_rng(seed)
    L = 0.15 * rng.standard_normal((n, p))
    w = max(n // p, 1)
    for j in range(p):
        seg = L[j * w:(j + 1) * w, j]
        seg += np.hanning(len(seg)) * (3.0 - 0.05 * j)
    Q, _ = np.linalg.qr(rng.standard_normal((p, p)))
    return L @ Q


@pytest.mark.parametrize("p", [2, 3, 8, 10, 12])
@pytest.mark.parametrize("n", [50, 1000, 10000, 70000])
def test_moment_route_matches_oracle(hip, n, p):
    from oracle import ref_numpy as O
    A = _loadings(n, p, 1000 * p + n % 997)
    B_ref, R_ref, n_iter = O.varimax(A)
    out = hip.rotate_loadings(A, n_left=n // 2, varimax_only=True, want_B=True)
    assert out["n_iter"] == n_iter
    assert _rel(out["R"], R_ref) < TOL
    assert _rel(out["B"], B_ref) < TOL


@pytest.mark.parametrize("p", [13, 16])
def test_more_modes_keep_the_persistent_kernel(hip, p):
    from oracle import ref_numpy as O
    A = _loadings(3000, p, 77 + p)
    B_ref, R_ref, n_iter = O.varimax(A)
    out = hip.rotate_loadings(A, n_left=1500, varimax_only=True, want_B=True)
    assert out["n_iter"] == n_iter
    assert _rel(out["R"], R_ref) < TOL
    assert _rel(out["B"], B_ref) < TOL


def test_quartimax_matches_oracle(hip):
    from oracle import ref_numpy as O
    A = _loadings(5000, 10, 5)
    B_ref, R_ref, n_iter = O.varimax(A, gamma=0.0)
    out = hip.rotate_loadings(A, n_left=2500, varimax_only=True, want_B=True, gamma=0.0)
    assert out["n_iter"] == n_iter
    assert _rel(out["R"], R_ref) < TOL
    assert _rel(out["B"], B_ref) < TOL


def test_two_calls_give_the_same_bits(hip):
    A = _loadings(70000, 10, 9)
    a = hip.rotate_loadings(A, n_left=35000, varimax_only=True, want_B=True)
    b = hip.rotate_loadings(A, n_left=35000, varimax_only=True, want_B=True)
    assert a["n_iter"] == b["n_iter"]
    assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["B"], b["B"])


def test_too_few_iterations_raise(hip):
    from oracle import ref_numpy as O
    A = _loadings(2000, 10, 11)
    _, _, n_iter = O.varimax(A)
    assert n_iter > 3
    with pytest.raises(RuntimeError):
        hip.rotate_loadings(A, n_left=1000, varimax_only=True, max_iter=n_iter - 2)
    assert hip.last_iters == n_iter - 2


def test_zero_row_is_linalg_error(hip):
    A = _loadings(2000, 10, 12)
    A[7] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        hip.rotate_loadings(A, n_left=1000)
