"""Inputs and float64 / extended-precision references of the Promax edge tests (tests/test_gpu_promax_edges.py,
scripts/promax_tail_accuracy.py).  Test infrastructure only, numpy only.

* `CASES`: (N, p, complex, power, n_left, seed) - the smallest shapes that reach each edge of the Promax passes of the fused
  rotation routes (tile tails, the n_left split, wide accumulation, long grids).
* `edge_loadings`: banded simple structure mixed by a random orthogonal / unitary matrix.
* `stop_margin`: the oracle's stopping ratio at the stop iteration and one before it (the iteration count is asserted for
  equality, so no case may stop on a knife edge).
* `promax_tail`: the part of `ref_numpy.promax` behind the Varimax loop, from given Varimax loadings and rotation; in float64 as
  written there, or with the N-sized sums and the column maxima in `np.longdouble` (the reference's own rounding noise is the
  difference of the two).
"""
import numpy as np

from . import ref_numpy as O

TOL_STOP = 1e-8          # Varimax stopping tolerance of every case
STOP_BELOW = 0.7         # ratio at the stop iteration <= STOP_BELOW * tol
STOP_ABOVE = 1.3         # ratio one iteration earlier >= STOP_ABOVE * tol
TAIL_FLOOR = 1e-13       # device bound of the decoupled tail = TAIL_MARGIN x reference noise, floored and capped
TAIL_CAP = 1e-10
TAIL_MARGIN = 100.0

# (N, p, complex, power, n_left, seed)
CASES = [
    (50, 13, False, 2, 17, 300),          # one partial tile, first p off the Moment route
    (63, 12, False, 2, 62, 301),          # Moment route, N = tile - 1, right block of one point
    (50, 2, False, 3, 25, 317),           # smallest p
    (64, 16, True, 3, 64, 303),           # exactly one tile, n_left = N, last p of the narrow grid
    (65, 17, False, 4, 0, 304),           # one point in the second tile, empty left block, first multi-tile Newton-Schulz p
    (200, 24, True, 2, 128, 305),         # split on a tile boundary, wide grid (p^2 * 2 >= 512)
    (1000, 33, False, 3, 129, 306),       # split one past a boundary, MAXE slot 5
    (900, 48, True, 2, 450, 320),         # largest fused complex p
    (800, 64, False, 2, 1, 64),           # largest fused real p (MAXE = 16, s4 = 15), left block of one point
    (70000, 4, False, 3, 65537, 309),     # long grid on the Moment route, nacc = 1094 > 256
    (66000, 14, True, 2, 33000, 310),     # long grid, persistent loop on 256 workgroups with the two-stage sum
    (131200, 6, False, 4, 131199, 311),   # 2050 tiles: two tiles per accumulation workgroup, split in the last tile
]


def case_id(case):
    n, p, cplx, power, n_left, _ = case
    return "%dx%d%s-pw%d-nl%d" % (n, p, "c" if cplx else "r", power, n_left)


def edge_loadings(n, p, cplx, seed):
    """Banded simple structure (band j of max(n // p, 1) points loads column j through a bump that is not zero at its ends, so
    that bands of three points still load their column), mixed by a random orthogonal / unitary matrix.  The band amplitude
    falls from 3.0 by 0.05 per column, but by no more than 1.5 over all columns: with 0.05 throughout, column 60 of a p = 64
    input has no band at all, Varimax then needs 300-900 iterations whose stopping ratio shrinks by ~8 % per iteration, and
    no seed gives the stop the margin that `stop_is_clear` asks for (40 seeds tried)."""
    rng = np.random.default_rng(seed)
    L = 0.15 * rng.standard_normal((n, p))
    w = max(n // p, 1)
    for j in range(p):
        L[j * w:(j + 1) * w, j] += np.hanning(w + 2)[1:-1] * (3.0 - min(0.05, 1.5 / p) * j)
    if cplx:
        L = L * np.exp(1j * rng.uniform(0, 2 * np.pi, (n, 1)) * 0.3) + 0.05j * rng.standard_normal((n, p))
        M = rng.standard_normal((p, p)) + 1j * rng.standard_normal((p, p))
    else:
        M = rng.standard_normal((p, p))
    Q, _ = np.linalg.qr(M)
    return L @ Q


def wide_loadings(n, p, cplx, seed):
    """the many-mode inputs of tests/test_gpu_rotation.py (its `_wide_loadings` is this function): bands of n // p points under
    np.hanning"""
    rng = np.random.default_rng(seed)
    L = 0.15 * rng.standard_normal((n, p))
    w = n // p
    for j in range(p):
        L[j * w:(j + 1) * w, j] += np.hanning(w) * (3.0 - 0.05 * j)
    if cplx:
        L = L * np.exp(1j * rng.uniform(0, 2 * np.pi, (n, 1)) * 0.3) + 0.05j * rng.standard_normal((n, p))
        M = rng.standard_normal((p, p)) + 1j * rng.standard_normal((p, p))
    else:
        M = rng.standard_normal((p, p))
    Q, _ = np.linalg.qr(M)
    return L @ Q


# more than 32 and fewer than 64 Varimax iterations (42): the per-iteration route crosses a batch of 32 launches and stops inside
# the next one.  (N, p, complex, power, n_left, seed) on `wide_loadings`
SLOW_CASE = (60, 20, True, 2, 30, 416)


def rel(a, b):
    """max-norm difference over the max of the reference (0 where both are exactly zero)"""
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def stop_margin(ratios, tol=TOL_STOP):
    """(ratio at the stop / tol, ratio one iteration earlier / tol) of the oracle's Varimax loop"""
    return ratios[-1] / tol, ratios[-2] / tol


def stop_is_clear(ratios, tol=TOL_STOP):
    at, before = stop_margin(ratios, tol)
    return at <= STOP_BELOW and before >= STOP_ABOVE


def oracle_case(case, gen=edge_loadings):
    """Input and float64 oracle of one case: dict with A, the results of ref_numpy.promax (B, R, Phi, n_iter), the block norms
    norm_left / norm_right, the stopping ratios of the loop, and the results of ref_numpy.varimax (Bv, Rv)."""
    n, p, cplx, power, n_left, seed = case
    A = gen(n, p, cplx, seed)
    ratios = []
    Bv, Rv, _ = O.varimax(A, tol=TOL_STOP, ratios=ratios)
    B, R, Phi, n_iter = O.promax(A, power, tol=TOL_STOP)
    return {"A": A, "B": B, "R": R, "Phi": Phi, "n_iter": n_iter, "ratios": ratios, "Bv": Bv, "Rv": Rv,
            "norm_left": np.linalg.norm(B[:n_left], axis=0), "norm_right": np.linalg.norm(B[n_left:], axis=0)}


def promax_tail(Bv, Rv, power, n_left, extended=False):
    """`ref_numpy.promax` behind its Varimax call, from the Varimax loadings `Bv` and rotation `Rv`, with the block norms of
    `ref_numpy.rotate`.  Returns (B, R, Phi, norm_left, norm_right, cond(X^H X)).

    extended=False: float64 throughout, the statements of ref_numpy.promax as they stand.
    extended=True : the four N-sized sums (X^H X, X^H P, the two block Grams of h X) and the column maxima in np.longdouble,
                    the p x p algebra in float64 - the formulation of the device (norms from L^H S L)."""
    X = Bv
    h = np.sqrt(np.sum(X * X.conj(), axis=1))
    X = (1.0 / h)[:, None] * X
    if not extended:
        Xn = X / np.max(np.abs(X), axis=0)
        P = Xn * np.abs(Xn) ** (power - 1)
        XX = X.conj().T @ X
        L = np.linalg.inv(XX) @ X.conj().T @ P
    else:
        ext = np.clongdouble if np.iscomplexobj(X) else np.longdouble
        Xe = X.astype(ext)
        Xn = Xe / np.max(np.abs(Xe), axis=0)
        P = Xn * np.abs(Xn) ** (power - 1)
        cdt = X.dtype
        XX = (Xe.conj().T @ Xe).astype(cdt)
        XP = (Xe.conj().T @ P).astype(cdt)
        He = h.real.astype(np.longdouble)[:, None] * Xe
        SL = (He[:n_left].conj().T @ He[:n_left]).astype(cdt)
        SR = (He[n_left:].conj().T @ He[n_left:]).astype(cdt)
        L = np.linalg.inv(XX) @ XP
    scale = np.diag(np.diag(np.linalg.inv(L.conj().T @ L)))
    L = L @ np.sqrt(scale)
    B = h[:, None] * (X @ L)
    R = Rv @ L
    Linv = np.linalg.inv(L)
    Phi = Linv @ Linv.conj().T
    if not extended:
        nl = np.linalg.norm(B[:n_left], axis=0)
        nr = np.linalg.norm(B[n_left:], axis=0)
    else:
        nl = np.sqrt(np.maximum(np.diag(L.conj().T @ SL @ L).real, 0.0))
        nr = np.sqrt(np.maximum(np.diag(L.conj().T @ SR @ L).real, 0.0))
    return B, R, Phi, nl, nr, float(np.linalg.cond(XX))


TAIL_NAMES = ("B", "R", "Phi", "norm_left", "norm_right")


def tail_noise(Bv, Rv, power, n_left):
    """largest relative difference (`rel`) between the float64 and the extended evaluation of the tail, and cond(X^H X)"""
    a = promax_tail(Bv, Rv, power, n_left, extended=False)
    b = promax_tail(Bv, Rv, power, n_left, extended=True)
    return max(rel(a[i], b[i]) for i in range(5)), a[5]


def tail_bound(noise):
    """device bound of the decoupled tail from the largest reference noise over all cases; None when a case is too ill-conditioned"""
    bound = TAIL_MARGIN * noise
    if bound > TAIL_CAP:
        return None
    return max(bound, TAIL_FLOOR)
