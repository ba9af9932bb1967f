"""Matrices, expectations and measures shared by tests/test_gpu_partial_eigh.py (the leading-eigenvector stage of the
eigensolver against numpy.linalg.eigh), tests/test_partial_solve_host.py (the same spectra against the guard model, no device)
and scripts/partial_eigh_edges.py.

Every matrix is Q diag(lam) Q^H from seeded numpy (Q from a QR factorisation, real or complex) or comes from the generators
of tests/test_gpu_tridiag.py.  A case states what the device is expected to do with it:

  n_eigvec  eigenvectors formed: the k' >= k of the partial stage, or n (all of them, the leading k rows copied out);
  tridiag   1: finished on the tridiagonal route, 0: by the Jacobi sweeps, None: not stated (all n vectors are formed and the
            `repeated` test of the full stage looks at eigenvalues that are rounding noise);
  route_free  the guard compares gaps of this spectrum that lie within a factor 10 of its thresholds: the device's eigenvalues
            differ from LAPACK's by ~n eps ||A||, so only the numerical result is asserted;
  hard      bars of the near-degenerate spectra of tests/test_gpu_tridiag.py (1e-12, 1e-10, 1e-10) instead of those of the
            separated ones (1e-13, 1e-12, 1e-12): eigenvalues / ||A||, max |U^H U - I|, max ||A u - lam u|| / ||A||.
"""
import numpy as np

from test_gpu_tridiag import _glued_wilkinson, _gram

BARS = {False: (1e-13, 1e-12, 1e-12), True: (1e-12, 1e-10, 1e-10)}
CLEAR_GAP = 1e-6             # a cut or a mode is compared with LAPACK's vectors where the gaps exceed this times ||A||
ROUTE_MARGIN = 10.0          # stated routes hold while every inspected gap is this factor away from its threshold
DECAY = 0.9
# Where all vectors are formed and the tail of the spectrum is rounding noise, the `repeated` test hands the matrix to the
# Jacobi sweeps - with n_lead exactly as without it, bit for bit.  At the two largest orders their eigenvalues miss the 1e-13
# of the separated spectra: 1.26e-13 (n = 1025, complex) and 1.27e-13 ||A|| (n = 1100) for the call with n_lead AND for
# hip.eigh(A) on the same matrix, against 5.8e-16 for LAPACK's own error against the planted spectrum
# (profiles/partial_eigh_edges.json).  The bar of those cases is 4 times the larger figure, the margin
# tests/test_gpu_partial_solve.py uses: the call with n_lead must not be worse than the one without.
SWEEPS_EIG_BAR = 4 * 1.27e-13


def orthogonal(n, cplx, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    if cplx:
        B = B + 1j * rng.standard_normal((n, n))
    return np.linalg.qr(B)[0]


def from_spectrum(lam, cplx, seed):
    Q = orthogonal(len(lam), cplx, seed)
    A = (Q * np.asarray(lam, dtype=np.float64)) @ Q.conj().T
    return (A + A.conj().T) / 2


def geometric(n, scale=1.0):
    return scale * DECAY ** np.arange(n, dtype=np.float64)


def clustered(n, k, width, rel=1e-5):
    """geometric decay; behind mode k (1-based) `width` further values at relative spacing `rel`, the decay resumes behind them"""
    lam = np.empty(n)
    lam[:k] = DECAY ** np.arange(k)
    for j in range(width):
        lam[k + j] = lam[k + j - 1] * (1.0 - rel)
    lam[k + width:] = lam[k + width - 1] * DECAY ** np.arange(1, n - k - width + 1)
    return lam


def paired(n, pairs, rel):
    """`pairs` leading pairs (2 * 0.8^j and that times 1 - rel), a gap, then geometric decay"""
    top = 2.0 * 0.8 ** np.arange(pairs)
    lead = np.stack([top, top * (1.0 - rel)], axis=1).ravel()
    return np.r_[lead, 0.1 * DECAY ** np.arange(n - 2 * pairs)]


def bit_equal_pair(n, seed):
    """eigenvalues 2, 2, 1.5, 1.4 * 0.9^i with the double one applied exactly: the first and the last coordinate are
    eigenvectors of the eigenvalue 2 (a block 2 I of the matrix in its eigenbasis), the n - 2 coordinates between them carry
    Q diag(rest) Q^T.  No Householder reflector of the reduction touches either coordinate (column 0 is zero below the
    diagonal, and no column has an entry in the last row to remove), so the tridiagonal matrix holds 2 twice, uncoupled, and
    the multisection - the same bracket sequence for both indices - returns the same bits twice.  (Anywhere else a coordinate
    becomes the pivot row of the column in front of it and the reflector mixes it in: measured at coordinates 137 and 401, the
    two values came out ulps apart, and the partial stage finished with two good vectors.)"""
    rest = np.r_[1.5, 1.4 * DECAY ** np.arange(n - 3)]
    A = np.zeros((n, n))
    A[1:n - 1, 1:n - 1] = from_spectrum(rest, False, seed)
    A[0, 0] = A[n - 1, n - 1] = 2.0
    return A


def indefinite_zero_diagonal(n, cplx, scale):
    rng = np.random.default_rng(77)
    B = rng.standard_normal((n, n))
    if cplx:
        B = B + 1j * rng.standard_normal((n, n))
    A = (B + B.conj().T) * scale
    np.fill_diagonal(A, 0.0)
    return A


def low_rank(n, cols, seed):
    Y = np.random.default_rng(seed).standard_normal((n, cols))
    return Y @ Y.T


def wilkinson_dense(glue):
    T = _glued_wilkinson(30, glue)
    Q = orthogonal(T.shape[0], False, 11)
    G = Q @ T @ Q.T
    return (G + G.T) / 2


class Case:
    def __init__(self, name, build, k, n_eigvec, tridiag=1, hard=False, route_free=False, vec_min_n="2", matrix=None, planted=None,
                 spectrum=None, eig_bar=None):
        self.name, self._build, self.k = name, build, k
        self.spectrum = spectrum                # the eigenvalues the matrix was built from, where LAPACK's own error is wanted
        self.eig_bar = eig_bar                  # eigenvalue bar where the one of the table does not apply (SWEEPS_EIG_BAR)
        self.planted = planted                  # the spectrum by construction, where the guard's reading of it turns on exact bits
        self.n_eigvec, self.tridiag, self.hard, self.route_free = n_eigvec, tridiag, hard, route_free
        self.vec_min_n = vec_min_n              # XMCA_TRIDIAG_VEC_MIN_N of the call; None: the default threshold (768)
        self.matrix = matrix or name            # cases of one matrix share it and its LAPACK decomposition

    def __repr__(self):
        return self.name


def bars(case):
    """(eigenvalues / ||A||, max |U^H U - I|, max ||A u - lam u|| / ||A||) the case is held to"""
    b = BARS[case.hard]
    return (case.eig_bar if case.eig_bar is not None else b[0], b[1], b[2])


_MATRICES, _REFERENCES = {}, {}


def matrix(case):
    if case.matrix not in _MATRICES:
        A = case._build()
        A.setflags(write=False)
        _MATRICES[case.matrix] = A
    return _MATRICES[case.matrix]


def reference(case):
    """numpy.linalg.eigh of the case's matrix, descending, computed once per matrix: (lam, U, LAPACK's own largest residual
    ||A u - lam u||_2 / ||A||)"""
    if case.matrix not in _REFERENCES:
        A = matrix(case)
        lam, U = np.linalg.eigh(A)
        lam, U = lam[::-1].copy(), U[:, ::-1].copy()
        res = float(np.max(np.linalg.norm(A @ U - U * lam, axis=0)) / np.max(np.abs(lam)))
        for x in (lam, U):
            x.setflags(write=False)
        _REFERENCES[case.matrix] = (lam, U, res)
    return _REFERENCES[case.matrix]


def _separated():
    out = []
    for n, cplx in [(130, False), (514, False), (577, True), (1025, True), (1100, False)]:
        name = "sep%d%s" % (n, "c" if cplx else "")
        for k in sorted({1, 2, 15, 16, 17, 63, 64, 65, n // 4, n // 4 + 1, n - 1}):
            if k > n - 1:
                continue
            thin = 4 * k <= n
            # all vectors: the full stage; at n = 130 the whole spectrum is separated (0.9^129 = 1e-6) and it finishes there, at the
            # larger orders the tail is rounding noise and either the full stage or the sweeps end the call
            tridiag = 1 if thin or n == 130 else None
            # 0.9^275 / 10 = 2.6e-14 ||A|| behind mode 275 is 8 times the absolute rule's eps ||A|| / 0.0675
            free = (n, k) == (1100, 275)
            out.append(Case("%s_k%d" % (name, k), (lambda n=n, cplx=cplx: from_spectrum(geometric(n), cplx, 100 + n)), k,
                            k if thin else n, tridiag, route_free=free, matrix=name, spectrum=geometric(n),
                            eig_bar=SWEEPS_EIG_BAR if n >= 1025 and not thin else None))
    return out


def _build_cases():
    cases = _separated()
    add = cases.append
    # a pair at the cut, relative gap 1e-5: asked for k the partner comes along, asked for k + 1 the set is whole
    for cplx in (False, True):
        name = "cutpair" + ("c" if cplx else "")
        for k in (10, 11):
            add(Case("%s_k%d" % (name, k), (lambda cplx=cplx: from_spectrum(clustered(600, 10, 1), cplx, 21)), k, 11, hard=True, matrix=name))
    # clusters behind the cut: relative spacing 1e-5 inside, a clear gap after
    add(Case("cluster5_k10", lambda: from_spectrum(clustered(600, 10, 5), False, 22), 10, 15, hard=True))
    add(Case("cluster8_k60", lambda: from_spectrum(clustered(600, 60, 8), False, 23), 60, 68, hard=True))            # k' crosses a lane block
    add(Case("cluster32_k10", lambda: from_spectrum(clustered(600, 10, 32), False, 24), 10, 42, hard=True))          # as wide as the cap
    add(Case("cluster33_k10", lambda: from_spectrum(clustered(600, 10, 33), False, 25), 10, 600, None, hard=True))   # one wider
    add(Case("cluster8_k60_n260", lambda: from_spectrum(clustered(260, 60, 8), False, 26), 60, 260, 1, hard=True))   # 68 > 260 / 4
    # the absolute rule alone: a graded spectrum whose relative gaps are 0.07 throughout, cut at 1e-16 ||A||
    add(Case("graded20_k480", lambda: from_spectrum(np.logspace(0, -20, 600), False, 27), 480, 600, None, hard=True))
    # near-degenerate pairs INSIDE the set
    add(Case("pairs_1e-10", lambda: from_spectrum(paired(640, 10, 1e-10), False, 28), 20, 20, hard=True))
    add(Case("pairs_1e-12", lambda: from_spectrum(paired(640, 10, 1e-12), False, 29), 20, 20, hard=True))
    add(Case("pairs_1e-14", lambda: from_spectrum(paired(640, 10, 1e-14), False, 30), 20, 20, hard=True, route_free=True))
    # pairs 3e-15 apart in a spectrum WITHOUT a noise tail (0.1 * 0.9^139 = 4e-8): not `repeated`, so the partial stage runs, and
    # where its clean-up refuses the set (measured: it does) the full stage goes on with the compact-WY factors already joined
    add(Case("pairs_3e-15_n160", lambda: from_spectrum(paired(160, 10, 3e-15), False, 35), 20, None, None, hard=True, route_free=True))
    # 30 x W21+: the 60 largest eigenvalues lie in one cluster, whichever way the guard reads it the result has to stand
    add(Case("wilkinson_1e-5", lambda: wilkinson_dense(1e-5), 30, None, None, hard=True, route_free=True))
    add(Case("wilkinson_1e-7", lambda: wilkinson_dense(1e-7), 30, None, None, hard=True, route_free=True))
    # bit-equal leading pair: the sweeps, all vectors in scratch planes, two rows handed out
    # (LAPACK's QL iteration returns the pair 6 ulp apart; the two unit vectors ARE eigenvectors of exactly 2: the guard model is
    # asked about the planted values)
    add(Case("bitequal_k2", lambda: bit_equal_pair(600, 31), 2, 600, 0, hard=True, planted=np.r_[2.0, 2.0, 1.5, 1.4 * DECAY ** np.arange(597)]))
    # a null space of dimension 580 BEHIND the cut: the partial stage runs where the full solve goes to the sweeps
    add(Case("lowrank_k10", lambda: low_rank(600, 20, 32), 10, 10, hard=True))
    for cplx in (False, True):
        for scale in (1e6, 1e-6):
            # (the complex matrix has a relative gap of 3.6e-3 behind mode 10: within a factor 10 of the relative rule)
            add(Case("indefinite%s_%g" % ("c" if cplx else "", scale), (lambda cplx=cplx, scale=scale: indefinite_zero_diagonal(400, cplx, scale)),
                     10, 10, route_free=cplx))
    # negative definite: the leading eigenvalues are the ones closest to zero, ||A|| is |lam_n|
    add(Case("negdef_k10", lambda: -from_spectrum(geometric(200), False, 33), 10, 10))
    # below the default threshold of the tridiagonal route with vectors: the sweeps, hand_out into the pitched plane
    add(Case("jacobi300_k10", lambda: from_spectrum(geometric(300), False, 34), 10, 300, 0, vec_min_n=None))
    return cases


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}


def gram(n, cplx):
    """the Gram matrices of tests/test_gpu_tridiag.py (bit comparison of the call without n_lead)"""
    return _gram(n, cplx)


def measure(A, lam_ref, U_ref, res_ref, lam, U, hard):
    """figures of one result U (n x k) with all n eigenvalues lam, against LAPACK's: a dict of
    eig, orth, res (what the bars are for), and - where the gaps allow it - proj / proj_bound (the component of span U
    outside LAPACK's span, Frobenius norm, against Davis-Kahan: (residual bar + LAPACK's own residual) ||A|| / gap sqrt k) and
    vec / vec_bound (the worst phase-aligned single vector relative to its own bound)."""
    n, k = U.shape
    nrm = float(np.max(np.abs(lam_ref)))
    out = {"eig": float(np.max(np.abs(lam - lam_ref)) / nrm),
           "orth": float(np.max(np.abs(U.conj().T @ U - np.eye(k)))),
           "res": float(np.max(np.linalg.norm(A @ U - U * lam[:k], axis=0)) / nrm)}
    gaps = lam_ref[:-1] - lam_ref[1:]
    clear = gaps > CLEAR_GAP * nrm
    budget = (BARS[hard][2] + res_ref) * nrm
    if k < n and clear[k - 1]:
        V = U_ref[:, :k]
        out["proj"] = float(np.linalg.norm(U - V @ (V.conj().T @ U)))
        out["proj_bound"] = float(budget / gaps[k - 1] * np.sqrt(k))
    worst = None
    for i in range(k):
        left = clear[i - 1] if i > 0 else True
        right = clear[i] if i < n - 1 else True
        if not (left and right):
            continue
        gap = min([gaps[j] for j in (i - 1, i) if 0 <= j < n - 1])
        u, v = U[:, i], U_ref[:, i]
        ph = np.vdot(v, u)
        ph = ph / abs(ph) if abs(ph) > 0 else 1.0
        err, bound = float(np.linalg.norm(u - v * ph)), float(budget / gap)
        if worst is None or err / bound > worst[0] / worst[1]:
            worst = (err, bound)
    if worst is not None:
        out["vec"], out["vec_bound"] = worst
    return out
