"""The numpy twin of `MCA.bootstrap_eofs` and the cases shared by tests/test_bootstrap_patterns_host.py and
tests/test_gpu_bootstrap_patterns.py.

Definition.  v0_s[:, j]: the model's unit singular vector of side s, mode j < k.  Replicate r resamples the time steps of every
field with the row index idx[r] (independent draws from the original fields), is centred, Hilbert-transformed if the model is
complex, and decomposed; v^r_s[:, j] are its k leading vectors.  c_rj = sum_s sum_n conj(v0_s[n, j]) v^r_s[n, j];
g_rj = |c_rj| / n_fields; u_rj = conj(c_rj) / |c_rj| (1 where c_rj = 0); d = u_rj v^r - v0; S = sum_r d, Q = sum_r |d|^2;
mean = v0 + S / R, std = sqrt(max(0, Q - |S|^2 / R) / (R - 1))."""
import numpy as np
from scipy.signal import hilbert

from golden_inputs import _signal_field

# (T, N or (N_left, N_right), k, block_size) of the end-to-end cases
E2E_SHAPES = [(36, 70, 3, 3), (36, (70, 45), 3, 3), (24, 300, 2, 1), (40, 17, 2, 4), (30, 63, 2, 2), (30, (65, 64), 2, 2),
              (30, 257, 3, 5), (100, 40, 3, 5)]
E2E_RUNS = 8
MIN_RELGAP = 0.005


def case_fields(T, N, k, seed=0):
    """One or two real T x N fields with k + 1 planted modes driven by the same time series"""
    rng = np.random.default_rng([seed, T, k] + list(np.atleast_1d(N)))
    shared = rng.standard_normal((T, k + 1))
    return [_signal_field(rng, T, int(n), k + 1, decay=0.5, noise=0.3, pcs=shared)[0] for n in np.atleast_1d(N)]


def leading_vectors(fields, k, cplx):
    """([N_s x k unit vectors per side], all singular values) of real fields: centred, `scipy.signal.hilbert` along time if
    cplx, then the SVD of the field (one) or of X^H Y / (T - 1) (two)"""
    Z = [np.asarray(f, dtype=np.float64) - np.asarray(f, dtype=np.float64).mean(axis=0) for f in fields]
    if cplx:
        Z = [hilbert(z, axis=0) for z in Z]
    T = Z[0].shape[0]
    if len(Z) == 1:
        _, s, vh = np.linalg.svd(Z[0], full_matrices=False)
        return [vh[:k].conj().T], s ** 2 / (T - 1)
    p, s, qh = np.linalg.svd(Z[0].conj().T @ Z[1] / (T - 1), full_matrices=False)
    return [p[:, :k], qh[:k].conj().T], s


def pattern_stats(v0, reps):
    """The statistics of the definition.  v0: [N_s x k per side]; reps: per run [N_s x k per side].
    Returns (mean per side, std per side, congruence k x R)."""
    R, k, n_fields = len(reps), v0[0].shape[1], len(v0)
    cplx = any(np.iscomplexobj(v) for v in v0) or any(np.iscomplexobj(v) for rep in reps for v in rep)
    dt = np.complex128 if cplx else np.float64
    v0 = [np.asarray(v, dtype=dt) for v in v0]
    S = [np.zeros(v.shape, dtype=dt) for v in v0]
    Q = [np.zeros(v.shape) for v in v0]
    g = np.zeros((k, R))
    for r, rep in enumerate(reps):
        # (summed along a contiguous axis: numpy adds pairwise there, which is what the rounding bound of the GPU test counts on)
        c = sum(np.ascontiguousarray((a.conj() * np.asarray(v, dtype=dt)).T).sum(axis=1) for a, v in zip(v0, rep))
        mag = np.abs(c)
        u = np.where(mag > 0, np.conj(c) / np.where(mag > 0, mag, 1.0), 1.0)
        g[:, r] = mag / n_fields
        for s in range(n_fields):
            d = u * np.asarray(rep[s], dtype=dt) - v0[s]
            S[s] += d
            Q[s] += np.abs(d) ** 2
    mean = [a + x / R for a, x in zip(v0, S)]
    std = [np.sqrt(np.maximum(0.0, q - np.abs(x) ** 2 / R) / (R - 1)) for q, x in zip(Q, S)]
    return mean, std, g


def twin(fields, idx, k, cplx):
    """`bootstrap_eofs` in numpy: dict with v0, mean, std (lists per side, N_s x k), congruence and singular_values (k x R) and
    min_relgap, the smallest relative gap (s_i - s_{i+1}) / s_i, i < k, among the k + 1 leading singular values of any replicate"""
    fields = [np.asarray(f, dtype=np.float64) for f in fields]
    v0, _ = leading_vectors(fields, k, cplx)
    reps, sig, gap = [], [], np.inf
    for rows in np.asarray(idx):
        v, s = leading_vectors([f[rows] for f in fields], k, cplx)
        reps.append(v)
        sig.append(s[:k])
        gap = min(gap, float(np.min((s[:k] - s[1:k + 1]) / s[:k])))
    mean, std, g = pattern_stats(v0, reps)
    return {'v0': v0, 'mean': mean, 'std': std, 'congruence': g, 'singular_values': np.array(sig).T, 'min_relgap': gap}


def mode_phases(v0_mine, v0_twin):
    """u (k,) with u_j v0_twin[:, j] ~ v0_mine[:, j], jointly over the sides: the sign / phase a decomposition is free to choose"""
    c = sum((b.conj() * a).sum(axis=0) for a, b in zip(v0_mine, v0_twin))
    return c / np.abs(c)


def random_replicates(rng, N, k, R, cplx, spread=0.5):
    """v0 and R replicates for the kernel tests, per side of width N[s]: unit columns; a replicate is v0 plus `spread` times a random
    unit vector, normalised, times one random sign / phase per (run, mode) shared by the sides.  The LAST run is orthogonal to v0
    with c = 0 exactly: v0 is zero at the last grid point of every side and that run is the unit vector there (the zero vector
    where N = 1)."""
    def unit(shape):
        x = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0.0)
        return x

    v0, reps = [], [[] for _ in range(R)]
    phase = np.exp(2j * np.pi * rng.random((R, k))) if cplx else rng.choice([-1.0, 1.0], (R, k))
    for n in N:
        a = unit((n, k))
        if n > 1:
            a[-1] = 0.0
        a /= np.linalg.norm(a, axis=0)
        v0.append(a)
        for r in range(R - 1):
            w = unit((n, k))
            w /= np.linalg.norm(w, axis=0)
            v = a + spread * w
            reps[r].append(phase[r] * v / np.linalg.norm(v, axis=0))
        last = np.zeros((n, k), dtype=a.dtype)
        if n > 1:
            last[-1] = 1.0
        reps[R - 1].append(last)
    return v0, reps
