"""Inputs and measures shared by tests/test_gpu_partial_solve.py, tests/test_partial_solve_host.py and
scripts/partial_solve_accuracy.py: planted fields from seeded numpy.

A planted field is a sum of p = k + 6 orthogonal modes - orthonormal time series (orthogonal to the constant, so centering
leaves them alone) times orthonormal maps - with amplitudes 0.8^i, plus white noise whose largest singular value is about
1e-3 of the last planted amplitude.  sigma^2 then falls by 0.64 from mode to mode: a relative gap of 0.36 behind every
leading mode, far above the 1e-3 at which the guard of the partial eigenvector stage starts to extend the set."""
import numpy as np

PLANTED_EXTRA = 6
PLANTED_DECAY = 0.8
GUARD_RELGAP = 1e-3          # csrc/jacobi.h TRD_PARTIAL_RELGAP


def planted_amplitudes(k, tie=None):
    """amplitudes of the k + 6 planted modes; tie = (i, rel): amplitude i + 1 (0-based) is set to amplitude i * (1 - rel)"""
    a = PLANTED_DECAY ** np.arange(k + PLANTED_EXTRA, dtype=np.float64)
    if tie is not None:
        i, rel = tie
        a[i + 1] = a[i] * (1.0 - rel)
    return a


def planted_fields(T, Ns, k, seed, dtype=np.float64, tie=None):
    """list of centred-on-arrival fields (T x N for N in Ns) sharing their planted time series"""
    rng = np.random.default_rng(seed)
    a = planted_amplitudes(k, tie)
    p = a.size
    Q, _ = np.linalg.qr(np.concatenate([np.ones((T, 1)), rng.standard_normal((T, p))], axis=1))
    Qt = Q[:, 1:]                                            # orthonormal, orthogonal to the constant
    out = []
    for N in Ns:
        Qs, _ = np.linalg.qr(rng.standard_normal((N, p)))
        noise = rng.standard_normal((T, N)) * (1e-3 * a[-1] / (np.sqrt(T) + np.sqrt(N)))
        out.append(((Qt * a) @ Qs.T + noise).astype(dtype))
    return out


def gram_spectrum(X, complexify=False):
    """eigenvalues (descending) of the float64 Gram matrix of the centred field (of its analytic signal: complexify)"""
    Xc = np.asarray(X, dtype=np.float64)
    Xc = Xc - Xc.mean(axis=0)
    if complexify:
        from scipy.signal import hilbert
        Xc = hilbert(Xc, axis=0)
    return np.linalg.eigvalsh(Xc @ Xc.conj().T)[::-1]


def mode_error(A, B):
    """largest per-mode difference of phase-aligned columns, relative to the mode's largest entry"""
    ph = np.sum(np.conj(B) * A, axis=0)
    ph = np.where(np.abs(ph) > 0, ph / np.maximum(np.abs(ph), 1e-300), 1.0)
    A = A / ph
    return float(np.max(np.max(np.abs(A - B), axis=0) / np.max(np.abs(B), axis=0)))


def orth_defect(V):
    return float(np.max(np.abs(V.conj().T @ V - np.eye(V.shape[1]))))


def flat(eofs):
    """(space..., modes) -> (N, modes)"""
    e = np.asarray(eofs)
    return e.reshape(-1, e.shape[-1])


# (name, T, Ns, complexify, dtype, ks): the smallest shapes that reach each branch of the partial route
#   768: the threshold of the tridiagonal route with vectors, on the dual side;  800: no multiple of 64, 128 or 512;
#   1100: more than two super-blocks of 512 reflectors;  1600 complexified: an analytic-signal subspace of dimension 801 (complex
#   planes);  k = 64 / 65: one block of the twisted kernel, and one column more
ONE_FIELD_CASES = [
    ("t768", 768, (1100,), False, np.float64, (10,)),
    ("t800", 800, (1000,), False, np.float64, (1, 2, 10, 64, 65)),
    ("t1100", 1100, (1300,), False, np.float64, (10, 65)),
    ("t1600c", 1600, (1700,), True, np.float64, (10,)),
    ("t800f32", 800, (1000,), False, np.float32, (10,)),
]
TWO_FIELD_CASE = ("t800two", 800, (1000, 900), False, np.float64, (10,))
TWO_FIELD_CPLX_CASE = ("t800twoc", 800, (1000, 900), True, np.float64, (10,))      # both wide, complexified: the analytic-signal frame
JACOBI_CASE = ("t300", 300, (500,), False, np.float64, (10,))


ALL_CASES = {c[0]: c for c in ONE_FIELD_CASES + [TWO_FIELD_CASE, TWO_FIELD_CPLX_CASE, JACOBI_CASE]}


def case_seed(name, k):
    return 1000 * sum(ord(c) for c in name) + k


def case_fields(name, k, tie=None):
    _, T, Ns, cplx, dtype, _ = ALL_CASES[name]
    return planted_fields(T, Ns, k, case_seed(name, k), dtype, tie)


def oracle(fields, cplx, k):
    """float64 reference (oracle/ref_numpy.py, SVD) on the same input: (V per field: N x k, pcs per field: T x k)"""
    from oracle import ref_numpy as O
    X = [O.flatten_and_center(np.asarray(f, dtype=np.float64))[0] for f in fields]
    ref = O.solve(X, complexify=cplx)
    V = [v[:, :k] for v in ref["V"]]
    pcs = [x @ v / np.sqrt(ref["singular_values"][:k]) for x, v in zip(ref["fields"], V)]
    return V, pcs


def model_state(m):
    """what `solve(n_modes=k)` and `solve()` + `truncate(k)` have to agree on, besides the vectors"""
    out = {"analysis": dict(m._analysis), "singular_values": m.singular_values(), "explained_variance": m.explained_variance(),
           "scf": m.scf(), "rule_north": m.rule_north()}
    for key, v in m.norm().items():
        out["norm_" + key] = v
    return out


_RUNS = {}


def run_case(hip, name, k):
    """The full solve (+ truncate) and then, on the SAME handle, solve(n_modes=k) of one case - each once per process: states,
    eofs(k) / pcs(k), the handle's reports, and the float64 oracle."""
    if (name, k) in _RUNS:
        return _RUNS[(name, k)]
    from xmca_amd.array import MCA, _LazyVectors
    _, T, Ns, cplx, dtype, _ = ALL_CASES[name]
    fields = case_fields(name, k)
    keys = ["left", "right"][:len(fields)]
    full = MCA(*fields, handle=hip)
    full.solve(complexify=cplx)
    r = {"T": T, "Ns": Ns, "dtype": np.dtype(dtype), "keys": keys, "cplx": cplx}
    r["full_info"] = hip.solve_info()
    r["full_result"] = hip.result_info()
    r["full_eofs"] = {key: flat(v) for key, v in full.eofs(k).items()}
    r["full_pcs"] = full.pcs(k)
    full.truncate(k)
    r["full_state"] = model_state(full)
    part = MCA(*fields, handle=hip)
    part.solve(complexify=cplx, n_modes=k)
    r["part_info"] = hip.solve_info()
    r["part_result"] = hip.result_info()
    r["part_lazy"] = isinstance(part._V, _LazyVectors) and part._V._pending == set(keys) and part._V._rank
    r["part_eofs"] = {key: flat(v) for key, v in part.eofs(k).items()}
    r["part_pcs"] = part.pcs(k)
    r["still_resident"] = part._vectors_resident()
    r["part_state"] = model_state(part)
    oV, opcs = oracle(fields, cplx, k)
    r["oracle_eofs"] = dict(zip(keys, oV))
    r["oracle_pcs"] = dict(zip(keys, opcs))
    _RUNS[(name, k)] = r
    return r
