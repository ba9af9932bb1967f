"""The cases of `xmca_amd.prepare.anomalies` and its numpy float64 restatement, shared by the host and GPU tests and
by scripts/anomalies_accuracy.py.

A case is (T, N, k); k names the basis (BASES).  A gap pattern is laid over the case's field deterministically, and the columns that
must come back fitted follow from integer counts alone (`expected_fitted`): a column is fitted when it has at least k present
values and - the indicator bases - a value in every phase; every basis here is well-posed on such a column (the host test checks the
smallest pivot share against PIVOT_FLOOR, far from the 1e-8 of the definition).

The restatement fits every column by `numpy.linalg.lstsq` on its present rows, applies the count rule and the pivot criterion by a
plain Cholesky loop, widens float32 inputs, fits in float64 and rounds once."""
import functools

import numpy as np

PIVOT_MIN = 1e-8
PIVOT_FLOOR = 0.5           # smallest d_j / A[j][j] the cases may show on a column that counts as fitted (the smallest is 0.67)

# k -> the arguments of time_basis: mean only, mean + trend, two harmonics + trend, monthly means + trend, the cap
BASES = {1: dict(), 2: dict(trend=True), 6: dict(period=12, harmonics=2, trend=True), 13: dict(period=12, trend=True),
         16: dict(period=16, harmonics=7, trend=True)}
INDICATOR = (13,)           # the bases with phase means: a phase without a value leaves the column unfitted

# T: 17 (the smallest record), 33 (the chunk cut of the column pass that leaves empty chunks; half a row tile + 1), 49 (four periods
# of 12 plus one), 130 (two row tiles of 64 and two rows).  N: the edges of one wave (63, 64, 65), of one workgroup (257), and 1.
# The two largest bases need two periods of record (24, 32 time steps) for the gap patterns to leave them well-posed.
CASES = [(17, 1, 1), (17, 64, 2), (17, 65, 6), (33, 63, 1), (33, 257, 6), (33, 64, 13), (49, 65, 13), (49, 1, 13), (49, 257, 16),
         (49, 63, 2), (130, 257, 13), (130, 64, 16), (130, 65, 1), (130, 1, 6), (130, 63, 16)]
PATTERNS = ("none", "random", "step", "column", "few", "phase")
PIPELINE_CASE = (49, 65, 13)


def case_name(case):
    return "T%d-N%d-k%d" % tuple(case)


def patterns_of(case):
    return [p for p in PATTERNS if p != "phase" or case[2] in INDICATOR]


def basis_of(case):
    from xmca_amd.prepare import time_basis
    return time_basis(case[0], **BASES[case[2]])


def _forced_rows(case):
    """the leading time steps that the random gaps leave alone: two periods of the basis, at most T; for a basis without a period
    min(T // 2, 24), so that the smallest records carry random gaps too"""
    T, period = case[0], BASES[case[2]].get("period")
    return min(T, 2 * period) if period else min(T // 2, 24)


@functools.lru_cache(maxsize=None)
def case_field(case, pattern, dtype="float64"):
    """(X, expected fitted mask): a seasonal cycle, a trend and noise about 15 (max|X| ~ 25) with the gaps of `pattern`"""
    T, N, k = case
    rng = np.random.default_rng(1000 * T + 10 * N + k)
    t = np.arange(T)[:, None]
    X = (15.0 + 5.0 * np.cos(2 * np.pi * t / 12.0 + rng.uniform(0, 6.28, N)) + 2.0 * np.sin(2 * np.pi * t / 6.0)
         + 0.02 * t * rng.standard_normal(N) + rng.standard_normal((T, N)))
    expected = np.ones(N, dtype=bool)
    if pattern != "none":
        gaps = rng.random((T, N)) < 0.3
        gaps[:_forced_rows(case)] = False
        X[gaps] = np.nan
    if pattern == "step":
        X[T - 2, :] = np.nan                      # (T - 2 >= the period: its phase keeps an earlier value)
    elif pattern == "column":
        X[:, N // 2] = np.nan
        expected[N // 2] = False
    elif pattern == "few":
        X[k - 1:, N - 1] = np.nan                 # k - 1 present values
        expected[N - 1] = False
    elif pattern == "phase":
        period = BASES[k]["period"]
        X[5::period, 0] = np.nan                  # no value of phase 5
        expected[0] = False
    X = X.astype(dtype)
    X.setflags(write=False)
    expected.setflags(write=False)
    return X, expected


def expected_fitted(case, X):
    """the fitted mask by integer counts alone: at least k present values and, for an indicator basis, a value in every phase"""
    T, N, k = case
    present = np.isfinite(X)
    ok = present.sum(axis=0) >= k
    if k in INDICATOR:
        period = BASES[k]["period"]
        for ph in range(period):
            ok &= present[ph::period].sum(axis=0) >= 1
    return ok


def pivot_shares(A):
    """d_j / A[j][j] of the Cholesky factorisation of A in the order of its columns (NaN after a pivot that is not positive)"""
    k = A.shape[0]
    L = np.zeros((k, k))
    out = np.full(k, np.nan)
    for j in range(k):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        out[j] = d / A[j, j] if A[j, j] > 0 else 0.0
        if not d > 0:
            break
        L[j, j] = np.sqrt(d)
        for r in range(j + 1, k):
            L[r, j] = (A[r, j] - np.dot(L[r, :j], L[j, :j])) / L[j, j]
    return out


def passes(A):
    s = pivot_shares(A)
    return bool(np.all(s > PIVOT_MIN))            # (False for a NaN)


def restate(X, B):
    """(field in X's dtype, coefficients k x N, fitted N) of a T x N field with NaN gaps on the T x k basis B"""
    dtype = X.dtype
    Xw = np.asarray(X, dtype=np.float64)
    T, N = Xw.shape
    k = B.shape[1]
    field = np.full((T, N), np.nan)
    coef = np.full((k, N), np.nan)
    fitted = np.zeros(N, dtype=bool)
    for n in range(N):
        p = np.isfinite(Xw[:, n])
        Bp = B[p]
        if p.sum() < k or not passes(Bp.T @ Bp):
            continue
        c = np.linalg.lstsq(Bp, Xw[p, n], rcond=None)[0]
        fitted[n] = True
        coef[:, n] = c
        field[p, n] = Xw[p, n] - Bp @ c
    return field.astype(dtype), coef, fitted


@functools.lru_cache(maxsize=None)
def reference(case, pattern, dtype="float64"):
    """the restatement of a case, computed once and shared (read-only)"""
    X, _ = case_field(case, pattern, dtype)
    out = restate(X, basis_of(case))
    for a in out:
        a.setflags(write=False)
    return out


def ulp32(x):
    """the spacing of float32 at |x|"""
    return float(np.spacing(np.float32(abs(x))))


def max_abs_diff(a, b):
    """max |a - b| over the entries where either is finite, NaN positions having to agree (else inf)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return np.inf
    d = np.abs(a - b)[~np.isnan(a)]
    return float(d.max()) if d.size else 0.0


def orthogonality(field, X, B, fitted):
    """max over the fitted columns n and the basis columns c of |sum_present b_tc r_tn| / sum_present |b_tc|: a weighted mean of the
    residual, so entries each within e of the exact residual keep it within e"""
    r = np.asarray(field, dtype=np.float64)
    present = np.isfinite(np.asarray(X, dtype=np.float64))[:, fitted]
    r = np.where(present, r[:, fitted], 0.0)
    worst = 0.0
    for c in range(B.shape[1]):
        num = np.abs(np.einsum("t,tn->n", B[:, c], r))
        den = np.einsum("t,tn->n", np.abs(B[:, c]), present.astype(np.float64))
        if num.size:
            worst = max(worst, float(np.max(num / den)))
    return worst


def figures(case, pattern, dtype, out, again):
    """What the device's result `out` = anomalies(X) and `again` = anomalies(out['field']) show against the restatement, in the units
    of the bounds: float64 fields in max|X|, float32 fields in float32 ulps of max|X|, coefficients in max|X| (re-fitted float32
    ones in ulps)."""
    X, _ = case_field(case, pattern, dtype)
    field, coef, fitted = reference(case, pattern, dtype)
    top = float(np.nanmax(np.abs(X))) if np.isfinite(X).any() else 1.0
    unit = top if np.dtype(dtype) == np.float64 else ulp32(top)
    B = basis_of(case)
    refit = np.asarray(again["coefficients"])
    return {"field": max_abs_diff(out["field"], field) / unit,
            "coefficients": max_abs_diff(out["coefficients"].reshape(coef.shape), coef) / top,
            "orthogonality": orthogonality(out["field"], X, B, fitted) / unit,
            "refit": (float(np.nanmax(np.abs(refit))) if np.isfinite(refit).any() else 0.0) / unit}
