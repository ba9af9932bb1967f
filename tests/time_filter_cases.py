"""What the tests of `xmca_amd.prepare.time_filter` compare with: a numpy restatement of the definition - the same
ascending chain in float64 (a multiply and an add per tap where the device uses one fma), a longdouble truth beside it, the NaN rules
spelled out with plain loops - the per-entry error bound of the issue, and the deterministic, seeded cases.

The cases are placed around the tile of the filter kernel, R = 16 output rows x C = 256 columns (`_hip.time_filter_tile()`; a test
asserts that they straddle the tile the library reports): T in {R - 1, R, R + 1, 2 R + 1} and more, N in {1, C - 1, C, C + 1,
4 C + 1}, L in {1, 3, 2 R + 1, 1025} (2 R + 1: the halo is wider than a tile)."""
import functools

import numpy as np

from xmca_amd.prepare import lanczos_weights

R, C = 16, 256
U = 2.0 ** -53

# (name, T, N, L, weights, gap pattern, min_weight, modes)
CASES = [
    ("one-weight", R - 1, 1, 1, "sym", "none", 0.5, "snr"),
    ("one-weight-gaps", 2 * R + 1, C, 1, "asym", "scattered", 0.5, "snr"),
    ("three-scattered", R, C - 1, 3, "asym", "scattered", 0.5, "snr"),
    ("three-step", R + 1, C, 3, "sym", "step", 0.6, "snr"),
    ("three-none", R, C + 1, 3, "sym", "none", 0.5, "snr"),
    ("three-column", 2 * R + 1, 4 * C + 1, 3, "sym", "column", 0.7, "snr"),
    ("halo-scattered", 2 * R + 1, C + 1, 2 * R + 1, "asym", "scattered", 0.4, "snr"),
    ("halo-sparse", 5 * R + 3, C + 1, 2 * R + 1, "sym", "sparse", 0.5, "snr"),
    ("halo-run", 100, 65, 2 * R + 1, "sym", "run", 0.3, "snr"),
    ("halo-edges", 100, C - 1, 2 * R + 1, "asym", "edges", 0.5, "snr"),
    ("halo-band", 6 * R + 1, C + 1, 2 * R + 1, "band", "step", 0.5, "sn"),
    ("short-record", R + 4, C + 1, 2 * R + 1, "sym", "scattered", 0.5, "sr"),
    ("long-column", 1100, 20, 1025, "sym", "column", 0.5, "snr"),
    ("long-short-record", 700, 20, 1025, "asym", "scattered", 0.45, "sr"),
]
# modes: s = strict with edges='nan', n = strict with edges='trim' (needs T >= L), r = renormalise
MODES = {"s": dict(missing="nan", edges="nan"), "n": dict(missing="nan", edges="trim"), "r": dict(missing="renormalise", edges="nan")}
PATTERNS = ("none", "scattered", "sparse", "step", "column", "run", "edges")
DTYPES = ("float64", "float32")


def case_name(case):
    return case[0]


def runs():
    """every (case, mode letter, complement) the GPU tests run"""
    return [(case, m, comp) for case in CASES for m in case[7] for comp in (False, True)]


def case_weights(case):
    name, T, N, L, kind, pattern, min_weight, modes = case
    if kind == "sym":
        return lanczos_weights(L, 0.1)
    if kind == "band":
        return lanczos_weights(L, (0.08, 0.25))
    rng = np.random.default_rng(1000 + L)          # asymmetric, mixed signs, sum 1
    w = rng.uniform(-0.25, 1.0, L)
    return w / w.sum()


def case_field(case, dtype="float64"):
    """The T x N field of a case in `dtype`: 10 + noise + a slow wave, with the gaps of its pattern as NaN."""
    name, T, N, L, kind, pattern, min_weight, modes = case
    h = L // 2
    rng = np.random.default_rng(7 * T + 13 * N + L)
    X = 10.0 + rng.standard_normal((T, N)) + 3.0 * np.cos(2 * np.pi * 0.03 * np.arange(T))[:, None]
    if pattern == "scattered":
        X[rng.random((T, N)) < 0.10] = np.nan
    elif pattern == "sparse":          # few enough that strict windows survive
        X[rng.random((T, N)) < 0.004] = np.nan
    elif pattern == "step":
        X[T // 2] = np.nan
    elif pattern == "column":
        X[:, N // 3] = np.nan
        X[T // 2 + 3, -1] = np.nan
    elif pattern == "run":             # a run longer than L in every third column, at staggered places
        for n in range(0, N, 3):
            start = 5 + (7 * n) % (T - L - 12)
            X[start:start + L + 7, n] = np.nan
    elif pattern == "edges":           # the first and last h steps
        X[:h] = np.nan
        X[T - h:] = np.nan
    else:
        assert pattern == "none", pattern
    return X.astype(dtype)


def weight_sum(w):
    """sum(w) in ascending order in float64 (what `time_filter` multiplies min_weight with)"""
    s = np.float64(0.0)
    for v in np.asarray(w, dtype=np.float64):
        s = s + v
    return float(s)


def sums(X, w, real=np.float64):
    """The window sums of the definition in the arithmetic `real`, tap by tap in ascending k, each entry's chain starting from +0:
    num = sum_present w_k x, den = sum_present w_k, absx = sum_present |w_k x|, absw = sum_present |w_k|, and the number of entries of
    the window that are missing or outside the record.  (T, N) each."""
    X = np.asarray(X)
    w = np.asarray(w, dtype=np.float64)
    T, N = X.shape
    L = w.size
    h = L // 2
    present = np.zeros((T + 2 * h, N), dtype=bool)          # rows outside the record count as missing
    present[h:h + T] = ~np.isnan(X)
    wide = np.zeros((T + 2 * h, N), dtype=real)
    wide[h:h + T] = np.where(np.isnan(X), 0.0, X.astype(real))
    num, den, absx, absw = (np.zeros((T, N), dtype=real) for _ in range(4))
    gone = np.zeros((T, N), dtype=np.int64)
    for k in range(L):                                      # window entry k of output row t is row t + k - h: padded row t + k
        p = present[k:k + T]
        x = wide[k:k + T]
        wk = real(w[k])
        num = np.where(p, num + wk * x, num)
        den = np.where(p, den + wk, den)
        absx = np.where(p, absx + abs(wk) * np.abs(x), absx)
        absw = np.where(p, absw + abs(wk), absw)
        gone += ~p
    return num, den, absx, absw, gone


def nan_rule(X, gone, den, den_min, renormalise):
    """The NaN positions of the result on the full record, entry by entry: strict - any of the L window entries missing or outside;
    renormalise - X[t, n] itself missing, or den < den_min."""
    T, N = X.shape
    out = np.zeros((T, N), dtype=bool)
    for t in range(T):
        for n in range(N):
            if renormalise:
                out[t, n] = bool(np.isnan(X[t, n])) or bool(den[t, n] < den_min)
            else:
                out[t, n] = gone[t, n] > 0
    return out


def restate(X, w, complement=False, missing="nan", min_weight=0.5, edges="nan"):
    """`time_filter` in numpy float64: the ascending chain, the output rounded once to the dtype of X."""
    X = np.asarray(X)
    w = np.asarray(w, dtype=np.float64)
    h = w.size // 2
    num, den, _, _, gone = sums(X, w)
    renorm = missing == "renormalise"
    den_min = float(np.float64(min_weight) * np.float64(weight_sum(w))) if renorm else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        S = num / den if renorm else num
    y = X.astype(np.float64) - S if complement else S
    y = np.where(nan_rule(X, gone, den, den_min, renorm), np.nan, y).astype(X.dtype)
    return y[h:X.shape[0] - h] if edges == "trim" else y


@functools.lru_cache(maxsize=None)
def _truth_sums(name, dtype):
    case = next(c for c in CASES if c[0] == name)
    X = case_field(case, dtype)
    w = case_weights(case)
    return X, w, sums(X, w, np.longdouble), sums(X, w)


@functools.lru_cache(maxsize=None)
def expected_nan(name, dtype, renorm):
    """the NaN positions of a case on the full record, by `nan_rule` on the float64 chain of the denominators"""
    case = next(c for c in CASES if c[0] == name)
    X, w, _, (num64, den64, _, _, gone) = _truth_sums(name, dtype)
    den_min = float(np.float64(case[6]) * np.float64(weight_sum(w))) if renorm else 0.0
    return nan_rule(X, gone, den64, den_min, renorm)


def reference(case, mode, complement, dtype):
    """(expected NaN mask, truth in longdouble, per-entry bound) of a run, on the rows the mode returns.  The bound, nothing of it
    measured: 2 [(L + 4) 2^-53 (sum |w_k x| + |S| sum_present |w_k|) / |den| + 2^-53 (|x_t| + |y|)], in strict mode den = 1 and the
    |S| sum |w| term absent; float32 adds half a float32 spacing at |y|; the factor 2 covers the higher-order terms of the
    first-order chain bound.  The NaN mask follows the float64 chain of the denominators (the device's: adding w_k is exact in both)."""
    name, T, N, L, kind, pattern, min_weight, modes = case
    X, w, (num, den, absx, absw, gone), _ = _truth_sums(name, dtype)
    renorm = MODES[mode]["missing"] == "renormalise"
    h = L // 2
    isnan = expected_nan(name, dtype, renorm)
    x = np.where(np.isnan(X), 0.0, X.astype(np.longdouble))
    with np.errstate(invalid="ignore", divide="ignore"):
        if renorm:
            S = num / den
            chain = (absx + np.abs(S) * absw) / np.abs(den)
        else:
            S = num
            chain = absx
        y = x - S if complement else S
        bound = 2 * ((L + 4) * U * chain + U * (np.abs(x) + np.abs(y)))
        if dtype == "float32":
            bound = bound + 0.5 * np.spacing(np.abs(y).astype(np.float32)).astype(np.longdouble)
    if MODES[mode]["edges"] == "trim":
        isnan, y, bound = isnan[h:T - h], y[h:T - h], bound[h:T - h]
    return isnan, y, bound


def worst_ratio(got, isnan, y, bound):
    """the largest error / bound over the entries that are not NaN (0 when there is none)"""
    live = ~isnan
    if not live.any():
        return 0.0
    err = np.abs(got.astype(np.longdouble)[live] - y[live])
    return float(np.max(err / bound[live]))


def threshold_margin(case, dtype="float64"):
    """min |den - den_min| / sum |w| over all entries of a renormalise case, in longdouble"""
    name, T, N, L, kind, pattern, min_weight, modes = case
    X, w, (num, den, absx, absw, gone), _ = _truth_sums(name, dtype)
    den_min = np.longdouble(float(np.float64(min_weight) * np.float64(weight_sum(w))))
    return float(np.min(np.abs(den - den_min)) / np.sum(np.abs(w)))


def response(w, f):
    """sum_k w_k cos(2 pi f (k - h)): what a cosine of frequency f is scaled by (symmetric weights)"""
    w = np.asarray(w, dtype=np.float64)
    h = w.size // 2
    return float(np.sum(w * np.cos(2 * np.pi * f * (np.arange(w.size) - h))))
