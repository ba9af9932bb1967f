"""What the tests of `xmca_amd.lagged.lead_lag_maps` compare with: a numpy restatement of the definition in the
device's summation order - the same ascending chains in float64 (a multiply and an add where the device uses one fma), the same
restatement in longdouble as the truth - the per-entry error bound of the issue, a Python restatement of the moment kernel's index
rules with its bounds asserted, and the deterministic, seeded cases.

The cases are placed around the tile of the moment kernel (`_hip.lead_lag_tile()`; a test asserts that they straddle the tile the
library reports): C = 256 columns of a workgroup, R = 8 rows of a piece, G(q) = 8, 6, 4, 3, 3, 2, 2, 2 lags of a group.  T in
{R - 1, R, R + 1, 2 R + 1, 97, 300}, N in {1, C - 1, C, C + 1, 4 C + 1}, q in {1, 2, 3, 5, 8}, lag lists of length
{1, G - 1, G, G + 1, 2 G + 1} - unsorted, with negative lags, +-(T - 1) (one pair), the lag with exactly min_pairs pairs and the one
with min_pairs - 1 - and nine gap patterns."""
import functools

import numpy as np

from xmca_amd import lagged

C, R = 256, 8
GROUPS = (8, 6, 4, 3, 3, 2, 2, 2)          # G(q), q = 1 .. 8
U = 2.0 ** -53
LIVE = 2.0 ** -40

# (name, T, N, q, lags, gap pattern, min_pairs)
CASES = [
    ("tiny-one", R - 1, 1, 1, (0,), "none", 3),                                                       # 1 lag
    ("tiny-ends", R - 1, C - 1, 1, (0, 4, -4, 5, -5, 6, -6), "none", 3),                               # G - 1; 3 pairs, 2 pairs, 1 pair
    ("piece", R, C, 2, (3, -2, 0, 1, -1, 2), "scattered", 3),                                          # G
    ("piece-plus", R + 1, C + 1, 3, (0, -1, 1, -3, 4), "step", 3),                                     # G + 1
    ("two-pieces", 2 * R + 1, 4 * C + 1, 5, (0, 1, -1, 2, -2, 9, -8), "column", 4),                    # 2 G + 1
    ("few", 97, C + 1, 8, (0, 5, -5, 12, -12), "few", 8),                                              # 2 G + 1
    ("run", 97, C - 1, 2, (4, -6, 0, 1, -1, 2, -2, 3, -3, 6, -4, 5, -5), "run", 8),                    # 2 G + 1
    ("edges", 97, C, 1, (-4, -3, -2, -1, 0, 1, 2, 3, 4), "edges", 8),                                  # G + 1
    ("alternate", 300, C + 1, 2, (0, 1, -1, 2, -7), "alternate", 8),                                   # G - 1
    ("constant", 300, C, 3, (0, 10, -10), "constant", 8),                                              # G - 1
    ("long-lags", 300, C + 1, 1, (0, 299, -299, 292, -292, 293, -293, 150, -150, 1, -1, 7, -13, 64, -64, 200, -250), "none", 8),   # 2 G + 1
    ("q5-groups", 97, 1, 5, (7, -3, 0), "scattered", 8),                                               # G
    ("q5-short", 97, C - 1, 5, (-1, 1), "scattered", 8),                                               # G - 1
    ("q8-group", 2 * R + 1, C, 8, (1, -2), "scattered", 3),                                            # G
    ("q8-plus", 97, 1, 8, (2, 0, -30), "run", 8),                                                      # G + 1
    ("q3-wide", 97, C - 1, 3, (0, 3, -3, 20, -20, 48, -48, 88, -89), "scattered", 8),                  # 2 G + 1; 9 and 8 pairs before gaps
    ("q1-group", 2 * R + 1, C + 1, 1, (0, 1, 2, 3, -1, -2, -3, 8), "scattered", 3),                    # G
]
PATTERNS = ("none", "scattered", "step", "column", "few", "run", "edges", "alternate", "constant")
DTYPES = ("float64", "float32")
DOFS = ("n", "bretherton")


def case_name(case):
    return case[0]


def case_by_name(name):
    return next(c for c in CASES if c[0] == name)


def case_index(case):
    """The (T, q) index of a case: AR(1) series with an offset (so that the centring matters), the first of them in the field."""
    name, T, N, q, lags, pattern, min_pairs = case
    rng = np.random.default_rng(31 * T + 7 * q + 1)
    e = rng.standard_normal((T, q))
    y = np.empty((T, q))
    y[0] = e[0]
    for t in range(1, T):
        y[t] = 0.6 * y[t - 1] + 0.8 * e[t]
    return y * (1.0 + 0.5 * np.arange(q)) + 5.0 - np.arange(q)


def case_field(case, dtype="float64"):
    """The T x N field of a case in `dtype`: 10 + noise + a slow wave + the first index delayed by two steps, with the gaps of its
    pattern as NaN."""
    name, T, N, q, lags, pattern, min_pairs = case
    rng = np.random.default_rng(7 * T + 13 * N + q)
    y0 = case_index(case)[:, 0]
    X = 10.0 + rng.standard_normal((T, N)) + 3.0 * np.cos(2 * np.pi * 0.03 * np.arange(T))[:, None]
    X[2:] += 0.7 * np.cos(np.arange(N))[None, :] * (y0[:-2, None] - y0.mean())
    if pattern == "scattered":
        X[rng.random((T, N)) < 0.10] = np.nan
    elif pattern == "step":                # a wholly missing time step
        X[T // 2] = np.nan
    elif pattern == "column":              # a wholly missing column, and a single gap in the last one
        X[:, N // 3] = np.nan
        X[T // 2 + 3, -1] = np.nan
    elif pattern == "few":                 # a column with min_pairs - 1 values, one with exactly min_pairs, scattered gaps elsewhere
        X[rng.random((T, N)) < 0.10] = np.nan
        X[:, 3] = np.nan
        X[10:10 + 2 * (min_pairs - 1):2, 3] = 10.0 + rng.standard_normal(min_pairs - 1)
        X[:, N - 2] = np.nan
        X[20:20 + min_pairs, N - 2] = 10.0 + rng.standard_normal(min_pairs)
    elif pattern == "run":                 # a run longer than the largest lag in every third column, at staggered places
        longest = max(abs(l) for l in lags) + 5
        for n in range(0, N, 3):
            start = 3 + (7 * n) % (T - longest - 6)
            X[start:start + longest, n] = np.nan
    elif pattern == "edges":               # the first and last steps
        X[:3] = np.nan
        X[T - 2:] = np.nan
    elif pattern == "alternate":           # columns present at every second step only: no neighbours, |P| = 0
        X[1::2, 0] = np.nan
        X[0::2, N // 2] = np.nan
        X[rng.random((T, N)) < 0.03] = np.nan
    elif pattern == "constant":            # exactly constant columns with a dyadic value, one of them with gaps
        X[:, 5] = 12.5
        X[:, N - 1] = -0.375
        X[rng.random(T) < 0.2, N - 1] = np.nan
    else:
        assert pattern == "none", pattern
    return X.astype(dtype)


# ---- the definition, in the device's order ---------------------------------------------------------------------------------------------
def column_means(X):
    """(c_n, n0): the mean of the present values of every column - one ascending float64 chain from +0.0, divided by their number; 0
    for an empty column."""
    X = np.asarray(X)
    s = np.zeros(X.shape[1], dtype=np.float64)
    n0 = np.zeros(X.shape[1], dtype=np.int64)
    for row in X:
        p = ~np.isnan(row)
        s = np.where(p, s + np.where(p, row, 0).astype(np.float64), s)
        n0 += p
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n0 > 0, s / n0, 0.0), n0


def centred(X):
    """(x', present, c_n, n0): x' = x - c_n in float64 (0 at the missing entries) - the values every chain of the device runs over"""
    cn, n0 = column_means(X)
    present = ~np.isnan(X)
    xp = np.where(present, np.where(present, X, 0).astype(np.float64) - cn[None, :], 0.0)
    return xp, present, cn, n0


def moments(xp, present, yc, lags, real=np.float64):
    """The sums of the definition in the arithmetic `real`, each an ascending chain in s from +0: per (lag, column) the pair count n,
    Sx, Sxx and - for the bound - sum |x'|; per (lag, column, series) Sy, Syy, Sxy, sum |y'| and sum |x' y'|."""
    T, N = xp.shape
    q = yc.shape[1]
    L = len(lags)
    x, y = xp.astype(real), yc.astype(real)
    out = {k: np.zeros((L, N), dtype=real) for k in ("sx", "sxx", "ax")}
    out.update({k: np.zeros((L, N, q), dtype=real) for k in ("sy", "syy", "sxy", "ay", "axy")})
    out["n"] = np.zeros((L, N), dtype=np.int64)
    for g, lag in enumerate(lags):
        for s in range(max(0, -lag), min(T, T - lag)):
            p = present[s + lag]
            xs = np.where(p, x[s + lag], 0)
            ys = np.where(p[:, None], y[s][None, :], 0)
            out["n"][g] += p
            out["sx"][g] += xs
            out["sxx"][g] += xs * xs
            out["ax"][g] += np.abs(xs)
            out["sy"][g] += ys
            out["syy"][g] += ys * ys
            out["ay"][g] += np.abs(ys)
            out["sxy"][g] += xs[:, None] * ys
            out["axy"][g] += np.abs(xs[:, None] * ys)
    return out


def lag1_field(xp, present, n0, real=np.float64):
    """rho_x of every column in `real`: [sum_P x'_t x'_{t+1} / |P|] / [sum_present x'^2 / n0], 0 where |P| = 0 or the denominator is
    not positive, clamped to [-1, 1]."""
    x = xp.astype(real)
    N = x.shape[1]
    sq, sp = np.zeros(N, dtype=real), np.zeros(N, dtype=real)
    npairs = np.zeros(N, dtype=np.int64)
    for t in range(x.shape[0]):
        sq += x[t] * x[t]
        if t > 0:
            both = present[t] & present[t - 1]
            sp += np.where(both, x[t - 1] * x[t], 0)
            npairs += both
    with np.errstate(invalid="ignore", divide="ignore"):
        den = sq / n0.astype(real)
        rho = np.where((npairs > 0) & (den > 0), (sp / np.maximum(npairs, 1).astype(real)) / den, 0)
    return np.clip(rho, -1, 1).astype(real)


def lag1_index(yc, real=np.float64):
    """rho_y in `real`: the same expression on the gap-free centred index"""
    T = yc.shape[0]
    return lag1_field(yc.astype(np.float64), np.ones(yc.shape, dtype=bool), np.full(yc.shape[1], T), real)


def finish(m, min_pairs, rho_x=None, rho_y=None):
    """From the moments (in their own arithmetic): the centred moments, the live rule, r (clamped), slope, dof and n f."""
    real = m["sx"].dtype.type
    n = m["n"]
    with np.errstate(invalid="ignore", divide="ignore"):
        dn = n.astype(real)
        cxx = m["sxx"] - m["sx"] * m["sx"] / dn
        cyy = m["syy"] - m["sy"] * m["sy"] / dn[..., None]
        cxy = m["sxy"] - m["sx"][..., None] * m["sy"] / dn[..., None]
        live = (n >= min_pairs)[..., None] & (cxx > real(LIVE) * m["sxx"])[..., None] & (cyy > real(LIVE) * m["syy"])
        r = cxy / np.sqrt(cxx[..., None] * cyy)
        r = np.where(r > 1, real(1), np.where(r < -1, real(-1), r))
        slope = cxy / cyy
        if rho_x is None:
            nf = np.broadcast_to(dn[..., None], live.shape).copy()
        else:
            rho = rho_x.astype(real)[None, :, None] * rho_y.astype(real)[None, None, :]
            f = np.where(rho <= 0, real(1), (1 - rho) / (1 + rho))
            nf = dn[..., None] * f
        dof = np.minimum(np.broadcast_to(n[..., None], live.shape), np.floor(np.where(live, nf, 0)).astype(np.int64))
    dof = np.where(live, dof, 0)
    return dict(cxx=cxx, cyy=cyy, cxy=cxy, live=live, r=np.where(live, r, np.nan), slope=np.where(live, slope, np.nan), dof=dof, nf=nf)


def pvalue(r, dof):
    """`pearson_two_sided_p(r, dof / 2 - 1, pvalue_log_norm(dof))` of csrc/kernels.h in numpy float64, every entry with its own dof:
    the continued fraction of I_x(a, a) by the modified Lentz recurrence, an entry leaving the loop where the kernel's lane does; NaN
    where r is NaN or dof < 3."""
    from xmca_amd import _hip
    r = np.asarray(r, dtype=np.float64)
    dof = np.asarray(dof)
    out = np.full(r.shape, np.nan)
    sel = (dof >= 3) & ~np.isnan(r)
    if not sel.any():
        return out
    table = {int(k): _hip.pvalue_log_norm(int(k)) for k in np.unique(dof[sel])}
    k = dof[sel]
    a = 0.5 * k - 1.0
    log_norm = np.array([table[int(v)] for v in k])
    x = 0.5 * (1.0 - np.abs(r[sel]))
    zero = ~(x > 0.0)
    x = np.where(zero, 0.25, x)          # (a placeholder: those entries are 0 in the end)
    tiny, eps = 1e-300, 4.0 * 2.220446049250313e-16

    def guard(v):
        return np.where(np.abs(v) < tiny, tiny, v)
    a2 = a + a
    c = np.ones_like(x)
    d = 1.0 / guard(1.0 - a2 * x / (a + 1.0))
    h = d.copy()
    active = np.ones(x.shape, dtype=bool)
    for m in range(1, 1025):
        am = a + 2.0 * m
        t = m * (a - m) * x / ((am - 1.0) * am)
        d1 = 1.0 / guard(1.0 + t * d)
        c1 = guard(1.0 + t / c)
        h1 = h * (d1 * c1)
        t = -(a + m) * (a2 + m) * x / (am * (am + 1.0))
        d2 = 1.0 / guard(1.0 + t * d1)
        c2 = guard(1.0 + t / c1)
        delta = d2 * c2
        h2 = h1 * delta
        d, c, h = np.where(active, d2, d), np.where(active, c2, c), np.where(active, h2, h)
        active = active & ~(np.abs(delta - 1.0) <= eps)
        if not active.any():
            break
    with np.errstate(under="ignore"):
        p = 2.0 * np.exp(a * (np.log(x) + np.log1p(-x)) + log_norm) * h
    out[sel] = np.where(zero, 0.0, np.minimum(p, 1.0))
    return out


def restate(X, index, lags, min_pairs=8, dof="n", real=np.float64, with_p=True):
    """`lead_lag_maps` of a T x N field in numpy, in the arithmetic `real` (float64: the restatement, r and slope rounded once to the
    dtype of X and p computed from the rounded r; longdouble: the truth, nothing rounded and no p)."""
    X = np.asarray(X)
    y = np.asarray(index, dtype=np.float64)
    y = y[:, None] if y.ndim == 1 else y
    yc, _ = lagged.center_index(y)
    xp, present, cn, n0 = centred(X)
    m = moments(xp, present, yc, list(lags), real)
    rho_x = rho_y = None
    if dof == "bretherton":
        rho_x, rho_y = lag1_field(xp, present, n0, real), lag1_index(yc, real)
    f = finish(m, min_pairs, rho_x, rho_y)
    out = dict(pairs=m["n"], dof=f["dof"], live=f["live"], nf=f["nf"], moments=m, centred=f, lag1=rho_x, rho_y=rho_y)
    if real is np.float64:
        out["r"], out["slope"] = f["r"].astype(X.dtype), f["slope"].astype(X.dtype)
        if with_p:
            out["p"] = pvalue(out["r"].astype(np.float64), f["dof"])
    else:
        out["r"], out["slope"] = f["r"], f["slope"]
    return out


def bounds(truth, dtype):
    """The per-entry allowance of r and slope from the truth's own sums, in longdouble - nothing of it measured.  With u = 2^-53 and n
    the pair count: d(Cab) = 2 (n + 6) u [sum |a' b'| + sum |a'| sum |b'| / n],
    dr = dCxy / sqrt(Cxx Cyy) + (|r| / 2) (dCxx / Cxx + dCyy / Cyy) + 2 u |r|,  dslope = dCxy / Cyy + |slope| dCyy / Cyy + 2 u |slope|;
    the allowance is 2 d, plus half a float32 spacing at the value for a float32 field (the one rounding)."""
    m, f = truth["moments"], truth["centred"]
    with np.errstate(invalid="ignore", divide="ignore"):
        n = m["n"].astype(np.longdouble)
        k = 2 * (n + 6) * np.longdouble(U)
        dxx = k * (m["sxx"] + m["ax"] * m["ax"] / n)
        dyy = k[..., None] * (m["syy"] + m["ay"] * m["ay"] / n[..., None])
        dxy = k[..., None] * (m["axy"] + m["ax"][..., None] * m["ay"] / n[..., None])
        r, slope = truth["r"], truth["slope"]
        dr = dxy / np.sqrt(f["cxx"][..., None] * f["cyy"]) + np.abs(r) / 2 * (dxx / f["cxx"])[..., None] + np.abs(r) / 2 * dyy / f["cyy"] \
            + 2 * U * np.abs(r)
        ds = dxy / f["cyy"] + np.abs(slope) * dyy / f["cyy"] + 2 * U * np.abs(slope)
        br, bs = 2 * dr, 2 * ds
        if dtype == "float32":
            live = truth["live"]
            br = br + np.where(live, 0.5 * np.spacing(np.abs(np.where(live, r, 0)).astype(np.float32)).astype(np.longdouble), 0)
            bs = bs + np.where(live, 0.5 * np.spacing(np.abs(np.where(live, slope, 0)).astype(np.float32)).astype(np.longdouble), 0)
    return br, bs


@functools.lru_cache(maxsize=None)
def reference(name, dtype, dof):
    """(restatement, truth, bound of r, bound of slope) of a case; shared by the tests and left unchanged by them"""
    case = case_by_name(name)
    X, y = case_field(case, dtype), case_index(case)
    rest = restate(X, y, case[4], case[6], dof)
    truth = restate(X, y, case[4], case[6], dof, real=np.longdouble)
    br, bs = bounds(truth, dtype)
    return rest, truth, br, bs


def worst_ratio(got, want, bound, live):
    """the largest error / bound over the live entries (0 when there is none)"""
    if not live.any():
        return 0.0
    err = np.abs(np.asarray(got).astype(np.longdouble)[live] - want[live])
    return float(np.max(err / bound[live]))


# ---- the index rules of the moment kernel, in Python -----------------------------------------------------------------------------------
def kernel_walk(X, cn, yc, lags, cols=C, rows=R, groups=GROUPS):
    """The walk of `lead_lag_moments_kernel`, workgroup by workgroup with its bounds asserted: (n, Sx, Sxx, Sy, Syy, Sxy) in float64 with a
    multiply and an add where the kernel has an fma - the bits of `moments` if the index rules are right."""
    T, N = X.shape
    q = yc.shape[1]
    G = groups[q - 1]
    L = len(lags)
    n_out = np.full((L, N), -1, dtype=np.int64)
    sx, sxx = np.full((L, N), np.nan), np.full((L, N), np.nan)
    sy, syy, sxy = (np.full((L, N, q), np.nan) for _ in range(3))
    for by in range(-(-L // G)):
        for bx in range(-(-N // cols)):
            lane = np.arange(bx * cols, bx * cols + cols)
            lane = lane[lane < N]                                   # (a lane past the last column returns before any load)
            g0 = by * G
            lag = []
            for g in range(G):
                at = g0 + g if g0 + g < L else L - 1
                assert 0 <= at < L
                lag.append(lags[at])
            cnt = np.zeros((G, lane.size), dtype=np.int64)
            a_sx, a_sxx = np.zeros((G, lane.size)), np.zeros((G, lane.size))
            a_sy, a_syy, a_sxy = (np.zeros((G, lane.size, q)) for _ in range(3))
            for t0 in range(0, T, rows):
                v = []
                for i in range(rows):
                    t = t0 + i if t0 + i < T else T - 1
                    assert 0 <= t < T and lane.size and lane.max() < N
                    v.append(X[t, lane])
                for i in range(rows):
                    t = t0 + i
                    present = (t < T) & ~np.isnan(v[i])
                    x = np.where(present, np.where(present, v[i], 0).astype(np.float64) - cn[lane], 0.0)
                    for g in range(G):
                        s = t - lag[g]
                        inside = 0 <= s < T
                        sc = 0 if s < 0 else (s if s < T else T - 1)
                        assert 0 <= sc < T
                        pair = present & inside
                        xs = x if inside else np.zeros_like(x)
                        one = np.where(pair, 1.0, 0.0)
                        cnt[g] += pair
                        a_sx[g] = a_sx[g] + xs
                        a_sxx[g] = a_sxx[g] + xs * xs
                        yrow = yc[sc]
                        yp = one[:, None] * yrow[None, :]
                        a_sy[g] = a_sy[g] + yp
                        a_syy[g] = a_syy[g] + yp * yrow[None, :]
                        a_sxy[g] = a_sxy[g] + xs[:, None] * yrow[None, :]
            for g in range(G):
                if g0 + g < L:
                    assert (n_out[g0 + g, lane] == -1).all()          # every (lag, column) is written once
                    n_out[g0 + g, lane] = cnt[g]
                    sx[g0 + g, lane], sxx[g0 + g, lane] = a_sx[g], a_sxx[g]
                    sy[g0 + g, lane], syy[g0 + g, lane], sxy[g0 + g, lane] = a_sy[g], a_syy[g], a_sxy[g]
    assert (n_out >= 0).all()
    return n_out, sx, sxx, sy, syy, sxy
