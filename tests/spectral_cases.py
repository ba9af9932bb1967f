"""What the tests of `xmca_amd.spectral.spectral_maps` compare with: a numpy restatement of the definition in the
device's summation order - the same ascending chains in float64 (a multiply and an add where the device uses one fma), the same
restatement in longdouble with unrounded tables as the truth - the per-entry error bound, a Python restatement of the index rules of
the two kernels that run `spectral_segment` with their bounds asserted, and the deterministic, seeded cases.

The cases are placed around the tile of the segment kernel (`_hip.spectral_tile()`; a test asserts that they straddle the tile the
library reports): C = 256 columns of a workgroup, R = 8 rows of a piece, B(q) = 8, 8, 6, 4, 3 bins of a group.  T in
{L, L + step - 1, L + step, 3 L + 1}, L in {8, 9, 16, 64, 100} and once 4096, step in {L, L // 2, ceil(L / 4)} and a non-divisor,
N in {1, 255, 256, 257, 1025}, q in {0, 1, 2, 4}, bin lists of {1, B - 1, B, B + 1, 2 B + 1} entries - unsorted, with 0 and L // 2 -
three windows, both detrend modes and nine gap patterns."""
import functools

import numpy as np

from xmca_amd import lagged, spectral

C, R = 256, 8
GROUPS = (8, 8, 6, 4, 3)          # B(q), q = 0 .. 4
U = 2.0 ** -53
LIVE = 2.0 ** -40

# (name, T, N, q, L, step, window, detrend, bins, gap pattern, min_segments)
CASES = [
    ("tiny", 8, 1, 0, 8, 8, "boxcar", None, (0,), "none", 1),                                                          # 1 bin; T = L
    ("odd", 11, 255, 1, 9, 3, "hann", "mean", (4, 0, 2, 1, 3), "scattered", 1),                                        # T = L + step - 1
    ("l8", 25, 257, 1, 8, 2, "hann", "mean", (3, 0, 4, 1, 2), "scattered", 2),                                         # T = 3 L + 1
    ("two", 24, 256, 2, 16, 8, "hann", "mean", (8, 0, 3, 5, 1), "step", 1),                                            # B - 1; T = L + step
    ("three", 49, 257, 4, 16, 4, "custom", "mean", (0, 8, 2), "scattered", 2),                                         # B
    ("wide", 193, 1025, 0, 64, 32, "hann", "mean", (32, 0, 5, 17, 1, 9, 30, 2, 11, 31, 7, 3, 21, 13, 4, 8, 16), "column", 2),   # 2 B + 1
    ("nondiv", 301, 257, 1, 100, 37, "custom", None, (50, 0, 7, 3, 49, 12, 1, 25, 33), "overlap", 2),                  # B + 1
    ("single", 193, 255, 2, 64, 16, "hann", "mean", (0, 32, 1, 2, 3, 5, 8, 13, 21, 31, 4, 6, 10), "single", 3),        # 2 B + 1
    ("constant", 193, 256, 4, 64, 64, "boxcar", "mean", (1, 0, 32, 7, 9, 20, 3), "constant", 2),                       # 2 B + 1
    ("q1-group", 96, 1, 1, 64, 32, "hann", None, (32, 0, 4, 9, 2, 16, 1, 25), "none", 1),                              # B
    ("q0-group", 301, 256, 0, 100, 50, "boxcar", "mean", (0, 50, 10, 3, 1, 27, 49, 5), "few", 3),                      # B
    ("q0-minus", 95, 257, 0, 64, 32, "custom", "mean", (6, 0, 32, 1, 15, 2, 31), "none", 1),                           # B - 1
    ("q4-plus", 49, 255, 4, 16, 8, "hann", "mean", (8, 1, 0, 5), "step", 2),                                           # B + 1
    ("q4-minus", 100, 1, 4, 100, 100, "custom", None, (50, 0), "none", 1),                                             # B - 1
    ("q2-group", 49, 1025, 2, 16, 16, "boxcar", None, (8, 0, 1, 2, 5, 7), "scattered", 1),                             # B
    ("q2-plus", 96, 256, 2, 64, 32, "hann", "mean", (0, 32, 3, 1, 12, 2, 30), "overlap", 2),                           # B + 1
    ("big", 5120, 3, 1, 4096, 1024, "hann", "mean", (0, 2048, 1, 777, 2047), "single-big", 1),                         # L = 4096
]
PATTERNS = ("none", "scattered", "step", "column", "single", "few", "overlap", "constant", "single-big")
DTYPES = ("float64", "float32")
MAPS = ("power", "index_power", "cospectrum", "quadrature", "coherence", "phase", "gain")
CROSS = MAPS[1:] + ("p",)


def case_name(case):
    return case[0]


def case_by_name(name):
    return next(c for c in CASES if c[0] == name)


def segments_of(T, L, step):
    return (T - L) // step + 1


def case_window(case):
    """The float64 weights of a case; 'custom' is an asymmetric window of its own."""
    L, window = case[4], case[6]
    if window == "custom":
        j = np.arange(L)
        return 0.2 + ((7 * j) % 5) / 5.0 + j / L
    return spectral.welch_window(window, L)


def case_index(case):
    """The (T, max(q, 1)) index of a case: AR(1) series with an offset (so that the centring matters); the first one is in the field."""
    name, T, N, q = case[:4]
    q = max(q, 1)
    rng = np.random.default_rng(31 * T + 7 * q + 1)
    e = rng.standard_normal((T, q))
    y = np.empty((T, q))
    y[0] = e[0]
    for t in range(1, T):
        y[t] = 0.6 * y[t - 1] + 0.8 * e[t]
    return y * (1.0 + 0.5 * np.arange(q)) + 5.0 - np.arange(q)


def case_field(case, dtype="float64"):
    """The T x N field of a case in `dtype`: 10 + noise + the first index delayed by two steps in every column (the planted common
    signal that keeps |C| away from 0), with the gaps of its pattern as NaN."""
    name, T, N, q, L, step, window, detrend, bins, pattern, ms = case
    K = segments_of(T, L, step)
    rng = np.random.default_rng(7 * T + 13 * N + q)
    y0 = case_index(case)[:, 0]
    X = 10.0 + rng.standard_normal((T, N))
    X[2:] += (0.8 + 0.4 * np.cos(np.arange(N)))[None, :] * (y0[:-2, None] - y0.mean())
    if pattern == "scattered":                 # 10 % of the entries
        X[rng.random((T, N)) < 0.10] = np.nan
    elif pattern == "step":                    # a wholly missing time step: in the first segment only (K = 2), or in two inner ones
        X[2 if K == 2 else T // 2 - 4] = np.nan
    elif pattern == "column":                  # a wholly missing column (K_n = 0), and a single gap in the last one
        X[:, N // 3] = np.nan
        X[T // 2 + 3, -1] = np.nan
    elif pattern in ("single", "single-big"):  # a column with exactly one present segment; one with exactly min_segments - 1
        spans = [(1, 2 * step if K > 2 else step, L)] + ([(N - 2, step, L + (ms - 2) * step)] if pattern == "single" else [])
        for n, first, rows in spans:
            keep = X[first:first + rows, n].copy()
            X[:, n] = np.nan
            X[first:first + rows, n] = keep
    elif pattern == "few":                     # a column with exactly min_segments - 1 present segments, one with exactly min_segments
        for n, count in ((3, ms - 1), (N - 2, ms)):
            rows = L + (count - 1) * step
            keep = X[step:step + rows, n].copy()
            X[:, n] = np.nan
            X[step:step + rows, n] = keep
    elif pattern == "overlap":                 # gaps only in rows that segments 0 and 1 share, in every third column, staggered
        for n in range(0, N, 3):
            X[step + (5 * n) % (L - step), n] = np.nan
    elif pattern == "constant":                # exactly constant columns with a dyadic value, one of them with gaps in segment 0 only
        X[:, 5] = 12.5
        X[:, N - 1] = -0.375
        X[:L, N - 1][rng.random(L) < 0.2] = np.nan
    else:
        assert pattern == "none", pattern
    return X.astype(dtype)


# ---- the definition, in the device's order ---------------------------------------------------------------------------------------------
def column_means(X):
    """(c_n, n0): the mean of the present values of every column - one ascending float64 chain from +0.0 divided by their number; 0
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


def centred(X, demean):
    """(x', present): x' = x - c_n in float64 (c_n = 0 without detrending; 0 at the missing entries) - the values every chain runs over"""
    X = np.asarray(X)
    present = ~np.isnan(X)
    cn = column_means(X)[0] if demean else np.zeros(X.shape[1])
    return np.where(present, np.where(present, X, 0).astype(np.float64) - cn[None, :], 0.0), present, cn


def tables(w, L, bins, real=np.float64):
    """(tw (L, 2), W (F, 2), sum w^2) in `real`: float64 - what the device gets, evaluated in extended precision and rounded once;
    longdouble - unrounded."""
    c, ms = spectral._twiddle_extended(L)
    tw = np.stack([c, ms], axis=1)
    if real is np.float64:
        tw = tw.astype(np.float64)
    wl = np.asarray(w, dtype=np.float64).astype(np.longdouble)
    twl = tw.astype(np.longdouble)
    w2 = np.longdouble(0)
    for v in wl:
        w2 = w2 + v * v
    W = np.zeros((len(bins), 2), dtype=np.longdouble)
    for f, k in enumerate(bins):
        idx = 0
        for j in range(L):
            W[f] = W[f] + wl[j] * twl[idx]
            idx += int(k)
            if idx >= L:
                idx -= L
    return tw.astype(real), W.astype(real), real(w2)


def segment_spectra(x, present, w, tab, bins, L, step, demean, real=np.float64):
    """Every segment of every column of the plane x' in the arithmetic `real`: Z (K, N, F) as (zr, zi), the energy e (K, N), the
    present flag (K, N), and - for the bound - a = sum_j |w_j x'_j| and b = sum_j |x'_j| / L (K, N).  The chains run in ascending j
    from +0, the table offsets (k j) mod L are stepped as the kernel steps them."""
    tw, W, w2 = tab
    T, N = x.shape
    K, F = segments_of(T, L, step), len(bins)
    kb = np.asarray(bins, dtype=np.int64)
    x, wr = x.astype(real), np.asarray(w, dtype=np.float64).astype(real)
    zr, zi = np.zeros((K, N, F), dtype=real), np.zeros((K, N, F), dtype=real)
    e, a, b = (np.zeros((K, N), dtype=real) for _ in range(3))
    pres = np.zeros((K, N), dtype=bool)
    for m in range(K):
        seg = x[m * step:m * step + L]
        pres[m] = present[m * step:m * step + L].all(axis=0)
        re, im = np.zeros((N, F), dtype=real), np.zeros((N, F), dtype=real)
        s, p1, p2, sa, sb = (np.zeros(N, dtype=real) for _ in range(5))
        idx = np.zeros(F, dtype=np.int64)
        for j in range(L):
            wx = wr[j] * seg[j]
            s = s + seg[j]
            p1 = p1 + wr[j] * wx
            p2 = p2 + wx * wx
            sa = sa + np.abs(wx)
            sb = sb + np.abs(seg[j])
            re = re + wx[:, None] * tw[idx, 0][None, :]
            im = im + wx[:, None] * tw[idx, 1][None, :]
            assert np.array_equal(idx, (kb * j) % L)
            idx = idx + kb
            idx = np.where(idx >= L, idx - L, idx)
        mu = s / real(L) if demean else np.zeros(N, dtype=real)
        zr[m] = re - mu[:, None] * W[None, :, 0]
        zi[m] = im - mu[:, None] * W[None, :, 1]
        e[m] = p2 - mu * (real(2) * p1 - mu * w2)
        a[m], b[m] = sa, (sb / real(L) if demean else np.zeros(N, dtype=real))
    return dict(zr=zr, zi=zi, e=e, present=pres, a=a, b=b)


def accumulate(sx, sy, real=np.float64):
    """The sums over the present segments of every column in ascending m, in `real`: K_n, Sxx (N, F), R (N) and - with an index -
    Syy, Re C, Im C (N, F, q), Ry (N, q); for the bound sum |Y| |Z| as well."""
    K, N, F = sx["zr"].shape
    kn = np.zeros(N, dtype=np.int64)
    sxx, r = np.zeros((N, F), dtype=real), np.zeros(N, dtype=real)
    q = 0 if sy is None else sy["zr"].shape[1]
    syy, cre, cim, ayz = (np.zeros((N, F, q), dtype=real) for _ in range(4))
    ry = np.zeros((N, q), dtype=real)
    for m in range(K):
        p = sx["present"][m]
        zr, zi = sx["zr"][m], sx["zi"][m]
        kn += p
        sxx = np.where(p[:, None], sxx + (zr * zr + zi * zi), sxx)
        r = np.where(p, r + sx["e"][m], r)
        if q:
            yr, yi = sy["zr"][m].T[None, :, :], sy["zi"][m].T[None, :, :]          # (1, F, q)
            pp = p[:, None, None]
            syy = np.where(pp, syy + (yr * yr + yi * yi), syy)
            cre = np.where(pp, cre + (yr * zr[:, :, None] + yi * zi[:, :, None]), cre)
            cim = np.where(pp, cim + (yr * zi[:, :, None] - yi * zr[:, :, None]), cim)
            ayz = np.where(pp, ayz + np.sqrt(yr * yr + yi * yi) * np.sqrt(zr * zr + zi * zi)[:, :, None], ayz)
            ry = np.where(p[:, None], ry + sy["e"][m][None, :], ry)
    return dict(kn=kn, sxx=sxx, r=r, syy=syy, cre=cre, cim=cim, ry=ry, ayz=ayz)


def finish(acc, bins, L, fs, w2, ke, min_segments):
    """The maps from the sums, in their own arithmetic, (F, N) and (F, N, q): nothing rounded to the dtype of the field yet."""
    real = acc["sxx"].dtype.type
    kn = acc["kn"]
    kb = np.asarray(bins)
    side = np.where((kb == 0) | (2 * kb == L), real(1), real(2))
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = side[:, None] / (real(fs) * w2 * kn.astype(real))[None, :]          # (F, N)
        col_live = (kn >= min_segments) & (kn >= 1)
        sxx, syy, cre, cim = acc["sxx"].T, np.moveaxis(acc["syy"], 1, 0), np.moveaxis(acc["cre"], 1, 0), np.moveaxis(acc["cim"], 1, 0)
        nan = real(np.nan)
        out = dict(power=np.where(col_live[None, :], scale * sxx, nan), segments=kn, col_live=col_live)
        q = syy.shape[-1]
        if not q:
            return out
        cl = col_live[None, :, None]
        out["index_power"] = np.where(cl, scale[..., None] * syy, nan)
        out["cospectrum"] = np.where(cl, scale[..., None] * cre, nan)
        out["quadrature"] = np.where(cl, scale[..., None] * cim, nan)
        live = cl & (kn >= 2)[None, :, None] & (sxx > real(LIVE) * acc["r"][None, :])[..., None] & (syy > real(LIVE) * acc["ry"][None, :, :])
        c2 = cre * cre + cim * cim
        coh = c2 / (sxx[..., None] * syy)
        coh = np.where(coh > 1, real(1), np.where(coh < 0, real(0), coh))
        out["coherence"] = np.where(live, coh, nan)
        out["phase"] = np.where(live, np.arctan2(cim, cre), nan)
        out["gain"] = np.where(live, np.sqrt(c2) / syy, nan)
        out["live"] = live
        out["ke"] = np.broadcast_to(np.asarray(ke)[kn][None, :, None], live.shape)
    return out


def pvalue(coh, ke, real=np.longdouble):
    """(1 - coh)^(Ke - 1) as exp((Ke - 1) log1p(-coh)) in `real`, 0 where coh is 1, NaN where coh is"""
    c, k = np.asarray(coh).astype(real), np.asarray(ke).astype(real)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(np.isnan(c), real(np.nan), np.where(c >= 1, real(0), np.exp((k - 1) * np.log1p(-np.where(c >= 1, 0, c)))))


def restate(X, index, L, step=None, window="hann", detrend="mean", bins=None, fs=1.0, min_segments=2, real=np.float64):
    """`spectral_maps` of a T x N field in numpy, in the arithmetic `real` (float64: the restatement, every map rounded once to the
    dtype of X and p computed from the rounded coherence; longdouble: the truth, unrounded tables, nothing rounded, no p)."""
    X = np.asarray(X)
    T = X.shape[0]
    step = L // 2 if step is None else step
    w = window if isinstance(window, np.ndarray) else spectral.welch_window(window, L)
    bins = list(range(L // 2 + 1)) if bins is None else [int(k) for k in bins]
    demean = detrend == "mean"
    xp, present, cn = centred(X, demean)
    tab = tables(w, L, bins, real)
    sx = segment_spectra(xp, present, w, tab, bins, L, step, demean, real)
    sy = None
    if index is not None:
        y = np.asarray(index, dtype=np.float64)
        yc, _ = lagged.center_index(y[:, None] if y.ndim == 1 else y)
        sy = segment_spectra(yc, np.ones(yc.shape, dtype=bool), w, tab, bins, L, step, demean, real)
    acc = accumulate(sx, sy, real)
    K = segments_of(T, L, step)
    ke = spectral.effective_segments(np.arange(K + 1), w, step)
    out = finish(acc, bins, L, fs, tab[2], ke, min_segments)
    out.update(sums=acc, sx=sx, sy=sy, tables=tab, cn=cn, bins=bins)
    if real is np.float64:
        for key in MAPS:
            if key in out:
                out[key] = out[key].astype(X.dtype)
        if sy is not None:
            out["p"] = pvalue(out["coherence"].astype(np.float64), out["ke"], np.float64)
    return out


def bounds(truth, L, fs, dtype):
    """The per-entry allowance of every map from the truth's own sums, in longdouble - nothing of it measured.  With u = 2^-53:
    a chain of L fmas over products with a rounded table entry errs by at most (L + 2) u sum |w x'|; mu = s / L by (L + 1) u sum |x'| / L,
    its product with the rounded W_k by two more: each part of Z by dz = (L + 4) u (a + b |W_k|), a = sum |w x'|, b = sum |x'| / L (0
    without detrending), so Z as a complex number by ez = sqrt(2) dz; the same on the index gives ey.  Over the K_n present segments
      dSxx = sum_m (2 |Z| ez + ez^2) + (K_n + 3) u Sxx,   dSyy likewise,
      dC   = sqrt(2) [sum_m (|Y| ez + |Z| ey + ey ez) + (2 K_n + 3) u sum_m |Y| |Z|]   (C as a complex number),
    and with the five roundings of scale = side / (fs sum w^2 K_n) and of the product:
      d power = scale dSxx + 5 u power, d index_power likewise, d cospectrum = scale dC + 5 u |cospectrum|, d quadrature likewise,
      d coherence = 2 |C| dC / (Sxx Syy) + coherence (dSxx / Sxx + dSyy / Syy + 6 u),
      d gain = dC / Syy + gain (dSyy / Syy + 4 u),   d phase = dC / |C| + 4 pi u  (used only where |C| > 2^10 dC).
    The allowance is 2 d, plus half a float32 spacing at the value for a float32 field (the one rounding).  Returns the dict of
    allowances and `phase_ok`, the entries whose phase is compared."""
    ld = np.longdouble
    u = ld(U)
    sx, sy, acc = truth["sx"], truth["sy"], truth["sums"]
    W = truth["tables"][1]
    Wabs = np.sqrt(W[:, 0] ** 2 + W[:, 1] ** 2)                                   # (F,)
    kn = acc["kn"].astype(ld)
    kb = np.asarray(truth["bins"])
    side = np.where((kb == 0) | (2 * kb == L), ld(1), ld(2))
    rt2 = np.sqrt(ld(2))

    def err(s):          # (K, N', F): ez of every segment
        return rt2 * (L + 4) * u * (s["a"][:, :, None] + s["b"][:, :, None] * Wabs[None, None, :])
    ez = err(sx)
    zabs = np.sqrt(sx["zr"] ** 2 + sx["zi"] ** 2)
    pres = sx["present"][:, :, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        dsxx = np.where(pres, 2 * zabs * ez + ez * ez, 0).sum(axis=0) + (kn[:, None] + 3) * u * acc["sxx"]          # (N, F)
        scale = side[:, None] / (ld(fs) * truth["tables"][2] * kn)[None, :]                                           # (F, N)
        out = {"power": scale * dsxx.T + 5 * u * np.abs(truth["power"])}
        phase_ok = None
        if sy is not None:
            ey = err(sy)                                                                                              # (K, q, F)
            yabs = np.sqrt(sy["zr"] ** 2 + sy["zi"] ** 2)
            yabs_, ey_ = np.moveaxis(yabs, 1, 2)[:, None, :, :], np.moveaxis(ey, 1, 2)[:, None, :, :]                 # (K, 1, F, q)
            pp = pres[..., None]
            dsyy = np.where(pp, 2 * yabs_ * ey_ + ey_ * ey_, 0).sum(axis=0) + (kn[:, None, None] + 3) * u * acc["syy"]            # (N, F, q)
            dc = rt2 * (np.where(pp, yabs_ * ez[..., None] + zabs[..., None] * ey_ + ey_ * ez[..., None], 0).sum(axis=0)
                        + (2 * kn[:, None, None] + 3) * u * acc["ayz"])
            dsxx_, dsyy_, dc_ = dsxx.T[..., None], np.moveaxis(dsyy, 1, 0), np.moveaxis(dc, 1, 0)                     # (F, N, .)
            sxx_, syy_ = acc["sxx"].T[..., None], np.moveaxis(acc["syy"], 1, 0)
            cabs = np.sqrt(np.moveaxis(acc["cre"], 1, 0) ** 2 + np.moveaxis(acc["cim"], 1, 0) ** 2)
            sc = scale[..., None]
            out["index_power"] = sc * dsyy_ + 5 * u * np.abs(truth["index_power"])
            out["cospectrum"] = sc * dc_ + 5 * u * np.abs(truth["cospectrum"])
            out["quadrature"] = sc * dc_ + 5 * u * np.abs(truth["quadrature"])
            out["coherence"] = 2 * cabs * dc_ / (sxx_ * syy_) + truth["coherence"] * (dsxx_ / sxx_ + dsyy_ / syy_ + 6 * u)
            out["gain"] = dc_ / syy_ + truth["gain"] * (dsyy_ / syy_ + 4 * u)
            out["phase"] = dc_ / cabs + 4 * ld(np.pi) * u
            phase_ok = truth["live"] & (cabs > ld(2.0) ** 10 * dc_)
        for key in out:
            out[key] = 2 * out[key]
            if dtype == "float32":
                val = np.abs(np.where(np.isnan(truth[key]), 0, truth[key])).astype(np.float32)
                out[key] = out[key] + 0.5 * np.spacing(val).astype(ld)
    return out, phase_ok


def case_call(case, dtype="float64"):
    """(X, index or None, keyword arguments) of a case, as `spectral_maps` and `restate` take them"""
    name, T, N, q, L, step, window, detrend, bins, pattern, ms = case
    index = case_index(case)[:, :q] if q else None
    win = case_window(case) if window == "custom" else window
    return case_field(case, dtype), index, dict(step=step, window=win, detrend=detrend, bins=list(bins), fs=1.0, min_segments=ms)


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """(restatement, truth, allowances, phase_ok) of a case; shared by the tests and left unchanged by them"""
    case = case_by_name(name)
    X, index, kw = case_call(case, dtype)
    rest = restate(X, index, case[4], **kw)
    truth = restate(X, index, case[4], real=np.longdouble, **kw)
    allow, phase_ok = bounds(truth, case[4], kw["fs"], dtype)
    return rest, truth, allow, phase_ok


def live_of(res, key):
    """the entries of map `key` that hold a number"""
    if key == "power":
        return np.broadcast_to(res["col_live"][None, :], res["power"].shape)
    if key in ("index_power", "cospectrum", "quadrature"):
        return np.broadcast_to(res["col_live"][None, :, None], res[key].shape)
    return res["live"]


def angle_between(a, b):
    """|a - b| on the circle, in longdouble"""
    d = np.abs(np.asarray(a).astype(np.longdouble) - np.asarray(b).astype(np.longdouble))
    return np.minimum(d, 2 * np.longdouble(np.pi) - d)


def worst_ratio(got, want, bound, sel, circular=False):
    """the largest error / bound over the selected entries (0 when there is none; an exact value - an exactly constant column, whose
    bound is 0 as well - counts 0)"""
    if not sel.any():
        return 0.0
    err = angle_between(got, want) if circular else np.abs(np.asarray(got).astype(np.longdouble) - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(err[sel] == 0, 0, err[sel] / bound[sel])))


def p_ratio(p, coh, ke, live):
    """The worst |p - (1 - coh)^(Ke - 1)| / allowance at the device's own coherence, against longdouble.  t = (Ke - 1) log1p(-coh):
    log1p and the product err by at most 5 u |t|, exp by 4 u, the table entry Ke - 1 by 4 u more of |t| (Ke < 5 (Ke - 1) for Ke >= 1.25):
    |dp| / p <= 4 u + 9 u |ln p|; the allowance is twice that - 16 u (1 + |ln p|) p rounded up - plus 1e-300 for the subnormal range."""
    if not live.any():
        return 0.0
    want = pvalue(np.asarray(coh)[live], np.asarray(ke)[live])
    got = np.asarray(p)[live].astype(np.longdouble)
    with np.errstate(divide="ignore"):
        allow = 16 * np.longdouble(U) * (1 + np.abs(np.log(np.where(want > 0, want, 1)))) * want + np.longdouble(1e-300)
    return float(np.max(np.abs(got - want) / allow))


# ---- the index rules of the kernels, in Python ------------------------------------------------------------------------------------------
def _walk_segment(col, pres_col, c, row0, T, L, k, tw, w, rows):
    """`spectral_segment` of the lanes `col` (T x lanes, raw values), piece by piece with its bounds asserted"""
    B, lanes = len(k), col.shape[1]
    re, im = np.zeros((B, lanes)), np.zeros((B, lanes))
    s, p1, p2 = np.zeros(lanes), np.zeros(lanes), np.zeros(lanes)
    allp = np.ones(lanes, dtype=bool)
    idx = [0] * B
    for j0 in range(0, L, rows):
        v, ok = [], []
        for i in range(rows):
            j = j0 + i if j0 + i < L else L - 1
            assert 0 <= row0 + j < T
            v.append(col[row0 + j])
            ok.append(pres_col[row0 + j])
        for i in range(rows):
            inside = j0 + i < L
            j = j0 + i if inside else L - 1
            allp = allp & (ok[i] | (not inside))
            x = np.where(ok[i] & inside, np.where(ok[i], v[i], 0).astype(np.float64) - c, 0.0)
            wx = w[j] * x
            s = s + x
            p1 = p1 + w[j] * wx
            p2 = p2 + wx * wx
            for b in range(B):
                assert 0 <= idx[b] < L and (not inside or idx[b] == (k[b] * j) % L)
                re[b] = re[b] + wx * tw[idx[b], 0]
                im[b] = im[b] + wx * tw[idx[b], 1]
                nxt = idx[b] + k[b]
                idx[b] = nxt - L if nxt >= L else nxt
    return re, im, s, p1, p2, allp


def kernel_walk(X, cn, yc, w, tab, bins, L, step, demean, cols=C, rows=R, groups=GROUPS):
    """The walk of `spectral_index_kernel` and `spectral_segments_kernel`, workgroup by workgroup with their bounds asserted and every
    output written once: (K_n, Sxx, R, Syy, Re C, Im C, Ry) in float64 with a multiply and an add where the kernels have an fma - the
    bits of `accumulate` if the index rules are right."""
    tw, W, w2 = tab
    T, N = X.shape
    q = 0 if yc is None else yc.shape[1]
    B, F, K = groups[q], len(bins), segments_of(T, L, step)
    n_groups = -(-F // B)

    def group(by):
        f = [by * B + b if by * B + b < F else F - 1 for b in range(B)]
        assert all(0 <= v < F for v in f)
        return f, [int(bins[v]) for v in f]
    Y, ey = np.full((K, F, q, 2), np.nan), np.full((K, q), np.nan)
    if q:
        ones = np.ones(yc.shape, dtype=bool)
        for m in range(K):
            for by in range(n_groups):
                f, k = group(by)
                lane = np.minimum(np.arange(64), q - 1)
                assert m * step + L <= T
                re, im, s, p1, p2, allp = _walk_segment(yc[:, lane], ones[:, lane], 0.0, m * step, T, L, k, tw, w, rows)
                mu = s / np.float64(L) if demean else np.zeros(64)
                for b in range(B):
                    if by * B + b < F:
                        assert np.isnan(Y[m, f[b]]).all()
                        Y[m, f[b], :, 0] = (re[b] - mu * W[f[b], 0])[:q]
                        Y[m, f[b], :, 1] = (im[b] - mu * W[f[b], 1])[:q]
                if by == 0:
                    assert np.isnan(ey[m]).all()
                    ey[m] = (p2 - mu * (2.0 * p1 - mu * w2))[:q]
        assert not np.isnan(Y).any() and not np.isnan(ey).any()
    present = ~np.isnan(X)
    kn_out = np.full(N, -1, dtype=np.int64)
    sxx_out, r_out = np.full((N, F), np.nan), np.full(N, np.nan)
    syy_out, cre_out, cim_out = (np.full((N, F, q), np.nan) for _ in range(3))
    ry_out = np.full((N, q), np.nan)
    for by in range(n_groups):
        f, k = group(by)
        for bx in range(-(-N // cols)):
            lane_all = np.arange(bx * cols, bx * cols + cols)
            lane = np.minimum(lane_all, N - 1)                       # (a lane past the last column repeats it and writes nothing)
            write = lane_all < N
            assert lane.min() >= 0 and lane.max() < N
            sxx = np.zeros((B, cols))
            syy, cre, cim = (np.zeros((B, cols, q)) for _ in range(3))
            ry, r, kn = np.zeros((cols, q)), np.zeros(cols), np.zeros(cols, dtype=np.int64)
            for m in range(K):
                assert m * step + L <= T
                re, im, s, p1, p2, allp = _walk_segment(X[:, lane], present[:, lane], cn[lane], m * step, T, L, k, tw, w, rows)
                mu = s / np.float64(L) if demean else np.zeros(cols)
                one = np.where(allp, 1.0, 0.0)
                kn += allp
                r = r + np.where(allp, p2 - mu * (2.0 * p1 - mu * w2), 0.0)
                if q:
                    ry = ry + one[:, None] * ey[m][None, :]
                for b in range(B):
                    zr = np.where(allp, re[b] - mu * W[f[b], 0], 0.0)
                    zi = np.where(allp, im[b] - mu * W[f[b], 1], 0.0)
                    sxx[b] = sxx[b] + (zr * zr + zi * zi)
                    for j in range(q):
                        yr, yi = Y[m, f[b], j]
                        syy[b][:, j] = syy[b][:, j] + one * (yr * yr + yi * yi)
                        cre[b][:, j] = cre[b][:, j] + (yr * zr + yi * zi)
                        cim[b][:, j] = cim[b][:, j] + (yr * zi - yi * zr)
            at = lane_all[write]
            for b in range(B):
                if by * B + b < F:
                    assert np.isnan(sxx_out[at, f[b]]).all()          # every (bin, column) is written once
                    sxx_out[at, f[b]] = sxx[b][write]
                    syy_out[at, f[b]], cre_out[at, f[b]], cim_out[at, f[b]] = syy[b][write], cre[b][write], cim[b][write]
            if by == 0:
                assert (kn_out[at] == -1).all()
                kn_out[at], r_out[at], ry_out[at] = kn[write], r[write], ry[write]
    assert (kn_out >= 0).all() and not np.isnan(sxx_out).any() and not np.isnan(r_out).any()
    return kn_out, sxx_out, r_out, syy_out, cre_out, cim_out, ry_out
