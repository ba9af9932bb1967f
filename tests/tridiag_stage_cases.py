"""Cases, truth and float64 restatement for the two kernels behind the tridiagonal reduction: the Sturm
multisection `trd_bisect_kernel` (csrc/tridiag.h) and the twisted-factorisation vectors `trd_twisted_kernel` (csrc/tridiag_vec.h),
posed directly on a chosen (d, e) through `Handle.tridiag_eigenvalues` / `Handle.tridiag_vectors`.  No GPU code here.

  * truth of the eigenvalues: closed forms in numpy.longdouble where they exist (Toeplitz (2, -1), Clement, diagonal, identity),
    otherwise plain bisection on the division recurrence in longdouble, 90 halvings, with a pivmin guard (`truth_values`);
  * truth of a vector: the twisted factorisation in longdouble at the longdouble eigenvalue (`truth_vectors`), and
    sin(i k pi / (n + 1)) for Toeplitz (2, -1) (`toeplitz_vectors`);
  * restatement: the arithmetic of the two kernels in float64 numpy, separate multiply and add (`restate_values`,
    `restate_vectors`) - the reference the device is measured against.

Everything works on the SCALED matrix f (d, e), f the power of two of a solve (`scale_factor`: exact, so the truth of the scaled
matrix is f times the truth), and every error is in units of eps * bnorm, bnorm = max_i(|d_i| + |e_{i-1}| + |e_i|)."""
import functools

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
E2_FLOOR = 2.0 ** -200                    # floor of e^2 in trd_bisect_kernel
POINTS, PASSES = 16, 14                   # multisection: points per pass, passes
GAP_MIN = 1e-3                            # the angle is asked of eigenvalues whose gap exceeds GAP_MIN * bnorm


# ---- cases ------------------------------------------------------------------------------------------------------------------
class Case:
    """d (n), e (n - 1) in the caller's scale; closed: name of the closed form of the eigenvalues (None: bisection);
    vectors: whether the vector tests run on it; stride: the restatement of the VALUES is formed for every stride-th eigenvalue and
    the `stride` at either end only (1: all) - its worst error over a subset is at most the worst over all, so an allowance taken
    from it is never wider."""

    def __init__(self, name, d, e, closed=None, vectors=True, stride=1):
        self.name = name
        self.d = np.ascontiguousarray(d, dtype=np.float64)
        self.e = np.ascontiguousarray(e, dtype=np.float64)
        assert self.d.ndim == 1 and self.e.shape == (self.d.size - 1,)
        self.n = int(self.d.size)
        self.closed, self.vectors, self.stride = closed, vectors, stride
        self.f = scale_factor(self.d, self.e)
        self.ds, self.es = self.f * self.d, self.f * self.e
        self.bnorm = bnorm(self.ds, self.es)                    # of the scaled matrix

    def __repr__(self):
        return self.name


def scale_factor(d, e):
    """f = 2^-ex with f * max(|d|, |e|) in [0.5, 1); 1 for a zero matrix (trd_scale_kernel)."""
    m = max(float(np.max(np.abs(d))), float(np.max(np.abs(e))) if len(e) else 0.0)
    if not m > 0.0:
        return 1.0
    return float(np.ldexp(1.0, -int(np.frexp(m)[1])))


def bnorm(d, e):
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    r = np.abs(d).copy()
    r[:-1] += np.abs(e)
    r[1:] += np.abs(e)
    return float(np.max(r))


SIZES = (1, 2, 3, 8, 9, 15, 16, 17, 24, 25, 33, 63, 64, 65, 66, 127, 128, 129, 130, 257)


def _wilkinson_glued(blocks, glue):
    w = np.abs(np.arange(21) - 10.0)
    d = np.tile(w, blocks)
    e = np.ones(21 * blocks - 1)
    e[20::21] = glue
    return d, e


def toeplitz(n):
    return np.full(n, 2.0), np.full(n - 1, -1.0)


def clement(n):
    i = np.arange(1, n, dtype=np.float64)
    return np.zeros(n), np.sqrt(i * (n - i))


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for n in SIZES:
        rng = np.random.default_rng(1000 + n)
        out.append(Case("random_n%d" % n, rng.standard_normal(n), rng.standard_normal(n - 1)))
    for blocks, glue in ((6, 1e-3), (10, 1e-3), (6, 1e-7), (10, 1e-7)):
        out.append(Case("wilkinson21_x%d_glue%g" % (blocks, glue), *_wilkinson_glued(blocks, glue)))
    out.append(Case("toeplitz_n300", *toeplitz(300), closed="toeplitz"))
    out.append(Case("toeplitz_n4097", *toeplitz(4097), closed="toeplitz", vectors=False, stride=8))
    # (the integers are the eigenvalues of the matrix with EXACT square roots; e as rounded to double moves an eigenvalue by up to
    # 2 max |delta e| <= eps max e - of the size of the allowance.  The truth of the matrix handed in is the bisection; the host test
    # holds it to the integers within that perturbation bound)
    out.append(Case("clement_n200", *clement(200)))
    rng = np.random.default_rng(17)
    e = rng.standard_normal(119)
    e[16::17] = 0.0
    out.append(Case("random_n120_every_17th_e_zero", rng.standard_normal(120), e))
    d = np.logspace(0, -30, 150)
    out.append(Case("graded_logspace_n150", d, 0.3 * d[1:]))
    out.append(Case("ramp_n200_e_1e-120", np.arange(1.0, 201.0), np.full(199, 1e-120)))
    out.append(Case("identity_n100", np.ones(100), np.zeros(99), closed="diagonal"))
    out.append(Case("negative_definite_n130", -np.arange(1.0, 131.0), np.full(129, 0.5)))
    for scale in (1e150, 1e-150):
        rng = np.random.default_rng(150)
        out.append(Case("random_n100_scale%g" % scale, scale * rng.standard_normal(100), scale * rng.standard_normal(99)))
    rng = np.random.default_rng(256)
    out.append(Case("permuted_ramp_n256_e_0.01", rng.permutation(np.arange(1.0, 257.0)), np.full(255, 0.01)))
    out.append(Case("antidiagonal_2x2", np.zeros(2), np.ones(1)))
    out.append(Case("diagonal_n7", np.array([3.0, 1.0, 4.0, 1.5, 9.0, 2.0, 6.0]), np.zeros(6), closed="diagonal"))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return {c.name: c for c in cases()}[name]


def names(vectors=None):
    return [c.name for c in cases() if vectors is None or c.vectors == vectors]


# the cases whose eigenvalue is handed in exactly, so that a pivot is exactly zero: name -> (lam ascending, vectors as columns)
def exact_pivot_cases():
    h = np.sqrt(0.5)
    dg = case("diagonal_n7")
    order = np.argsort(dg.d)
    return {"antidiagonal_2x2": (np.array([-1.0, 1.0]), np.array([[h, h], [-h, h]])),
            "diagonal_n7": (dg.d[order], np.eye(7)[:, order])}


# ---- truth of the eigenvalues -----------------------------------------------------------------------------------------------
def closed_form(kind, c):
    """eigenvalues of the SCALED matrix, ascending, longdouble"""
    n = c.n
    if kind == "toeplitz":
        k = np.arange(1, n + 1, dtype=LD)
        pi = LD(4) * np.arctan(LD(1))
        lam = LD(2) - LD(2) * np.cos(k * pi / LD(n + 1))
    elif kind == "clement":
        lam = np.arange(-(n - 1), n, 2).astype(LD)
    elif kind == "diagonal":
        return np.sort(c.ds.astype(LD))
    else:
        raise KeyError(kind)
    return np.sort(lam) * LD(c.f)


def bisect_longdouble(ds, es, halvings=90):
    """All eigenvalues, ascending, by plain bisection on q_i = (d_i - x) - e_{i-1}^2 / q_{i-1} in longdouble, vectorised over the
    eigenvalues.  |q| < pivmin -> -pivmin (dstebz): without it a midpoint that makes a pivot exactly zero (Toeplitz, Clement)
    divides by zero."""
    d, e = np.asarray(ds, dtype=LD), np.asarray(es, dtype=LD)
    n = d.size
    e2 = e * e
    pivmin = np.finfo(LD).tiny * max(LD(1), e2.max() if n > 1 else LD(1))
    b = LD(bnorm(ds, es))
    lo = np.full(n, -b * LD(1.0000001) - np.finfo(LD).tiny)
    hi = -lo
    k = np.arange(n)
    for _ in range(halvings):
        mid = (lo + hi) / LD(2)
        q = d[0] - mid
        q = np.where(np.abs(q) < pivmin, -pivmin, q)
        cnt = (q < 0).astype(np.int64)
        for i in range(1, n):
            q = (d[i] - mid) - e2[i - 1] / q
            q = np.where(np.abs(q) < pivmin, -pivmin, q)
            cnt += q < 0
        below = cnt <= k                        # fewer than k + 1 eigenvalues lie below mid: eigenvalue k is at or above it
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
    return (lo + hi) / LD(2)


@functools.lru_cache(maxsize=None)
def truth_values(name):
    """eigenvalues of the scaled matrix, ascending, longdouble"""
    c = case(name)
    out = closed_form(c.closed, c) if c.closed else bisect_longdouble(c.ds, c.es)
    out.setflags(write=False)
    return out


def lam_for_vectors(name):
    """the truth rounded to double in the CALLER's scale, ascending: what the vector kernel is handed"""
    c = case(name)
    return (truth_values(name) / LD(c.f)).astype(np.float64)


# ---- truth of the vectors ---------------------------------------------------------------------------------------------------
def _floor(x, piv):
    return np.where(np.abs(x) >= piv, x, np.where(x < 0, -piv, piv))


def _twisted(d, e, lam, piv, one_over):
    """Columns: the twisted-factorisation vector of every lam, in the dtype of d.  The statement of trd_twisted_kernel: D+ forwards
    and D- backwards with the pivot floor, the twist at the first smallest |D+ + D- - (d - lam)|, z upwards with D+ and downwards
    with D-, the squares summed in the order of the walk, one scale at the end."""
    n, m = d.size, lam.size
    dt = d.dtype.type
    if n == 1:
        return np.ones((1, m), dtype=d.dtype)
    Dp, Dm = np.empty((n, m), dtype=d.dtype), np.empty((n, m), dtype=d.dtype)
    x = d[0] - lam
    for i in range(n - 1):
        x = _floor(x, piv)
        Dp[i] = x
        x = (d[i + 1] - lam) - (e[i] * one_over(x)) * e[i]
    Dp[n - 1] = _floor(x, piv)
    x = _floor(d[n - 1] - lam, piv)
    Dm[n - 1] = x
    for i in range(n - 2, -1, -1):
        x = _floor((d[i] - lam) - (e[i] * one_over(x)) * e[i], piv)
        Dm[i] = x
    gam = np.abs((Dp + Dm) - (d[:, None] - lam[None, :]))
    r = np.argmin(gam, axis=0)                                  # (the first occurrence)
    Z = np.zeros((n, m), dtype=d.dtype)
    Z[r, np.arange(m)] = dt(1)
    up, down = np.ones(m, dtype=d.dtype), np.zeros(m, dtype=d.dtype)
    for i in range(n - 2, -1, -1):
        on = i < r
        z = -(e[i] * one_over(Dp[i])) * Z[i + 1]
        Z[i] = np.where(on, z, Z[i])
        up = np.where(on, up + z * z, up)
    for i in range(n - 1):
        on = i >= r
        z = -(e[i] * one_over(Dm[i + 1])) * Z[i]
        Z[i + 1] = np.where(on, z, Z[i + 1])
        down = np.where(on, down + z * z, down)
    return Z * (dt(1) / np.sqrt(up + down))


@functools.lru_cache(maxsize=None)
def truth_vectors(name):
    """(n, n) longdouble: column k the unit vector of eigenvalue k (ascending) of the scaled matrix"""
    c = case(name)
    with np.errstate(all="ignore"):
        Z = _twisted(c.ds.astype(LD), c.es.astype(LD), truth_values(name), LD(10) ** -4000, lambda x: LD(1) / x)
    Z.setflags(write=False)
    return Z


def toeplitz_vectors(n):
    """(n, n) longdouble: column k-1 is sin(i k pi / (n + 1)), i = 1 .. n, scaled to unit length (eigenvalues ascending in k)"""
    pi = LD(4) * np.arctan(LD(1))
    i = np.arange(1, n + 1, dtype=LD)
    Z = np.sin(np.outer(i, i) * pi / LD(n + 1))
    return Z / np.sqrt(np.sum(Z * Z, axis=0))


# ---- restatement of the kernels in float64 ----------------------------------------------------------------------------------
def restate_values(ds, es, index=None):
    """trd_bisect_kernel in float64 numpy for the eigenvalues `index` (ascending numbering; None: all) of the scaled matrix: e^2
    with its floor 2^-200, the Gershgorin interval widened by 2.2e-16 bnorm n + 1e-300, 14 passes of 16 interior points, the count
    by the three-term recurrence of the minors with (p_i, p_{i-1}) rescaled by a power of two after every eighth row of the
    unrolled part, signs on the sign bit.  Returns 0.5 (lo + hi), ascending."""
    d = np.asarray(ds, dtype=np.float64)
    e = np.asarray(es, dtype=np.float64)
    n = d.size
    e2 = np.maximum(e * e, E2_FLOOR)
    el, er = np.concatenate(([0.0], np.abs(e))), np.concatenate((np.abs(e), [0.0]))
    rad = el + er
    gl, gu = float(np.min(d - rad)), float(np.max(d + rad))
    bn = max(abs(gl), abs(gu))
    gl -= 2.2e-16 * bn * n + 1e-300
    gu += 2.2e-16 * bn * n + 1e-300
    k = np.arange(n) if index is None else np.asarray(index, dtype=np.int64)
    lo, hi = np.full(k.size, gl), np.full(k.size, gu)
    frac = np.arange(1, POINTS + 1, dtype=np.float64) * (1.0 / 17.0)
    rows = np.arange(k.size)
    with np.errstate(all="ignore"):
        for _ in range(PASSES):
            x = lo[:, None] + (hi - lo)[:, None] * frac[None, :]
            pm = np.ones_like(x)
            pc = d[0] - x
            sc = np.signbit(pc)
            cnt = sc.astype(np.int64)
            i = 1
            while i + 8 <= n:
                for u in range(8):
                    pn = (d[i + u] - x) * pc - e2[i + u - 1] * pm
                    sn = np.signbit(pn)
                    cnt += sn ^ sc
                    sc, pm, pc = sn, pc, pn
                mx = np.maximum(np.abs(pc), np.abs(pm))
                pc = np.where(mx == 0.0, np.where(sc, -1.0, 1.0), pc)
                ex = np.frexp(mx)[1]
                pc, pm = np.ldexp(pc, -ex), np.ldexp(pm, -ex)
                i += 8
            for i in range(i, n):
                pn = (d[i] - x) * pc - e2[i - 1] * pm
                sn = np.signbit(pn)
                cnt += sn ^ sc
                sc, pm, pc = sn, pc, pn
            s = np.sum(cnt <= k[:, None], axis=1)
            x_lo = x[rows, np.maximum(s - 1, 0)]
            x_hi = x[rows, np.minimum(s, POINTS - 1)]
            lo = np.where(s > 0, x_lo, lo)
            hi = np.where(s < POINTS, x_hi, hi)
    return 0.5 * (lo + hi)


def twisted_pivot_floor(es):
    emax = float(np.max(np.abs(es))) if len(es) else 0.0
    return 2.3e-308 * max(1.0, emax * emax) * 1e20 + 1e-300


def restate_vectors(ds, es, lam_scaled):
    """trd_twisted_kernel in float64 numpy: columns = the vectors of `lam_scaled` (the scaled matrix's scale)"""
    d, e = np.asarray(ds, dtype=np.float64), np.asarray(es, dtype=np.float64)
    with np.errstate(all="ignore"):
        return _twisted(d, e, np.asarray(lam_scaled, dtype=np.float64), twisted_pivot_floor(e), lambda x: 1.0 / x)


def value_index(c):
    """the eigenvalues (ascending numbering) the restatement of the values is formed for"""
    if c.stride == 1:
        return np.arange(c.n)
    return np.unique(np.concatenate((np.arange(c.stride), np.arange(0, c.n, c.stride), np.arange(c.n - c.stride, c.n))))


# ---- figures, in units of eps * bnorm ---------------------------------------------------------------------------------------
def value_errors(name, lam_asc_scaled, index=None):
    """|lam - truth| / (eps bnorm) per eigenvalue; lam in the scaled matrix's scale (float64 or longdouble)"""
    c = case(name)
    t = truth_values(name)
    if index is not None:
        t = t[index]
    return np.abs(np.asarray(lam_asc_scaled, dtype=LD) - t).astype(np.float64) / (EPS * c.bnorm)


def device_values_scaled(name, lam_desc):
    """what `Handle.tridiag_eigenvalues` returns (descending, the caller's scale) -> ascending, the scaled matrix's scale, longdouble"""
    return np.asarray(lam_desc, dtype=LD)[::-1] * LD(case(name).f)


@functools.lru_cache(maxsize=None)
def restated_value_error(name):
    """r: the worst error of the restatement on the case"""
    c = case(name)
    idx = value_index(c)
    return float(np.max(value_errors(name, restate_values(c.ds, c.es, None if c.stride == 1 else idx), idx)))


def gaps(name):
    """distance of every eigenvalue of the scaled matrix to the nearest other one (longdouble; inf for n = 1)"""
    t = truth_values(name)
    g = np.full(t.size, np.inf, dtype=LD)
    if t.size > 1:
        dl = np.diff(t)
        g[:-1] = dl
        g[1:] = np.minimum(g[1:], dl)
    return g


def vector_figures(name, Y, first=0):
    """Of the columns of Y (float64), vectors of the eigenvalues first, first + 1, ... (ascending) of the case:
    res: ||T z - lam z||_2 / (eps bnorm), T the scaled matrix, lam the double handed to the kernel, in longdouble;
    ang: ||s z - z_truth||_2 * gap / (eps bnorm), s = +-1, where the gap exceeds GAP_MIN bnorm, NaN elsewhere;
    nrm: | ||z|| - 1 | / eps."""
    c = case(name)
    Z = np.asarray(Y, dtype=LD)
    m = Z.shape[1]
    d, e = c.ds.astype(LD), c.es.astype(LD)
    lam = (lam_for_vectors(name)[first:first + m]).astype(LD) * LD(c.f)
    R = d[:, None] * Z - Z * lam[None, :]
    if c.n > 1:
        R[:-1] += e[:, None] * Z[1:]
        R[1:] += e[:, None] * Z[:-1]
    res = np.sqrt(np.sum(R * R, axis=0)) / LD(EPS * c.bnorm)
    T = truth_vectors(name)[:, first:first + m]
    s = np.where(np.sum(Z * T, axis=0) < 0, LD(-1), LD(1))
    dist = np.sqrt(np.sum((Z * s - T) ** 2, axis=0))
    g = gaps(name)[first:first + m]
    ang = np.where(g > LD(GAP_MIN * c.bnorm), dist * np.where(np.isfinite(g), g, LD(0)) / LD(EPS * c.bnorm), LD(np.nan))
    nrm = np.abs(np.sqrt(np.sum(Z * Z, axis=0)) - LD(1)) / LD(EPS)
    return {"res": res.astype(np.float64), "ang": ang.astype(np.float64), "nrm": nrm.astype(np.float64)}


def worst(fig):
    """the largest residual and angle figure of `vector_figures` (0 where no column has a gap)"""
    ang = fig["ang"][~np.isnan(fig["ang"])]
    return float(np.max(fig["res"])), float(np.max(ang)) if ang.size else 0.0


@functools.lru_cache(maxsize=None)
def restated_vectors(name):
    c = case(name)
    Y = restate_vectors(c.ds, c.es, lam_for_vectors(name) * c.f)
    Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=None)
def restated_vector_figures(name):
    """(r_res, r_ang): the restatement's worst figures on the case"""
    return worst(vector_figures(name, restated_vectors(name)))
