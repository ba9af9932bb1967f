"""The two-ended Sturm count of `trd_bisect_kernel` (csrc/tridiag.h) restated in float64 numpy, and the inputs that aim at its
junction.  Cases, truth and helpers come from tests/tridiag_stage_cases.py; no GPU code here.

With m = n // 2 and a trial point x the kernel runs two chains of half the length,

    forward   p_0 = 1,  p_{i+1} = (d_i - x) p_i - e_{i-1}^2 p_{i-1}            up to p_m       (m rows),
    backward  q_n = 1,  q_{n+1} = 0,  q_i = (d_i - x) q_{i+1} - e_i^2 q_{i+2}   down to q_{m+1}  (nb = n - 1 - m rows),

and counts  changes(p_0 .. p_m) + changes(q_n .. q_{m+1}) + [gamma_m < 0],  sign(gamma_m) = sign(det) sign(p_m) sign(q_{m+1}),
det = p_{m+1} q_{m+1} - e_m^2 p_m q_{m+2}.  The backward chain is the forward chain of the reversed matrix.  Both chains are cut
into eight-row blocks (a power-of-two rescale of the pair behind each) by the shorter one's length nb; the rows left over - one
more in the forward chain when n is even - follow without a rescale.  A sign is the sign bit; e^2 has the floor 2^-200.  Everything
else (interval, 14 passes of 16 points, the choice of the bracket) is `restate_values` of tridiag_stage_cases.py."""
import functools

import numpy as np

import tridiag_stage_cases as C


def _chain(dd, cc, length, blocked, x):
    """Rows 0 .. length - 1 of one chain at the points x: dd[j] the diagonal entry of row j, cc[j] the squared coupling of rows
    j - 1 and j (cc[0] unused).  Returns (c_length, c_{length-1}, sign changes along 1, c_1, ..., c_length)."""
    if length == 0:
        return np.ones_like(x), np.zeros_like(x), np.zeros(x.shape, dtype=np.int64)
    pm = np.ones_like(x)
    pc = dd[0] - x
    sc = np.signbit(pc)
    cnt = sc.astype(np.int64)
    i = 1
    while i + 8 <= blocked:
        for u in range(8):
            pn = (dd[i + u] - x) * pc - cc[i + u] * pm
            sn = np.signbit(pn)
            cnt += sn ^ sc
            sc, pm, pc = sn, pc, pn
        mx = np.maximum(np.abs(pc), np.abs(pm))
        pc = np.where(mx == 0.0, np.where(sc, -1.0, 1.0), pc)
        ex = np.frexp(mx)[1]
        pc, pm = np.ldexp(pc, -ex), np.ldexp(pm, -ex)
        i += 8
    for i in range(i, length):
        pn = (dd[i] - x) * pc - cc[i] * pm
        sn = np.signbit(pn)
        cnt += sn ^ sc
        sc, pm, pc = sn, pc, pn
    return pc, pm, cnt


def two_ended_count(d, e2, x):
    """The count of the kernel at the points x (any shape) for the diagonal d (n) and the floored squares e2 (n - 1)."""
    n = d.size
    m = n // 2
    nb = n - 1 - m
    floor = C.E2_FLOOR
    cf = np.concatenate(([floor], e2))                      # cf[j]: rows j - 1 and j
    cb = np.concatenate(([floor], e2[::-1]))                # the same of the reversed matrix
    p_c, p_m, cnt_f = _chain(d, cf, m, nb, x)
    q_c, q_m, cnt_b = _chain(d[::-1], cb, nb, nb, x)
    ext = (d[m] - x) * p_c - cf[m] * p_m                    # p_{m+1}
    e2m = e2[m] if m < n - 1 else floor
    det = ext * q_c - (e2m * p_c) * q_m
    return cnt_f + cnt_b + (np.signbit(det) ^ np.signbit(p_c) ^ np.signbit(q_c))


def restate_values_two_ended(ds, es, index=None):
    """trd_bisect_kernel in float64 numpy, separate multiply and add, for the eigenvalues `index` (ascending numbering; None: all)
    of the scaled matrix.  Returns 0.5 (lo + hi), ascending."""
    d = np.asarray(ds, dtype=np.float64)
    e = np.asarray(es, dtype=np.float64)
    n = d.size
    e2 = np.maximum(e * e, C.E2_FLOOR)
    el, er = np.concatenate(([0.0], np.abs(e))), np.concatenate((np.abs(e), [0.0]))
    rad = el + er
    gl, gu = float(np.min(d - rad)), float(np.max(d + rad))
    bn = max(abs(gl), abs(gu))
    gl -= 2.2e-16 * bn * n + 1e-300
    gu += 2.2e-16 * bn * n + 1e-300
    k = np.arange(n) if index is None else np.asarray(index, dtype=np.int64)
    lo, hi = np.full(k.size, gl), np.full(k.size, gu)
    frac = np.arange(1, C.POINTS + 1, dtype=np.float64) * (1.0 / 17.0)
    rows = np.arange(k.size)
    with np.errstate(all="ignore"):
        for _ in range(C.PASSES):
            x = lo[:, None] + (hi - lo)[:, None] * frac[None, :]
            cnt = two_ended_count(d, e2, x)
            s = np.sum(cnt <= k[:, None], axis=1)
            x_lo = x[rows, np.maximum(s - 1, 0)]
            x_hi = x[rows, np.minimum(s, C.POINTS - 1)]
            lo = np.where(s > 0, x_lo, lo)
            hi = np.where(s < C.POINTS, x_hi, hi)
    return 0.5 * (lo + hi)


# ---- inputs that aim at the junction ----------------------------------------------------------------------------------------
REVERSED = ("random_n2", "random_n3", "random_n9", "random_n17", "random_n33", "random_n65", "random_n130", "wilkinson21_x6_glue1e-07",
            "graded_logspace_n150", "clement_n200", "negative_definite_n130", "permuted_ramp_n256_e_0.01")
HALF_SIZES = (4, 5, 14, 15, 16, 17, 18, 19, 31, 32, 33, 34, 35)    # each half crosses the eight-row block


@functools.lru_cache(maxsize=None)
def junction_cases():
    out = []
    for name in REVERSED:
        c = C.case(name)
        out.append(C.Case("reversed_" + name, c.d[::-1], c.e[::-1]))
    for n in HALF_SIZES:
        rng = np.random.default_rng(2000 + n)
        d, e = rng.standard_normal(n), rng.standard_normal(n - 1)
        m = n // 2
        out.append(C.Case("half_random_n%d" % n, d, e))
        for j, tag in ((m - 1, "below"), (m, "above")):                  # e = 0 on either side of the junction row m
            if 0 <= j < n - 1:
                ez = e.copy()
                ez[j] = 0.0
                out.append(C.Case("half_random_n%d_e_zero_%s" % (n, tag), d, ez))
    ramp, zeros = np.arange(1.0, 18.0), np.zeros(17)
    out.append(C.Case("spectrum_in_the_upper_half", np.concatenate((zeros, ramp)), np.full(33, 1e-3)))
    out.append(C.Case("spectrum_in_the_lower_half", np.concatenate((ramp, zeros)), np.full(33, 1e-3)))
    out.append(C.Case("diagonal_1_2", np.array([1.0, 2.0]), np.zeros(1)))
    out.append(C.Case("three_e_0_1", np.array([0.3, -0.7, 1.1]), np.array([0.0, 1.0])))
    out.append(C.Case("three_e_1_0", np.array([0.3, -0.7, 1.1]), np.array([1.0, 0.0])))
    out.append(C.Case("zero_diagonal_n34", np.zeros(34), np.random.default_rng(34).standard_normal(33)))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def junction_case(name):
    return {c.name: c for c in junction_cases()}[name]


def junction_names():
    return [c.name for c in junction_cases()]


@functools.lru_cache(maxsize=None)
def junction_truth(name):
    """eigenvalues of the scaled matrix, ascending, longdouble (bisect_longdouble)"""
    c = junction_case(name)
    out = C.bisect_longdouble(c.ds, c.es)
    out.setflags(write=False)
    return out


def junction_errors(name, lam_asc_scaled):
    """|lam - truth| / (eps bnorm) per eigenvalue; lam in the scaled matrix's scale"""
    c = junction_case(name)
    return np.abs(np.asarray(lam_asc_scaled, dtype=C.LD) - junction_truth(name)).astype(np.float64) / (C.EPS * c.bnorm)


@functools.lru_cache(maxsize=None)
def junction_restated_error(name):
    """r: the worst error of the existing one-ended restatement `restate_values` on the input"""
    c = junction_case(name)
    return float(np.max(junction_errors(name, C.restate_values(c.ds, c.es))))
