"""CPU restatements behind the edge tests of the blocked Cholesky (csrc/cholesky.h, csrc/chol64.h) and the batched FFT
(csrc/fft.h): tests/test_kernel_edges_oracle.py (no device) and tests/test_gpu_cholesky_fft_edges.py.

* cholesky_schedule / cholesky_sizes: the panel loop of cholesky_upper restated, and the smallest sizes that reach each of its
  slicing edges for a given number of compute units.
* fft_plan / stockham: fft_plan and fft_stage in float64 numpy - the same radix order, the same twiddle scheme, the same
  order of the sums - so that its distance from the truth is what the kernel's arithmetic costs, roundings of FMA aside.
* fft_truth / fft_ex_truth: the transform in long double (scipy.fft on clongdouble), and the definition above
  fft_batch_kernel assembled from it with every option.
* the inputs of the tests: Wishart and graded matrices, fields for the analytic frame.

numpy and scipy only; nothing here touches a device."""
import numpy as np
import scipy.fft

# ------------------------------------------------------------------------------------------------
# Cholesky: the panel loop of cholesky_upper
# ------------------------------------------------------------------------------------------------
CHOL_NB = 64
CHOL_FIXED_SIZES = (1, 15, 16, 17, 63, 64, 65, 79, 80, 81, 127, 128, 129, 191, 192, 193)
CHOL_SEARCH_CAP = 3000


def _ceil_div(a, b):
    return -(-a // b)


def cholesky_schedule(n, cus):
    """(k0, ntile, nsplit, kchunk, rows of the last slice) of every row update of cholesky_upper(n) on `cus` compute units
    (cholesky.h: the loop over k0 > 0)."""
    out = []
    for k0 in range(CHOL_NB, n, CHOL_NB):
        ntile = _ceil_div(n - k0, 64)
        nsplit = max(1, min(_ceil_div(3 * cus // 4, ntile), _ceil_div(k0, 64)))
        kchunk = _ceil_div(_ceil_div(k0, nsplit), 16) * 16
        nsplit = _ceil_div(k0, kchunk)
        out.append((k0, ntile, nsplit, kchunk, k0 - (nsplit - 1) * kchunk))
    return out


# edge -> predicate on one panel (k0, ntile, nsplit, kchunk, last)
CHOL_EDGES = {
    "nsplit_ge_5_not_multiple_of_4": lambda p: p[2] >= 5 and p[2] % 4 != 0,     # the clamped index of the slab sum is used
    "nsplit_gt_8": lambda p: p[2] > 8,
    "nsplit_gt_16": lambda p: p[2] > 16,
    "kchunk_odd_multiple_of_16": lambda p: (p[3] // 16) % 2 == 1,               # the k-loop ends on its first operand set
    "last_slice_32_rows": lambda p: p[2] > 1 and p[4] == 32,
    "last_slice_16_rows": lambda p: p[2] > 1 and p[4] == 16,
}


def cholesky_edges_reached(n, cus):
    sched = cholesky_schedule(n, cus)
    return {name for name, hit in CHOL_EDGES.items() if any(hit(p) for p in sched)}


def cholesky_sizes(cus, cap=CHOL_SEARCH_CAP):
    """{"fixed": sizes that do not depend on the chip, "edges": edge -> smallest n <= cap that reaches it,
    "skipped": edges no n <= cap reaches (with the reason), "sizes": all of them, sorted}"""
    edges, todo = {}, set(CHOL_EDGES)
    for n in range(CHOL_NB + 1, cap + 1):
        for name in sorted(todo & cholesky_edges_reached(n, cus)):
            edges[name] = n
            todo.discard(name)
        if not todo:
            break
    skipped = {name: "no n <= %d reaches it on %d compute units" % (cap, cus) for name in sorted(todo)}
    return {"fixed": list(CHOL_FIXED_SIZES), "edges": edges, "skipped": skipped,
            "sizes": sorted(set(CHOL_FIXED_SIZES) | set(edges.values()))}


# ------------------------------------------------------------------------------------------------
# Cholesky: inputs and measures
# ------------------------------------------------------------------------------------------------
def wishart(n, cplx, seed=0):
    """X X^H, X of n x (2n + 3) standard normal entries: Hermitian positive definite, condition number about 33"""
    rng = np.random.default_rng([seed, n, int(cplx)])
    X = rng.standard_normal((n, 2 * n + 3))
    if cplx:
        X = X + 1j * rng.standard_normal((n, 2 * n + 3))
    A = X @ X.conj().T
    A = (A + A.conj().T) / 2
    if cplx:
        A[np.diag_indices(n)] = A.diagonal().real
    return A


def graded(n, cplx, seed=0, decades=6.0):
    """D W D with W = wishart(n) and D falling evenly over decades / 2: the diagonal, and with it the squared pivots, spread
    over 10^decades (inside the 1e8 that factor_by_cholesky accepts)"""
    d = np.logspace(0.0, -decades / 2, n)
    A = wishart(n, cplx, seed + 1) * np.outer(d, d)
    return A


def centred_gram(n, cplx, seed=0):
    """X X^H of a field with its column means removed along the first axis: singular (the constant vector)"""
    rng = np.random.default_rng([seed, n, 2 + int(cplx)])
    X = rng.standard_normal((n, 2 * n + 3))
    if cplx:
        X = X + 1j * rng.standard_normal((n, 2 * n + 3))
    X = X - X.mean(axis=0)
    A = X @ X.conj().T
    A = (A + A.conj().T) / 2
    if cplx:
        A[np.diag_indices(n)] = A.diagonal().real
    return A


def chol_backward_error(R, A):
    """max |R^H R - A| / max diag(A), float64"""
    return float(np.max(np.abs(R.conj().T @ R - A)) / np.max(A.diagonal().real))


def lapack_upper(A):
    """LAPACK's factor as an upper triangular R with R^H R = A"""
    return np.linalg.cholesky(A).conj().T


def left_looking_cholesky(A, cus, drop_tail_slices=False, skip_second_operand_set=False):
    """The panel loop of cholesky_upper in float64 numpy with the slices of cholesky_schedule: (R, ok).  The two switches
    restate what two arithmetic mistakes in chol64_rowupdate_kernel would do - the slab sum stopping at the last full group
    of four slices; the second operand set of the k-loop (rows 16 .. 31 of every step of 32) left out when kchunk / 16 is odd -
    so that their cost can be shown without a device."""
    A = np.array(A)
    n = A.shape[0]
    sched = {p[0]: p for p in cholesky_schedule(n, cus)}
    ok = True
    for k0 in range(0, n, CHOL_NB):
        nb = min(CHOL_NB, n - k0)
        if k0 > 0:
            _, _, nsplit, kchunk, _ = sched[k0]
            total = np.zeros((nb, n - k0), dtype=A.dtype)
            for s in range(nsplit):
                if drop_tail_slices and s >= 4 * (nsplit // 4):
                    break
                rows = np.arange(s * kchunk, min(k0, (s + 1) * kchunk))
                if skip_second_operand_set and (kchunk // 16) % 2 == 1:
                    rows = rows[((rows - s * kchunk) // 16) % 2 == 0]
                total = total + A[rows, k0:k0 + nb].conj().T @ A[rows, k0:]
            A[k0:k0 + nb, k0:] -= total
        D = A[k0:k0 + nb, k0:k0 + nb]
        D = np.triu(D) + np.triu(D, 1).conj().T
        try:
            R11 = np.linalg.cholesky(D).conj().T
        except np.linalg.LinAlgError:
            return np.triu(A), False
        A[k0:k0 + nb, k0:k0 + nb] = R11
        if k0 + nb < n:
            A[k0:k0 + nb, k0 + nb:] = np.linalg.solve(R11.conj().T, A[k0:k0 + nb, k0 + nb:])
    return np.triu(A), ok


# ------------------------------------------------------------------------------------------------
# FFT: plan, stage and truth
# ------------------------------------------------------------------------------------------------
FFT_MAX_N = 5120
FFT_RADICES = (4, 2, 3, 5, 7)
FFT_LENGTHS = (2, 3, 4, 5, 7, 8, 9, 16, 25, 27, 49, 125, 343, 512, 540, 2048, 2049 - 1, 2187, 3125, 4096, 4374, 4375, 4802,
               5000, 5040, 5103, 5120)
# cos / sin of 2 pi k / R as fft.h spells them (FftRoots)
FFT_ROOTS = {
    2: ((1.0, -1.0), (0.0, 0.0)),
    3: ((1.0, -0.5, -0.5), (0.0, 0.86602540378443864676, -0.86602540378443864676)),
    4: ((1.0, 0.0, -1.0, 0.0), (0.0, 1.0, 0.0, -1.0)),
    5: ((1.0, 0.30901699437494742410, -0.80901699437494742410, -0.80901699437494742410, 0.30901699437494742410),
        (0.0, 0.95105651629515357212, 0.58778525229247312917, -0.58778525229247312917, -0.95105651629515357212)),
    7: ((1.0, 0.62348980185873353053, -0.22252093395631440429, -0.90096886790241912624, -0.90096886790241912624,
         -0.22252093395631440429, 0.62348980185873353053),
        (0.0, 0.78183148246802980871, 0.97492791218182360702, 0.43388373911755812048, -0.43388373911755812048,
         -0.97492791218182360702, -0.78183148246802980871)),
}


def fft_plan(n):
    """The radices of the stages in order, or None when fft.h refuses the length"""
    if n < 2 or n > FFT_MAX_N:
        return None
    plan, rest = [], n
    for r in FFT_RADICES:
        while rest % r == 0 and len(plan) < 24:
            plan.append(r)
            rest //= r
    return plan if rest == 1 else None


def _sincospi(ang):
    """sin(pi ang), cos(pi ang) rounded once to float64 (through long double), as a correctly rounded sincospi gives them"""
    pi = np.longdouble("3.14159265358979323846264338327950288")
    x = np.asarray(ang, dtype=np.longdouble) * pi
    return np.sin(x).astype(np.float64), np.cos(x).astype(np.float64)


def _stage(ar, ai, n, R, Ns, sign, roots=None):
    """fft_stage<R>: ar, ai of shape (..., n) float64 -> the planes after the stage (every product and sum a separate float64
    rounding, in the kernel's order)"""
    rc, rs = (roots or FFT_ROOTS)[R]
    nr = n // R
    j = np.arange(nr)
    k = j % Ns
    c1, s1 = np.ones(nr), np.zeros(nr)
    if Ns > 1:
        s1, c1 = _sincospi(2.0 * k.astype(np.float64) / float(Ns * R))
        s1 = s1 * sign
    wr, wi = c1.copy(), s1.copy()
    vr, vi = [ar[..., j]], [ai[..., j]]
    for r in range(1, R):
        xr, xi = ar[..., j + r * nr], ai[..., j + r * nr]
        vr.append(xr * wr - xi * wi)
        vi.append(xr * wi + xi * wr)
        if r + 1 < R:
            t = wr * c1 - wi * s1
            wi = wr * s1 + wi * c1
            wr = t
    outr, outi = np.empty_like(ar), np.empty_like(ai)
    j0 = (j - k) * R + k
    for q in range(R):
        zr, zi = vr[0].copy(), vi[0].copy()
        for r in range(1, R):
            c, sn = rc[(q * r) % R], sign * rs[(q * r) % R]
            zr = zr + (vr[r] * c - vi[r] * sn)
            zi = zi + (vr[r] * sn + vi[r] * c)
        outr[..., j0 + q * Ns] = zr
        outi[..., j0 + q * Ns] = zi
    return outr, outi


def stockham(x, sign=-1, roots=None):
    """The transform of fft_batch_kernel along the last axis in float64 numpy: sum_t x[t] exp(sign 2 pi i k t / n).
    `roots`: another table in place of FFT_ROOTS (what a wrong constant would cost)."""
    x = np.asarray(x)
    n = x.shape[-1]
    plan = fft_plan(n)
    if plan is None:
        raise ValueError("no plan for length %d" % n)
    ar = np.array(x.real, dtype=np.float64)
    ai = np.array(x.imag, dtype=np.float64) if np.iscomplexobj(x) else np.zeros_like(ar)
    Ns = 1
    for R in plan:
        ar, ai = _stage(ar, ai, n, R, Ns, float(sign), roots)
        Ns *= R
    return ar + 1j * ai


def fft_truth(x, sign=-1):
    """The same transform in long double (scipy.fft on clongdouble), any length"""
    x = np.asarray(x).astype(np.clongdouble)
    if sign < 0:
        return scipy.fft.fft(x, axis=-1)
    return np.conj(scipy.fft.fft(np.conj(x), axis=-1))


def fft_error(y, truth):
    """max |y - truth| / max |truth|"""
    truth = np.asarray(truth)
    return float(np.max(np.abs(np.asarray(y).astype(np.clongdouble) - truth)) / np.max(np.abs(truth)))


def fft_present_bar(n):
    """the bar of test_fft_matches_numpy (tests/test_gpu_kernels.py)"""
    return 1e-13 * np.sqrt(n) * np.log2(n + 1)


def fft_input(batch, n, cplx, seed=0):
    rng = np.random.default_rng([seed, batch, n, int(cplx)])
    x = rng.standard_normal((batch, n))
    return x + 1j * rng.standard_normal((batch, n)) if cplx else x


def fft_ex_truth(x, n, sign, n_keep=None, conj_in=False, sin=None, sa=None, sb=None, scale=1.0):
    """out[b][k] = sa[k] sb[b] scale sum_{t < n_in} x'[b][t] exp(sign 2 pi i k t / n), k < n_keep, in long double;
    x (batch, n_in) holds the n_in elements that are read, x' = sin * conj(x) with conj_in, sin * x without."""
    x = np.asarray(x).astype(np.clongdouble)
    batch, n_in = x.shape
    if conj_in:
        x = np.conj(x)
    if sin is not None:
        x = x * np.asarray(sin, dtype=np.longdouble)[None, :]
    full = np.zeros((batch, n), dtype=np.clongdouble)
    full[:, :n_in] = x
    y = fft_truth(full, sign)[:, :n if n_keep is None else n_keep]
    y = y * np.longdouble(scale)
    if sa is not None:
        y = y * np.asarray(sa, dtype=np.longdouble)[None, :]
    if sb is not None:
        y = y * np.asarray(sb, dtype=np.longdouble)[:, None]
    return y


# ------------------------------------------------------------------------------------------------
# analytic frame end to end
# ------------------------------------------------------------------------------------------------
ANALYTIC_CASES = [(T, two) for T in (12, 35, 22, 33) for two in (False, True)]     # 12, 35: FFT route; 22, 33: GEMM fallback
ANALYTIC_MIN_MODES = 5
ANALYTIC_GAP = 0.02


def analytic_m(T):
    """modes of the analytic frame (solver.h analytic_basis)"""
    return T // 2 + 1 if T % 2 == 0 else (T + 1) // 2


def analytic_fields(T, two_fields, seed=0):
    """Real float64 fields wider than T (N = 3 T, and 2 T for the second one) whose frequency k carries the amplitude 0.9^k:
    the singular values of the complexified model fall by about 0.81 a mode, so that most modes stand clear of their
    neighbours while sigma_1 / sigma_m stays below 50 at the 17 modes of T = 33 and 35.  That ratio is kept small on purpose:
    a two-field solve squares the spectrum (HISTORY.md, accuracy of small modes: vectors to about 5e-14 (sigma_1 / sigma_i)^2
    over the relative gap), so modes a factor 1500 below the first - what 0.8^k gives, measured 7.2e-8 at T = 33 - are out of
    reach of a 1e-8 comparison of vectors whatever route forms the Gram matrix, and would say nothing about the frame."""
    rng = np.random.default_rng([seed, T, int(two_fields)])
    t = np.arange(T)
    out = []
    for N in ([3 * T, 2 * T] if two_fields else [3 * T]):
        X = np.zeros((T, N))
        for k in range(1, T // 2 + 1):
            amp = 0.9 ** k
            X += amp * (np.outer(np.cos(2 * np.pi * k * t / T), rng.standard_normal(N))
                        + np.outer(np.sin(2 * np.pi * k * t / T), rng.standard_normal(N)))
        out.append(X + 0.01 * rng.standard_normal((T, N)))
    return out


def separated_modes(sigma, m, gap=ANALYTIC_GAP):
    """indices i < m of the singular values above 1e-8 sigma_1 whose distance to both neighbours exceeds gap * sigma_i"""
    s = np.asarray(sigma, dtype=np.float64)
    keep = []
    for i in range(min(m, len(s))):
        if not s[i] > 1e-8 * s[0]:
            continue
        lo = s[i - 1] - s[i] if i > 0 else np.inf
        hi = s[i] - s[i + 1] if i + 1 < len(s) else np.inf
        if lo > gap * s[i] and hi > gap * s[i]:
            keep.append(i)
    return keep
