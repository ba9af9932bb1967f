"""Field-side kernels through `_hip.Handle` against plain float64 numpy references, at the shapes where their work
decomposition changes: 256 columns per workgroup, COL_CHUNKS = 32 row chunks of ceil(T / min(32, T)) rows, `ew_grid`'s cap of
8192 blocks of 256 (grid-stride above T N = 2 097 152), the 8-column groups of `eof_mix_kernel` and the 32 x 32 tiles of
`eof_transpose_kernel` (xmca_amd/csrc/kernels.h).  Copies are checked bit for bit; every tolerance states its reason."""
import numpy as np
import pytest

from xmca_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
GRID_STRIDE = 8192 * 256                       # elements beyond which the elementwise kernels loop grid-stride


@pytest.fixture(scope="module")
def h():
    handle = _hip.Handle(0)
    yield handle
    handle.close()


def _bits(a):
    """the bit patterns of a float array (NaN == NaN, -0 != +0)"""
    a = np.ascontiguousarray(a)
    if np.iscomplexobj(a):
        a = a.view(a.real.dtype)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _per(T):
    """rows per chunk of the column kernels"""
    return -(-T // min(32, T))


# ----------------------------------------------------------------------------------------------
# a. constructor preprocessing: set_field -> compact_field -> center_field -> scale_field -> get_field
# ----------------------------------------------------------------------------------------------
def _nan_placements(T, N):
    """name -> list of (row or None for the whole column, column)"""
    per = _per(T)
    last = N - 1
    out = {"none": []}
    if N > 1:
        out["columns"] = [(None, 0), (None, N // 2)] + ([(None, last)] if N > 2 else [])
    for name, row in (("row0", 0), ("row_per-1", per - 1), ("row_per", min(per, T - 1)), ("row_T-1", T - 1)):
        out[name] = [(row, last)] + ([(row, min(255, last - 1))] if N > 1 else [])
    out["every"] = [(None, c) for c in range(N)]
    return out


def _field(rng, T, N, dtype, nans=(), offset=0.0, scale=1.0):
    X = (offset + scale * rng.standard_normal((T, N))).astype(dtype)
    for r, c in nans:
        if r is None:
            X[:, c] = np.nan
        else:
            X[r, c] = np.nan
    return X


def _moments_ref(Xk):
    """column mean and (two-pass, ddof 0) std in extended precision, rounded to float64"""
    x = Xk.astype(np.longdouble)
    mean = x.sum(axis=0) / x.shape[0]
    std = np.sqrt(((x - mean) ** 2).sum(axis=0) / x.shape[0])
    return mean.astype(np.float64), std.astype(np.float64)


def _check_centered(X, mean, std, Xc):
    """X: the raw NaN-free columns; mean / std / Xc: what the device returned for them"""
    dtype = X.dtype
    mref, sref = _moments_ref(X)
    amax = np.max(np.abs(X.astype(np.float64)), axis=0)
    # float64 sums over at most 1000 rows: a few eps of the largest entry; 1e-14 leaves room and still sees a one-pass std
    assert np.all(np.abs(mean - mref) <= 1e-14 * amax), np.max(np.abs(mean - mref) / amax)
    assert np.all(np.abs(std - sref) <= 1e-14 * amax), np.max(np.abs(std - sref) / amax)
    ref = (X.astype(np.float64) - mref).astype(dtype)
    err = np.abs(Xc.astype(np.float64) - ref.astype(np.float64))
    if dtype == np.float32:
        # the device rounds float64(x) - mean once to float32: its mean is off by eps64 |x| at most, so 1 ulp of the result
        ulp = np.spacing(np.maximum(np.abs(ref), np.abs(Xc))).astype(np.float64)
        assert np.all(err <= ulp), np.max(err / ulp)
    else:
        # x - mean in float64 with the two means a few eps |x| apart
        assert np.all(err <= 4 * np.finfo(np.float64).eps * amax), np.max(err / amax)


def _preprocess_and_check(h, X, w=None):
    T, N = X.shape
    dtype = X.dtype
    h.set_field(0, X)
    keep, nk = h.compact_field(0, N)
    ref_keep = ~np.isnan(X).any(axis=0)
    assert np.array_equal(keep, ref_keep)
    assert nk == int(ref_keep.sum())
    if nk == 0:                                    # nothing left: the field stays as it was, the caller reports it
        assert _same_bits(h.get_field(0, (T, N), dtype), X)
        return
    Xk = np.ascontiguousarray(X[:, ref_keep])
    assert _same_bits(h.get_field(0, (T, nk), dtype), Xk)       # the kept columns, in order, bit for bit
    mean, std, n_nan = h.center_field(0, nk)
    assert n_nan == 0
    Xc = h.get_field(0, (T, nk), dtype)
    _check_centered(Xk, mean, std, Xc)
    if w is not None:
        wk = np.ascontiguousarray(w[ref_keep].astype(dtype))
        for divide in (0, 1):
            h.scale_field(0, wk, divide=divide)
            got = h.get_field(0, (T, nk), dtype)
            # the kernel applies the host's own operation in the field's dtype: bit for bit
            ref = Xc / wk if divide else Xc * wk
            assert _same_bits(got, ref.astype(dtype)), divide
            Xc = got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [2, 3, 31, 32, 33, 65, 1000])
def test_preprocessing_at_chunk_and_workgroup_edges(h, dtype, T):
    rng = np.random.default_rng(T)
    for N in (1, 255, 256, 257):
        w = rng.uniform(0.3, 3.0, N)
        for name, nans in _nan_placements(T, N).items():
            X = _field(rng, T, N, dtype, nans, offset=rng.uniform(-5, 5), scale=rng.uniform(0.5, 4.0))
            try:
                _preprocess_and_check(h, X, w if name in ("none", "columns") else None)
            except AssertionError as e:
                raise AssertionError("N=%d nan=%s: %s" % (N, name, e)) from e


@pytest.mark.parametrize("dtype", DTYPES)
def test_preprocessing_offset_field_needs_a_two_pass_std(h, dtype):
    """mean 300, std 1e-2: a one-pass (sum x^2 - T mean^2) std loses (300 / 1e-2)^2 eps ~ 1e-7 relative"""
    rng = np.random.default_rng(300)
    X = _field(rng, 1000, 257, dtype, [(None, 3), (500, 100)], offset=300.0, scale=1e-2)
    _preprocess_and_check(h, X, rng.uniform(0.3, 3.0, 257))


@pytest.mark.parametrize("dtype", DTYPES)
def test_preprocessing_grid_stride(h, dtype):
    """T N = 2.3e6 > 8192 * 256: gather_columns / scale_columns loop grid-stride; NaN columns in the last workgroup too"""
    T, N = 33, 70_001
    assert T * N > GRID_STRIDE
    rng = np.random.default_rng(70001)
    nans = [(None, 0), (None, 12345), (None, N - 1), (0, 256), (_per(T), 40_000), (T - 1, N - 2)]
    _preprocess_and_check(h, _field(rng, T, N, dtype, nans, offset=2.0), rng.uniform(0.3, 3.0, N))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [3, 33, 1000])
def test_center_field_with_nan_columns_left_in(h, dtype, T):
    """without compact_field: the NaN-free columns are centered, the NaN columns come back bit-unchanged with NaN mean and
    std, and the count is the number of NaN entries"""
    rng = np.random.default_rng(T + 7)
    N = 257
    per = _per(T)
    nans = [(None, 1), (0, 256), (per - 1, 100), (min(per, T - 1), 255), (T - 1, 0), (T - 1, 256)]
    X = _field(rng, T, N, dtype, nans, offset=1.5)
    h.set_field(0, X)
    mean, std, n_nan = h.center_field(0, N)
    bad = np.isnan(X).any(axis=0)
    assert n_nan == int(np.isnan(X).sum())
    assert np.all(np.isnan(mean[bad])) and np.all(np.isnan(std[bad]))
    Xc = h.get_field(0, (T, N), dtype)
    assert _same_bits(np.ascontiguousarray(Xc[:, bad]), np.ascontiguousarray(X[:, bad]))
    _check_centered(np.ascontiguousarray(X[:, ~bad]), mean[~bad], std[~bad], np.ascontiguousarray(Xc[:, ~bad]))


def test_float32_field_promoted_by_complexify_extended_comes_back_exactly(h):
    rng = np.random.default_rng(5)
    X = _field(rng, 33, 257, np.float32, offset=3.0)
    h.set_field(0, X)
    h.complexify_extended(33, 12.0)
    assert h.field_dtype == np.float64                   # resident in float64 now
    assert _same_bits(h.get_field(0, (33, 257), np.float32), X)


# ----------------------------------------------------------------------------------------------
# b. correlate: column moments + GEMM + pearson_finish_kernel
# ----------------------------------------------------------------------------------------------
def _pearson_ref(X, Y):
    """corr(X[:, n], Y[:, j]) in float64 from the test's own inputs, clipped like np.corrcoef (tools/array.py:pearsonr)"""
    a = X.astype(np.float64)
    b = Y.astype(np.float64)
    a = a - a.mean(axis=0)
    b = b - b.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (a.T @ b) / np.outer(np.sqrt((a * a).sum(axis=0)), np.sqrt((b * b).sum(axis=0)))
    return np.clip(r, -1, 1)


def _centered(rng, T, N, dtype):
    X = rng.standard_normal((T, N)) * rng.uniform(0.1, 10.0, N)
    return (X - X.mean(axis=0)).astype(dtype)


# float64: X^T Y in the float64 GEMM, ~T eps.  float32: Y is rounded to float32 for the GEMM (~6e-8 relative), so r moves by
# ~1e-7; 2e-6 leaves the GEMM's float32 products room and stays far inside the model-level 2e-5.
R_TOL = {np.float64: 1e-12, np.float32: 2e-6}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [3, 33, 1000])
def test_correlate_matches_pearson(h, dtype, T):
    rng = np.random.default_rng(T + 11)
    worst = 0.0
    for N in (1, 255, 257, 4097):
        X = _centered(rng, T, N, dtype)
        h.set_field(0, X)
        for m in (1, 3, 17):
            Y = rng.standard_normal((T, m)) * 2.0 + rng.uniform(-3, 3, m)       # PCs with a nonzero mean as well
            r = h.correlate(0, Y, N)
            ref = _pearson_ref(X, Y)
            err = np.max(np.abs(r - ref))
            worst = max(worst, err)
            assert r.shape == (N, m) and np.all(np.abs(r) <= 1)
            assert err < R_TOL[dtype], (N, m, err)
    if T > 3:
        assert np.allclose(_pearson_ref(X[:, :40], Y), np.corrcoef(X[:, :40].astype(np.float64), Y, rowvar=False)[:40, 40:],
                           rtol=0, atol=1e-13)


@pytest.mark.parametrize("dtype", DTYPES)
def test_correlate_grid_stride(h, dtype):
    """N m = 2.2e6 > 8192 * 256: pearson_finish_kernel loops grid-stride"""
    T, N, m = 33, 130_001, 17
    assert N * m > GRID_STRIDE
    rng = np.random.default_rng(17)
    X = _centered(rng, T, N, dtype)
    Y = rng.standard_normal((T, m)) + 1.0
    h.set_field(0, X)
    r = h.correlate(0, Y, N)
    assert np.all(np.abs(r) <= 1)
    assert np.max(np.abs(r - _pearson_ref(X, Y))) < R_TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,N", [(3, 2), (33, 257), (1000, 255)])
def test_correlate_perfectly_correlated_and_constant_columns(h, dtype, T, N):
    """Y[:, j] = +-a X[:, c]: |r| = 1 and never beyond (the GEMM and the column moments sum in different orders; the
    kernel clamps like np.corrcoef).  An all-zero column of Y or of the field gives NaN, which the clamp keeps."""
    rng = np.random.default_rng(T * N)
    X = _centered(rng, T, N, dtype)
    X[:, N - 1] = 0
    h.set_field(0, X)
    cols = [0, N // 2, max(N - 2, 0)]
    scales = [1.0, 3.0, 1e-3, 7.5e4, 0.1]
    Y, pairs = [], []
    for c in cols:
        for a in scales:
            for s in (1.0, -1.0):
                pairs.append((c, s, len(Y)))
                Y.append(s * a * X[:, c].astype(np.float64))
    Y.append(np.zeros(T))
    Y.append(rng.standard_normal(T) + 4.0)
    Y = np.stack(Y, axis=1)
    r = h.correlate(0, Y, N)
    zero_y = Y.shape[1] - 2
    finite_x = np.ones(N, dtype=bool)
    finite_x[N - 1] = False
    assert np.all(np.isnan(r[:, zero_y]))                   # constant PC
    assert np.all(np.isnan(r[N - 1, :]))                    # constant grid point
    ok = np.abs(r[~np.isnan(r)])
    assert np.all(ok <= 1)
    # float64: the pair is exactly proportional, r = +-1 to rounding; float32: Y is rounded to float32 for the GEMM
    tol = 1e-14 if dtype == np.float64 else R_TOL[np.float32]
    for c, s, j in pairs:
        if finite_x[c]:
            assert abs(r[c, j] - s) <= tol, (c, s, r[c, j] - s)
    ref = _pearson_ref(X, Y)
    both = finite_x[:, None] & ~np.isnan(ref)
    assert np.array_equal(np.isnan(r), np.isnan(ref))
    assert np.max(np.abs(r[both] - ref[both])) < R_TOL[dtype]


# ----------------------------------------------------------------------------------------------
# c. eofs: eof_transpose_kernel (W = None) and eof_mix_kernel
# ----------------------------------------------------------------------------------------------
def _solved(h, kind, T, N, seed):
    """solve one field of `kind` on the handle; returns its rank"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, N)) * (0.98 ** np.arange(N))
    if kind == "complex":
        X = X + 1j * rng.standard_normal((T, N)) * (0.98 ** np.arange(N))
    elif kind == "f32":
        X = X.astype(np.float32)
    h.set_field(0, X)
    rank = h.solve(1)
    assert bool(h._lib.xmca_is_complex(h._h)) == (kind == "complex")
    if kind == "f32" and N > T:
        assert h.vectors_are_f32(0)                         # real float32 field, dual side: vectors resident in float32
    return rank


EOF_SOLVES = [("real", 64, 31), ("real", 64, 32), ("real", 64, 33), ("real", 40, 257), ("complex", 70, 33), ("complex", 40, 257),
              ("f32", 40, 257), ("f32", 20, 33)]


@pytest.mark.parametrize("kind,T,N", EOF_SOLVES)
def test_eofs_transpose_is_an_exact_copy(h, kind, T, N):
    rank = _solved(h, kind, T, N, seed=N)
    tested = 0
    for q in (1, 31, 32, 33):
        if q > rank:
            continue
        for dt in DTYPES:
            got = h.eofs(0, N, q, None, dt)
            assert _same_bits(got, np.ascontiguousarray(h.vectors(0, q, N, dt).T)), (q, dt)
            tested += 1
    assert tested >= 2


def _mix_ref(V64, W):
    """V[:, :m] @ W in extended precision; elementwise scale |V| |W|"""
    cplx = np.iscomplexobj(V64) or np.iscomplexobj(W)
    ld = np.clongdouble if cplx else np.longdouble
    ref = (V64.astype(ld) @ W.astype(ld)).astype(np.complex128 if cplx else np.float64)
    return ref, np.abs(V64) @ np.abs(W)


@pytest.mark.parametrize("kind,T,N", [("real", 64, 33), ("real", 40, 257), ("complex", 40, 257), ("f32", 40, 257)])
def test_eofs_mix_matches_float64_product(h, kind, T, N):
    rank = _solved(h, kind, T, N, seed=N + 1)
    rng = np.random.default_rng(rank)
    for q in (1, 7, 8, 9, 17):
        for m in sorted({1, 2, 8, 9, rank // 2, rank}):
            V64 = np.ascontiguousarray(h.vectors(0, m, N, np.float64).T)
            for w_cplx in (False, True):
                W = rng.standard_normal((m, q)) + (1j * rng.standard_normal((m, q)) if w_cplx else 0)
                ref, scale = _mix_ref(V64, W)
                for dt in DTYPES:
                    got = h.eofs(0, N, m, W, dt)
                    ctx = (q, m, w_cplx, dt)
                    assert got.shape == (N, q) and np.iscomplexobj(got) == np.iscomplexobj(ref), ctx
                    if dt == np.float64:
                        # m float64 products summed once: m eps |V||W| at most, m <= 64
                        assert np.all(np.abs(got - ref) <= 1e-14 * scale), ctx
                    else:
                        # one rounding of the float64 sum: 1 float32 ulp (plus the float64 bar where the sum cancels)
                        r32 = ref.astype(got.dtype)
                        for g, rr, sc in ((got.real, r32.real, scale), (got.imag, r32.imag, scale)) if np.iscomplexobj(got) \
                                else ((got, r32, scale),):
                            bound = np.spacing(np.abs(rr)).astype(np.float64) + 1e-14 * sc
                            assert np.all(np.abs(g.astype(np.float64) - rr.astype(np.float64)) <= bound), ctx


@pytest.mark.parametrize("kind,T,N", [("real", 64, 33), ("complex", 40, 257), ("f32", 40, 257)])
def test_eofs_selection_matrix_is_exact(h, kind, T, N):
    """`_eofs_from_device` sends np.eye(m)[:, keep] for eofs(slice(2, None)) and the like: the selected vectors, exactly"""
    rank = _solved(h, kind, T, N, seed=N + 2)
    for m in (3, 9, rank):
        for keep in (slice(2, None), [0, m - 1], [m - 1]):
            W = np.eye(m)[:, keep]
            for dt in DTYPES:
                got = h.eofs(0, N, m, W, dt)
                ref = np.ascontiguousarray(h.vectors(0, m, N, dt).T[:, keep])
                assert _same_bits(got, ref), (m, keep, dt)


# ----------------------------------------------------------------------------------------------
# d. project: U = X~ V on the resident field
# ----------------------------------------------------------------------------------------------
def _project_ref(X, V, analytic):
    """X~ @ V in float64 and its elementwise scale; X~ = X + i H X with H the circulant of `hilbert_imag_column`"""
    X = X.astype(np.float64)
    if analytic:
        H = _hip.hilbert_imag_operator(X.shape[0])
        HX = H @ X
        return (X + 1j * HX) @ V, (np.abs(X) + np.abs(H) @ np.abs(X)) @ np.abs(V)
    return X @ V, np.abs(X) @ np.abs(V)


# float64: one GEMM (+ one T x T GEMM for the analytic signal); float32: field and V in float32 for the GEMM (~6e-8 each)
P_TOL = {np.float64: 1e-13, np.float32: 2e-6}


def _check_project(h, X, V, analytic):
    T, N = X.shape
    got = h.project(0, V, T)
    ref, scale = _project_ref(X, V, analytic)
    assert got.shape == ref.shape and np.iscomplexobj(got) == np.iscomplexobj(ref)
    err = np.abs(got - ref) / scale
    assert np.max(err) < P_TOL[X.dtype.type], np.max(err)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [3, 33, 130])
@pytest.mark.parametrize("N", [1, 257, 5000])
def test_project_real_complex_and_implicit_analytic(h, dtype, T, N):
    rng = np.random.default_rng(T * 10 + N)
    X = (rng.standard_normal((T, N)) + 0.5).astype(dtype)
    for m in (1, 9):
        Vr = rng.standard_normal((N, m))
        Vc = Vr + 1j * rng.standard_normal((N, m))
        h.set_field(0, X)
        _check_project(h, X, Vr, False)                     # real field, real V
        _check_project(h, X, Vc, False)                     # real field, complex V
        h.complexify(T)                                     # before any solve: U = W + i Ht W with W = X V
        _check_project(h, X, Vr, True)
        _check_project(h, X, Vc, True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,N", [(33, 1), (130, 1), (130, 100), (33, 33)])
def test_project_after_solve_with_explicit_imaginary_planes(h, dtype, T, N):
    """N <= T: `Solver::analytic_route` is false, so solve() forms X_im = Ht X on the device and project() uses the
    stored planes"""
    rng = np.random.default_rng(T + N)
    X = rng.standard_normal((T, N)).astype(dtype)
    X = (X - X.mean(axis=0)).astype(dtype)
    h.set_field(0, X)
    h.complexify(T)
    h.solve(1)
    assert h._lib.xmca_is_complex(h._h) == 1
    for m in (1, 9):
        _check_project(h, X, rng.standard_normal((N, m)), True)
        _check_project(h, X, rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m)), True)
