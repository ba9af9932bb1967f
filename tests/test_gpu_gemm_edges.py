"""csrc/gemm.h at the edges of its staging, its k-slices, its split-K hand-over and its epilogue, through the C ABI
(`Handle.gemm`, `Handle.gemm_ex`).  Every product is compared with the float64 product of the same operands, error over
max(|A| @ |B|) under the project's bars (float64 1e-13, float32 2e-6); the operands are chosen so that the bars can see the
mistake each group is about.  Shapes are the smallest that reach the branch named beside them.

* X3 terms: operands whose three bfloat16 pieces are known and positive (oracle/bf16x3_model.py); tests/test_bf16x3_model.py
  shows on the CPU model that each of the six terms left out, or al paired with bl, exceeds the bar at every shape used here.
  The same operands through XMCA_GEMM_BF16X3=0 (v_mfma_f32_16x16x4_f32) in a child process.
* ragged last k-row: a row-fast operand whose extent is no multiple of the 16-byte chunk and a contraction that ends on a
  k-tile: the last k-tile leaves the LDS-DMA path, whose last chunk would straddle the end of the operand.
* leading dimensions beyond the extent, padding filled with NaN; the whole-operand register path at ld * sizeof(T) * 128 = 2^32.
* float32 slices of 16 384 products and blocks of 512; split-K tickets, slab order, split counts above the k-tile count;
  mirror at tile edges; beta, row / column scales, ldc, float32 results.

XMCA_GEMM_EDGES_RECORD=<file>: the largest error over scale of every group is written there (scripts/gemm_edges_accuracy.py).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import bf16x3_model as X

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = {np.float64: 1e-13, np.float32: X.BAR}
BK = {np.float64: 16, np.float32: 32}            # k-tile of csrc/gemm.h: 128 bytes
CE = {np.float64: 2, np.float32: 4}              # elements of a 16-byte chunk
DTYPES = [np.float64, np.float32]
ORIENTATIONS = [(True, True), (True, False), (False, True), (False, False)]
FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _record_figures():
    yield
    dst = os.environ.get("XMCA_GEMM_EDGES_RECORD")
    if dst:
        with open(dst, "w") as f:
            json.dump(FIGURES, f, indent=1, sort_keys=True)


def _note(group, dtype, err):
    key = "%s/%s" % (group, np.dtype(dtype).name)
    FIGURES[key] = max(FIGURES.get(key, 0.0), float(err))


def _stored(A, B, a_kfast, b_nfast):
    return (A if a_kfast else np.ascontiguousarray(A.T)), (B if b_nfast else np.ascontiguousarray(B.T))


def _normal(rng, shape, dtype):
    return rng.standard_normal(shape).astype(dtype)


def _check(group, dtype, C, A, B, ctx, alpha=1.0, bar=None):
    """error of C against alpha * A @ B in float64, over max(|A| @ |B|) (times |alpha|): recorded, printed, asserted"""
    ref, scale = X.reference(A, B)
    err = float(np.max(np.abs(C - alpha * ref))) / (abs(alpha) * scale)
    _note(group, dtype, err)
    print("%s %s %s: %.3g" % (group, np.dtype(dtype).name, ctx, err))
    assert err < (BAR[dtype] if bar is None else bar), (group, ctx, err)     # (a NaN in C fails too)
    return err


# ------------------------------------------------------------------------------------------------
# the six terms of the three-way bfloat16 product
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def x3_results(hip):
    """every X3 product of oracle.bf16x3_model.device_calls on the device, once: key -> (C, A, B, keyword arguments)"""
    return {key: (hip.gemm(As, Bs, **kw), A, B, kw) for key, As, Bs, kw, A, B in X.device_calls()}


def test_x3_terms_are_all_there(x3_results):
    """measured on the MI355X: at most 1.81e-6 (one slice, K = 512: a whole block of 512 in the float32 accumulators) and 7.4e-7
    with the library's own slices; the smallest mutation of tests/test_bf16x3_model.py is 4.6e-6; a scratch build without
    XMCA_X3_TERM(ah, bl) fails here"""
    assert len(x3_results) == 4 * len(X.X3_SHAPES) + 2 * len(X.X3_GRAM_SHAPES)
    for key, (C, A, B, kw) in x3_results.items():
        _check("x3_terms", np.float32, C, A, B, key)
        if kw.get("mirror"):
            assert np.array_equal(C, C.T), key


X3_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oracle import bf16x3_model as X
from xmca_amd import _hip
h = _hip.Handle(0)
np.savez(sys.argv[2], **{key: h.gemm(As, Bs, **kw) for key, As, Bs, kw, A, B in X.device_calls()})
"""


def test_x3_operands_through_the_plain_float32_path_in_a_child(x3_results, tmp_path):
    """XMCA_GEMM_BF16X3 is read once per process: a fresh process runs the same calls on v_mfma_f32_16x16x4_f32.  Every result
    meets the bar; the calls that leave the slicing to the library also agree with the X3 result within 1e-6 of max |A||B|.

    The calls forced into one slice do not, and are not asked to: measured on the MI355X 2.7e-6 at (128, 128, 512), 2.4e-6 at
    (128, 128, 544) and the 129 x 544 Gram, 1.4e-6 at (5, 7, 16384), against at most 8.0e-7 with the library's slices.  A
    block of 512 all-positive products in float32 accumulators is at the limit of the bar in either path - gemm.h's own estimate
    is 1.3e-6 per block: the plain path measures +-1.35e-6 around a zero mean, X3 a mean of +0.9e-6 and at most 1.81e-6 (the
    rounding bias of its small terms, oracle/bf16x3_model.py) - so the two can differ by the sum, and no tighter agreement
    follows from the bar that each of them meets."""
    dst = str(tmp_path / "plain.npz")
    r = subprocess.run([sys.executable, "-c", X3_CHILD, REPO, dst], env=dict(os.environ, XMCA_GEMM_BF16X3="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plain = np.load(dst)
    assert sorted(plain.files) == sorted(x3_results)
    differs = False
    for key, (C, A, B, kw) in x3_results.items():
        P = plain[key]
        _check("x3_operands_plain_f32_path", np.float32, P, A, B, key)
        _, scale = X.reference(A, B)
        gap = float(np.max(np.abs(P - C))) / scale
        print("x3 against plain %s: %.3g" % (key, gap))
        if kw["splits"] == 0:
            _note("x3_against_plain_f32_path", np.float32, gap)
            assert gap < 1e-6, (key, gap)
        else:
            _note("x3_against_plain_f32_path_forced_into_one_slice", np.float32, gap)
        differs = differs or not np.array_equal(P, C)
    assert differs                                   # the child did take another path


# ------------------------------------------------------------------------------------------------
# staging: ragged last k-row, padded leading dimensions, whole-operand register path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("which", ["A", "B"])
def test_ragged_row_fast_operand_with_a_contraction_that_ends_on_a_k_tile(hip, dtype, which):
    """extent of the row-fast operand not a multiple of the chunk, K a multiple of the k-tile: at K = BK the decrement leaves
    no DMA tile at all; with splits=2 at K = 4 BK the last slice ends on a k-tile and the first stays on the DMA path.

    These shapes take the `--nfull` line of the kernel (ragged, kend == K, a whole number of k-tiles) and pin what comes out of
    the register staging that follows it.  They do not show that the line is needed: a scratch build without it passes them
    all on the MI355X - the range check of the 16-byte LDS-DMA clips a chunk that straddles the end of the operand per 4-byte
    word, so its valid elements arrive and the rest are zeros."""
    bk = BK[dtype]
    rng = np.random.default_rng(17 + bk + (which == "B"))
    extents = [1, 3, 37, 129, 131] if which == "A" else [1, 2, 3, 53, 131]
    for ext in extents:
        for K, splits in [(bk, 0), (2 * bk, 0), (3 * bk, 0), (4 * bk, 2)]:
            M, N = (ext, 40) if which == "A" else (37, ext)
            A, B = _normal(rng, (M, K), dtype), _normal(rng, (K, N), dtype)
            for other in (True, False):          # orientation of the other operand
                a_kfast, b_nfast = (False, other) if which == "A" else (other, True)
                As, Bs = _stored(A, B, a_kfast, b_nfast)
                C = hip.gemm(As, Bs, a_kfast=a_kfast, b_nfast=b_nfast, splits=splits)
                _check("ragged_last_k_row", dtype, C, A, B, (which, ext, K, splits, a_kfast, b_nfast))


def _padded(X2, pad):
    """X2 as the leading columns of a NaN-filled array that is `pad` wider -> (view, ld)"""
    buf = np.full((X2.shape[0], X2.shape[1] + pad), np.nan, dtype=X2.dtype)
    buf[:, :X2.shape[1]] = X2
    return buf[:, :X2.shape[1]], buf.shape[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("a_kfast,b_nfast", ORIENTATIONS)
def test_leading_dimensions_beyond_the_extent(hip, dtype, a_kfast, b_nfast):
    M, N, K = 37, 53, 48
    rng = np.random.default_rng(M + N + K)
    A, B = _normal(rng, (M, K), dtype), _normal(rng, (K, N), dtype)
    As, Bs = _stored(A, B, a_kfast, b_nfast)
    Av, lda = _padded(As, 5)
    Bv, ldb = _padded(Bs, 3)
    for splits in (0, 2):
        C = hip.gemm(Av, Bv, a_kfast=a_kfast, b_nfast=b_nfast, lda=lda, ldb=ldb, splits=splits)
        _check("padded_leading_dimensions", dtype, C, A, B, (a_kfast, b_nfast, lda, ldb, splits))
    with pytest.raises(ValueError):
        hip.gemm(Av, Bv, a_kfast=a_kfast, b_nfast=b_nfast, lda=lda + 1, ldb=ldb)      # not the stride of the array passed


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("which", ["A", "B"])
def test_whole_operand_register_path_at_its_threshold(hip, dtype, which):
    """ld * sizeof(T) * 128 = 2^32: tile offsets no longer fit the 32-bit DMA offsets and every k-tile is staged through
    registers; one element less is still the DMA path.  Two rows of the K-fast operand, the rest of each row NaN."""
    K, small, two = 40, 5, 2
    threshold = (1 << 32) // (128 * np.dtype(dtype).itemsize)
    assert threshold == {np.float64: 4194304, np.float32: 8388608}[dtype]
    rng = np.random.default_rng(threshold % 1000 + (which == "B"))
    M, N = (two, small) if which == "A" else (small, two)
    A, B = _normal(rng, (M, K), dtype), _normal(rng, (K, N), dtype)
    for ld in (threshold, threshold - 1):
        buf = np.full((two, ld), np.nan, dtype=dtype)
        for other in (True, False):
            if which == "A":
                buf[:, :K] = A
                As, Bs = _stored(A, B, True, other)
                C = hip.gemm(buf[:, :K], Bs, a_kfast=True, b_nfast=other, lda=ld)
            else:
                buf[:, :K] = B.T
                As, Bs = _stored(A, B, other, False)
                C = hip.gemm(As, buf[:, :K], a_kfast=other, b_nfast=False, ldb=ld)
            _check("register_path_threshold", dtype, C, A, B, (which, ld, other))
        del buf
    hip.trim_pool()


# ------------------------------------------------------------------------------------------------
# float32: slices of 16 384 products, blocks of 512
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16384, 16385, 16416, 32737, 32768])
@pytest.mark.parametrize("a_kfast", [True, False], ids=["x3", "native"])
def test_float32_slice_boundaries(hip, K, a_kfast):
    """contractions at, one element, one k-tile past, just below and at two slices; a large common offset as in
    test_gemm_f32_wide_accumulation and that test's measure and bar: max |C - ref| / max |ref| < 5e-7.  splits=1 is one slice
    where the length allows it (the library cuts longer contractions itself), splits=3 three slices."""
    rng = np.random.default_rng(K)
    A = (rng.standard_normal((5, K)) + 3.0).astype(np.float32)
    B = (rng.standard_normal((K, 7)) + 3.0).astype(np.float32)
    ref = A.astype(np.float64) @ B.astype(np.float64)
    As, Bs = _stored(A, B, a_kfast, True)
    for splits in (0, 3, 1):
        C = hip.gemm(As, Bs, a_kfast=a_kfast, b_nfast=True, splits=splits)
        err = float(np.max(np.abs(C - ref)) / np.max(np.abs(ref)))
        _note("float32_slices_rel_to_result", np.float32, err)
        print("float32_slices K=%d a_kfast=%d splits=%d: %.3g" % (K, a_kfast, splits, err))
        assert err < 5e-7, (K, a_kfast, splits, err)


# ------------------------------------------------------------------------------------------------
# split-K: tickets, slab order, split counts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_split_k_twice_is_bit_identical_and_leaves_the_tickets_at_zero(hip, dtype):
    rng = np.random.default_rng(777)
    Xg = _normal(rng, (129, 777), dtype)
    gram = dict(a_kfast=True, b_nfast=False, upper_only=True, mirror=1, splits=3)
    G1 = hip.gemm(Xg, Xg, **gram)
    G2 = hip.gemm(Xg, Xg, **gram)
    assert np.array_equal(G1, G2) and np.array_equal(G1, G1.T)
    _check("split_k", dtype, G1, Xg, np.ascontiguousarray(Xg.T), "gram 129x777 splits=3")
    A, B = _normal(rng, (200, 517), dtype), _normal(rng, (517, 130), dtype)
    C1 = hip.gemm(A, B, splits=4)
    C2 = hip.gemm(A, B, splits=4)
    assert np.array_equal(C1, C2)
    _check("split_k", dtype, C1, A, B, "200x130x517 splits=4")
    # other tile counts on the same workspace (1 and 9 tiles after 3 and 4): a ticket left above zero would end a tile early
    for M, N, K in [(37, 53, 64), (260, 300, 96)]:
        A, B = _normal(rng, (M, K), dtype), _normal(rng, (K, N), dtype)
        for a_kfast, b_nfast in [(True, True), (False, False)]:
            As, Bs = _stored(A, B, a_kfast, b_nfast)
            C = hip.gemm(As, Bs, a_kfast=a_kfast, b_nfast=b_nfast, splits=2)
            _check("split_k", dtype, C, A, B, ("after", M, N, K, a_kfast, b_nfast))
    assert np.array_equal(hip.gemm(Xg, Xg, **gram), G1)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("a_kfast,b_nfast", ORIENTATIONS)
def test_more_splits_than_k_tiles(hip, dtype, a_kfast, b_nfast):
    """splits=8 at K = 40: three k-tiles (float64) or two (float32) clip it; the result is that of the clipped count, bit for bit"""
    M, N, K = 37, 53, 40
    rng = np.random.default_rng(40)
    A, B = _normal(rng, (M, K), dtype), _normal(rng, (K, N), dtype)
    As, Bs = _stored(A, B, a_kfast, b_nfast)
    C = hip.gemm(As, Bs, a_kfast=a_kfast, b_nfast=b_nfast, splits=8)
    _check("split_k", dtype, C, A, B, ("splits=8", a_kfast, b_nfast))
    nkt = -(-K // BK[dtype])
    assert np.array_equal(C, hip.gemm(As, Bs, a_kfast=a_kfast, b_nfast=b_nfast, splits=nkt))


# ------------------------------------------------------------------------------------------------
# mirror at tile edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("T", [127, 128, 256, 257])
def test_mirror_at_tile_edges(hip, dtype, T):
    N = 96
    rng = np.random.default_rng(T)
    Xf, Yf = _normal(rng, (T, N), dtype), _normal(rng, (T, N), dtype)
    iu = np.triu_indices(T, 1)
    block_upper = iu[0] // 128 != iu[1] // 128          # strictly upper BLOCK tiles are mirrored with the sign
    diag_tile = np.arange(T)[:, None] // 128 == np.arange(T)[None, :] // 128
    for splits in (0, 2):
        G = hip.gemm(Xf, Xf, a_kfast=True, b_nfast=False, upper_only=True, mirror=1, splits=splits)
        assert np.array_equal(G, G.T), (T, splits)
        _check("mirror", dtype, G, Xf, np.ascontiguousarray(Xf.T), ("+1", T, splits))
        H = hip.gemm(Xf, Yf, a_kfast=True, b_nfast=False, upper_only=True, mirror=-1, splits=splits)
        ref, scale = X.reference(Xf, np.ascontiguousarray(Yf.T))
        seen = diag_tile | np.triu(np.ones((T, T), dtype=bool))     # diagonal tiles whole, the others above the diagonal
        err = float(np.max(np.abs(H - ref)[seen])) / scale
        _note("mirror", dtype, err)
        assert err < BAR[dtype], ("-1", T, splits, err)
        assert np.array_equal(H.T[iu][block_upper], -H[iu][block_upper]), (T, splits)


# ------------------------------------------------------------------------------------------------
# epilogue options (xmca_gemm_ex)
# ------------------------------------------------------------------------------------------------
def _epilogue_check(dtype, got, A, B, ctx, alpha=1.0, beta=0.0, C0=None, rs=None, cs=None):
    """against alpha * rs[m] * cs[n] * (A @ B) + beta * C0 in float64, over the largest alpha * rs[m] * cs[n] * (|A| @ |B|)[m, n]"""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    M, N = A.shape[0], B.shape[1]
    w = abs(alpha) * np.abs(np.ones(M) if rs is None else rs)[:, None] * np.abs(np.ones(N) if cs is None else cs)[None, :]
    f = alpha * (np.ones(M) if rs is None else rs)[:, None] * (np.ones(N) if cs is None else cs)[None, :]
    ref = f * (A64 @ B64) + (beta * C0.astype(np.float64) if beta != 0.0 else 0.0)
    scale = float(np.max(w * (np.abs(A64) @ np.abs(B64))))
    err = float(np.max(np.abs(got.astype(np.float64) - ref))) / scale
    _note("epilogue", dtype, err)
    print("epilogue %s %s: %.3g" % (np.dtype(dtype).name, ctx, err))
    assert err < BAR[dtype], (ctx, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("M,N,K", [(130, 67, 48), (129, 129, 80)])
def test_epilogue_beta_scales_and_ldc(hip, dtype, M, N, K):
    rng = np.random.default_rng(M + N + K)
    A, B = _normal(rng, (M, K), dtype), _normal(rng, (K, N), dtype)
    C0 = rng.standard_normal((M, N))
    rs, cs = rng.uniform(0.5, 2.0, M) * rng.choice([-1.0, 1.0], M), rng.uniform(0.5, 2.0, N)
    for a_kfast, b_nfast in ORIENTATIONS:
        As, Bs = _stored(A, B, a_kfast, b_nfast)
        kw = dict(a_kfast=a_kfast, b_nfast=b_nfast)
        for beta in (0.0, 1.0, -0.5):
            got = hip.gemm_ex(As, Bs, C0, alpha=0.75, beta=beta, **kw)
            _epilogue_check(dtype, got, A, B, (kw, "beta", beta), alpha=0.75, beta=beta, C0=C0)
        for r, c in [(rs, None), (None, cs), (rs, cs)]:
            got = hip.gemm_ex(As, Bs, C0, beta=-0.5, row_scale=r, col_scale=c, **kw)
            _epilogue_check(dtype, got, A, B, (kw, "scales", r is not None, c is not None), beta=-0.5, C0=C0, rs=r, cs=c)
        # beta = 0: what C held is not read - NaN does not leak; padded rows: the padding comes back as it went in
        got = hip.gemm_ex(As, Bs, np.full((M, N), np.nan), row_scale=rs, **kw)
        _epilogue_check(dtype, got, A, B, (kw, "nan C"), rs=rs)
        Cp = rng.standard_normal((M, N + 3))
        got = hip.gemm_ex(As, Bs, Cp, beta=1.0, col_scale=cs, **kw)
        assert got.shape == Cp.shape and np.array_equal(got[:, N:], Cp[:, N:]), kw
        _epilogue_check(dtype, got[:, :N], A, B, (kw, "ldc"), beta=1.0, C0=Cp[:, :N], cs=cs)
        got2 = hip.gemm_ex(As, Bs, Cp, beta=1.0, col_scale=cs, splits=2, **kw)
        assert np.array_equal(got2[:, N:], Cp[:, N:]), kw
        _epilogue_check(dtype, got2[:, :N], A, B, (kw, "beta=1 splits=2"), beta=1.0, C0=Cp[:, :N], cs=cs)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_epilogue_beta_with_the_mirror_on_a_symmetric_matrix(hip, dtype):
    """the rank-K update of a symmetric matrix (the Cholesky updates): upper tiles only, mirrored.  (upper_only needs a square
    result: the 129 x 129 shape only.)"""
    T, K = 129, 80
    rng = np.random.default_rng(T + K)
    Xf = _normal(rng, (T, K), dtype)
    S = rng.standard_normal((T, T))
    S = S + S.T
    for splits in (0, 2):
        got = hip.gemm_ex(Xf, Xf, S, b_nfast=False, alpha=-1.0, beta=1.0, upper_only=True, mirror=1, splits=splits)
        assert np.array_equal(got, got.T), splits
        _epilogue_check(dtype, got, Xf, np.ascontiguousarray(Xf.T), ("mirror", splits), alpha=-1.0, beta=1.0, C0=S)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("M,N,K", [(130, 67, 48), (129, 129, 80)])
def test_float32_result_is_the_float64_result_rounded(hip, dtype, M, N, K):
    rng = np.random.default_rng(M * N + K)
    A, B = _normal(rng, (M, K), dtype), _normal(rng, (K, N), dtype)
    C0 = rng.standard_normal((M, N + 3)).astype(np.float32)
    rs = rng.uniform(0.5, 2.0, M)
    for a_kfast, b_nfast in ORIENTATIONS:
        As, Bs = _stored(A, B, a_kfast, b_nfast)
        for beta, splits in [(0.0, 0), (-0.5, 0), (1.0, 2)]:
            kw = dict(a_kfast=a_kfast, b_nfast=b_nfast, alpha=0.75, beta=beta, row_scale=rs, splits=splits)
            wide = hip.gemm_ex(As, Bs, C0.astype(np.float64), **kw)
            narrow = hip.gemm_ex(As, Bs, C0, **kw)
            assert narrow.dtype == np.float32 and np.array_equal(narrow[:, N:], C0[:, N:]), kw
            want = wide[:, :N].astype(np.float32)
            ulps = np.abs(narrow[:, :N].astype(np.float64) - want) / np.spacing(np.abs(want)).astype(np.float64)
            _note("float32_result_ulps", dtype, ulps.max())
            assert ulps.max() <= 1.0, (kw, ulps.max())
