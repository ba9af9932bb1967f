"""GPU: the consumers of the chunked column pass (xmca_amd/csrc/column_pass.h) at the edges of its row cut - one row per chunk, a
short last chunk, empty trailing chunks - and on both sides of the 256 columns of a workgroup.  The restatement and the shapes:
tests/column_pass_cases.py.  Where a result is a quotient of chunked sums it is compared bit for bit."""
import numpy as np
import pytest

import column_pass_cases as P
import extended_eofs_cases as E

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
IDS = {np.float64: "f64", np.float32: "f32"}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS.get)
@pytest.mark.parametrize("rows", P.ROWS)
def test_center_field_mean_is_the_chunked_sum_over_rows(hip, rows, dtype):
    for cols in P.COLS:
        X = P.field(rows, cols, dtype, 1)
        hip.set_field(0, X)
        mean, std, n_nan = hip.center_field(0, cols)
        assert n_nan == 0
        assert np.array_equal(_bits(mean), _bits(P.chunked_sum(X.astype(np.float64)) / rows)), cols


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS.get)
@pytest.mark.parametrize("rows", (1,) + P.ROWS)
def test_gap_center_at_the_chunk_edges(hip, rows, dtype):
    for cols in P.COLS:
        X = P.with_gaps(P.field(rows, cols, dtype, 2))
        present = ~np.isnan(X)
        assert present.any(axis=0).all()
        X64 = X.astype(np.float64)
        mean, mask, A, scale = hip.gap_center(X)
        count = present.sum(axis=0)
        assert np.array_equal(_bits(mean), _bits(P.chunked_sum(X64, where=present) / count)), cols
        assert mask.dtype == np.uint8 and np.array_equal(mask, np.isnan(X).astype(np.uint8)), cols
        with np.errstate(invalid="ignore"):
            ref = np.where(present, (X64 - mean).astype(dtype).astype(np.float64), 0.0)
        assert np.array_equal(_bits(A), _bits(ref)), cols
        # the scale as tests/test_gpu_fill_gaps.py bounds it: a float64 sum of squares of values stored in the field's dtype,
        # around column means that are off by `bound` at most
        xl = np.where(present, X64, 0.0).astype(np.longdouble)
        al = np.where(present, xl - xl.sum(axis=0) / count, 0.0)
        ref_scale = float(np.sqrt((al * al).sum() / present.sum()))
        eps = float(np.finfo(dtype).eps)
        bound = count * U * np.nanmax(np.abs(X64), axis=0)
        tol = ref_scale * (present.sum() * U + 2 * eps) + 2 * bound.max()
        print("gap_center scale rows %d cols %d %s: %.3e (bound %.3e)" % (rows, cols, IDS[dtype], abs(scale - ref_scale), tol))
        assert abs(scale - ref_scale) <= tol, cols


def _real_gram(n, seed):
    X = P.field(n, 17, np.float64, seed)            # (not centred: the column means of K are far from zero)
    G = X @ X.T
    return (G + G.T) / 2


@pytest.mark.parametrize("Tp,M,tau", [(Tp, 1, 1) for Tp in (1,) + P.ROWS] + [(33, 3, 2)])
def test_lag_gram_centring_at_the_chunk_edges(hip, Tp, M, tau):
    """symmetric to the bit (the sum of the two means commutes), and float64 double centring within the bound of
    tests/test_gpu_extended_eofs.py for this entry: (T' + M) 2^-52 max|K|"""
    G = _real_gram(Tp + (M - 1) * tau, 5)
    K = E.lag_sum(G, M, tau)
    Kc = hip.lag_gram(G, M, tau, True)
    assert Kc.shape == (Tp, Tp)
    assert np.array_equal(_bits(Kc), _bits(Kc.T))
    bound = (Tp + M) * 2.0 ** -52 * np.abs(K).max()
    err = np.abs(Kc - E.double_center(K)).max()
    print("lag_gram T' = %d, M = %d, tau = %d: error %.3g, bound %.3g" % (Tp, M, tau, err, bound))
    assert err <= bound


def _std_ref(X):
    """two-pass sample standard deviation (ddof = 1) of the columns in extended precision"""
    x = X.astype(np.longdouble)
    d = x - x.sum(axis=0) / x.shape[0]
    return np.sqrt((d * d).sum(axis=0) / (x.shape[0] - 1)).astype(np.float64)


def _column_scale(hip, X):
    """d of `extended_rule_n` alone: M = 1, one mode, no surrogate (run_begin == run_end)"""
    T, N = X.shape
    hip.set_field(0, X)
    lam, d, runs = hip.extended_rule_n(T, N, 1, 1, 1, np.zeros(N), 0, 0, 0)
    assert runs.shape == (0, 1)
    return d


def _check_scale(X, d):
    # a two-pass float64 sum over at most 65 rows: (T + 3) 2^-53 < 1e-14 relative, the room `_check_centered` of
    # tests/test_gpu_field_kernels.py gives the same kind of sum (there against the largest entry: the smaller of the two here)
    ref = _std_ref(X)
    room = 1e-14 * np.minimum(ref, np.max(np.abs(X.astype(np.float64)), axis=0))
    err = np.abs(d - ref)
    print("column scale %s %s: %.3e of the room" % (X.shape, X.dtype, np.max(err / room)))
    assert np.all(err <= room)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS.get)
@pytest.mark.parametrize("rows", P.ROWS)
def test_column_scale_of_extended_rule_n_at_the_chunk_edges(hip, rows, dtype):
    for cols in P.COLS:
        X = P.field(rows, cols, dtype, 3)
        _check_scale(X, _column_scale(hip, X))


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS.get)
def test_column_scale_of_an_offset_field_needs_two_passes(hip, dtype):
    """mean 300, spread 1e-2: a one-pass (sum x^2 - T mean^2) formula loses (300 / 1e-2)^2 eps ~ 1e-7 relative"""
    X = P.field(65, 257, dtype, 4, offset=300.0, spread=1e-2)
    _check_scale(X, _column_scale(hip, X))
