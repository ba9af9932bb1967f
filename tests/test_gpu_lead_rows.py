"""The skinny product behind the leading modes of a one-field solve (csrc/kernels.h lead_rows, through xmca_lead_rows):
out (rows <= 16, n) = A (rows, K) B in float64, B read once in either orientation, the contraction cut over the waves of a
workgroup and over workgroups and summed in a fixed order.

Reference: float64 numpy `A @ B`.  Tolerance per element: C * K * 2**-53 * sum_k |a||b| (times |scale|) with C = 4.  The kernel
rounds once per addition (fused multiply-adds: K roundings, the sums of the waves and chunks among them) and once for the row
scale (K + 1), numpy once per product, per addition and for the scale (2 K): 3 K + 1 roundings, each of a value bounded by the
sum of the |a||b|, so C = 4 covers both sides for every K >= 1.  Two calls on the same input must agree bit for bit: no
atomics, no order that depends on the scheduling."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C_TOL = 4.0
KS = (1, 63, 64, 65, 1000)
NS = (1, 63, 64, 65, 1001)
ROWS = (1, 10, 16)
PAD = 5                      # odd: padded rows are not 16-byte aligned


def _operands(rows, K, n, b_kfast, padded, seed):
    """A (rows, lda), B in the kernel's orientation with ldb, NaN in every padding column: a read outside the operand shows"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((rows, K))
    b = rng.standard_normal((K, n))                       # b[k, j] = B(k, j)
    pad = PAD if padded else 0
    A = np.full((rows, K + pad), np.nan)
    A[:, :K] = a
    if b_kfast:
        B = np.full((n, K + pad), np.nan)
        B[:, :K] = b.T
    else:
        B = np.full((K, n + pad), np.nan)
        B[:, :n] = b
    return a, b, A, B


@pytest.mark.parametrize("with_scale", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("padded", [False, True], ids=["dense", "padded"])
@pytest.mark.parametrize("b_kfast", [True, False], ids=["B_k_fast", "B_n_fast"])
def test_lead_rows_match_numpy_and_repeat_bit_for_bit(hip, b_kfast, padded, with_scale):
    cut = set()
    for K in KS:
        for n in NS:
            for rows in ROWS:
                a, b, A, B = _operands(rows, K, n, b_kfast, padded, seed=1000 * K + 10 * n + rows)
                scale = np.random.default_rng(rows).uniform(0.5, 2.0, rows) if with_scale else None
                out0 = np.full((rows, n + (PAD if padded else 0)), -7.0)       # sentinel: the padding must come back as it went
                got, chunks = hip.lead_rows(A, B, b_kfast, K, n, scale=scale, out=out0)
                again, _ = hip.lead_rows(A, B, b_kfast, K, n, scale=scale, out=out0)
                cut.add(chunks > 1)
                s = np.ones(rows) if scale is None else scale
                ref = s[:, None] * (a @ b)
                bound = C_TOL * K * 2.0 ** -53 * s[:, None] * (np.abs(a) @ np.abs(b))
                err = np.abs(got[:, :n] - ref)
                what = (K, n, rows)
                assert np.all(np.isfinite(got[:, :n])), what
                assert np.all(err <= bound), (what, float(np.max(err / bound)))
                assert np.all(got[:, n:] == -7.0), what
                assert np.array_equal(got, again), what
    # both forms ran: one workgroup per column block over all of K, and chunks of K summed by the second kernel
    assert cut == {False, True}


def test_lead_rows_refuses_more_rows_than_it_holds(hip):
    with pytest.raises(ValueError):
        hip.lead_rows(np.ones((17, 8)), np.ones((8, 4)), False, 8, 4)
