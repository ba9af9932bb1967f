"""CPU: the restatements behind tests/test_gpu_cholesky_fft_edges.py (oracle/kernel_edges.py) hold what that file relies on -
the Cholesky sizes reach every slicing edge of cholesky_upper, the float64 Stockham model stays within a small multiple of
pocketfft's own distance from a long-double transform, the long-double truth with options is the definition, a root
constant wrong in its 13th digit is far above the bar the device test derives, and the generators give what they promise."""
import numpy as np
import pytest

from oracle import kernel_edges as K
from oracle import ref_numpy as O

OPTION_LENGTHS = (12, 35, 4374, 5000)


def test_cholesky_sizes_reach_every_edge_at_256_compute_units():
    got = K.cholesky_sizes(256)
    print("cholesky sizes at 256 compute units:", got)
    assert got["skipped"] == {}
    assert got["edges"] == {"nsplit_ge_5_not_multiple_of_4": 321, "nsplit_gt_8": 577, "nsplit_gt_16": 1089,
                            "kchunk_odd_multiple_of_16": 1793, "last_slice_32_rows": 1793, "last_slice_16_rows": 1793}
    assert got["fixed"] == [1, 15, 16, 17, 63, 64, 65, 79, 80, 81, 127, 128, 129, 191, 192, 193]
    reached = set()
    for n in got["sizes"]:
        reached |= K.cholesky_edges_reached(n, 256)
    assert reached == set(K.CHOL_EDGES)
    # the odd multiple at 1793 is 80 rows: the k-loop (steps of 32) ends after multiply(o0) alone
    assert any(p[3] == 80 for p in K.cholesky_schedule(1793, 256))
    assert all(p[3] == 64 for n in range(65, 1793) for p in K.cholesky_schedule(n, 256))
    # rest of 1, 15, 16, 17, 63, 64 columns behind the first panel; a short last block of 1 and 63 rows
    assert {n - 64 for n in got["fixed"] if 64 < n <= 128} >= {1, 15, 16, 17, 63, 64}
    assert {n % 64 for n in got["fixed"]} >= {1, 63}


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_cholesky_schedule_covers_the_contraction(cus):
    for n in list(range(1, 400)) + [1793, 2501, 2920]:
        sched = K.cholesky_schedule(n, cus)
        assert [p[0] for p in sched] == list(range(64, n, 64))
        for k0, ntile, nsplit, kchunk, last in sched:
            assert kchunk % 16 == 0 and kchunk >= 64 and ntile == -(-(n - k0) // 64)
            assert (nsplit - 1) * kchunk < k0 <= nsplit * kchunk and 0 < last <= kchunk and last % 16 == 0


def test_cholesky_sizes_name_what_the_cap_leaves_out():
    got = K.cholesky_sizes(256, cap=600)
    assert set(got["skipped"]) == {"nsplit_gt_16", "kchunk_odd_multiple_of_16", "last_slice_32_rows", "last_slice_16_rows"}
    assert all("600" in why for why in got["skipped"].values())
    assert max(got["sizes"]) == 577


def test_fft_plan_is_the_kernels():
    assert K.fft_plan(5120) == [4, 4, 4, 4, 4, 5] and K.fft_plan(4374) == [2] + [3] * 7 and K.fft_plan(5103) == [3] * 6 + [7]
    assert K.fft_plan(8) == [4, 2] and K.fft_plan(5040) == [4, 4, 3, 3, 5, 7]
    assert K.fft_plan(1) is None and K.fft_plan(22) is None and K.fft_plan(5121) is None and K.fft_plan(5184) is None
    assert all(K.fft_plan(n) for n in K.FFT_LENGTHS + OPTION_LENGTHS)


@pytest.mark.parametrize("n", sorted(set(K.FFT_LENGTHS + OPTION_LENGTHS)))
def test_stockham_is_within_a_small_multiple_of_pocketfft(n):
    """Every stage rounds a twiddle product and R - 1 terms per output; w^r by repeated product adds up to R - 2 = 5 roundings
    to a twiddle at radix 7, where pocketfft reads it from a table: ten times pocketfft's own error is room for that and no
    more (measured 0.9 to 2.3)."""
    assert np.finfo(np.clongdouble).eps < 1e-18            # the truth is wider than float64
    for cplx in (True, False):
        for sign in (-1, 1):
            x = K.fft_input(3, n, cplx)
            truth = K.fft_truth(x, sign)
            assert truth.dtype == np.clongdouble
            ref = np.fft.fft(x) if sign < 0 else np.conj(np.fft.fft(np.conj(x)))
            e_model, e_pocket = K.fft_error(K.stockham(x, sign), truth), K.fft_error(ref, truth)
            print("n %d complex %d sign %+d: stockham %.2e pocketfft %.2e ratio %.2f" % (n, cplx, sign, e_model, e_pocket, e_model / e_pocket))
            assert e_pocket < 1e-15 and e_model < 10 * e_pocket
            assert 3 * max(e_model, e_pocket) < K.fft_present_bar(n)


@pytest.mark.parametrize("n", [7, 49, 343, 4375, 4802, 5040, 5103])
def test_a_root_of_radix_7_wrong_in_its_13th_digit_is_above_the_device_bar(n):
    """what the third scratch edit of the device tests (one FftRoots<7>::s constant) costs, on the model"""
    rc, rs = K.FFT_ROOTS[7]
    wrong = dict(K.FFT_ROOTS)
    wrong[7] = (rc, (rs[0], 0.78183148246812980871) + rs[2:])
    x = K.fft_input(3, n, True)
    truth = K.fft_truth(x, -1)
    bar = 3 * max(K.fft_error(K.stockham(x, -1), truth), K.fft_error(np.fft.fft(x), truth))
    err = K.fft_error(K.stockham(x, -1, roots=wrong), truth)
    print("n %d: wrong root %.2e, bar %.2e" % (n, err, bar))
    assert err > 3 * bar


def test_truth_with_options_is_the_definition():
    rng = np.random.default_rng(5)
    n, n_in, n_keep, batch = 12, 7, 5, 3
    x = rng.standard_normal((batch, n_in)) + 1j * rng.standard_normal((batch, n_in))
    sin, sa, sb = rng.standard_normal(n_in), rng.standard_normal(n_keep), rng.standard_normal(batch)
    for sign in (-1, 1):
        for conj_in in (False, True):
            got = K.fft_ex_truth(x, n, sign, n_keep=n_keep, conj_in=conj_in, sin=sin, sa=sa, sb=sb, scale=0.25)
            xs = (np.conj(x) if conj_in else x) * sin
            w = np.exp(sign * 2j * np.pi * np.outer(np.arange(n_keep), np.arange(n_in)) / n)
            ref = 0.25 * sa[None, :] * sb[:, None] * (xs @ w.T)
            assert got.shape == (batch, n_keep) and np.max(np.abs(got - ref)) < 1e-13 * np.max(np.abs(ref))


def test_cholesky_inputs_are_what_they_say():
    for cplx in (False, True):
        A = K.wishart(65, cplx)
        assert np.array_equal(A, A.conj().T) and A.dtype == (np.complex128 if cplx else np.float64)
        assert 10 < np.linalg.cond(A) < 100
        G = K.graded(129, cplx)
        piv = np.abs(K.lapack_upper(G).diagonal()) ** 2
        assert np.array_equal(G, G.conj().T) and 1e5 < piv.max() / piv.min() < 1e8
        S = K.centred_gram(80, cplx)
        assert np.max(np.abs(S @ np.ones(80))) < 1e-10 * np.max(np.abs(S))
        R = K.lapack_upper(A)
        assert np.array_equal(R, np.triu(R)) and K.chol_backward_error(R, A) < 1e-14


@pytest.mark.parametrize("n,mistake", [(321, "drop_tail_slices"), (1089, "drop_tail_slices"), (1793, "skip_second_operand_set")])
def test_two_mistakes_in_the_row_update_are_above_the_device_bar(n, mistake):
    """the first two scratch edits of the device tests, on a numpy restatement of the panel loop with the device's slices
    (256 compute units): as it is the loop meets the bar of the device test, with either mistake it misses it or reports a
    pivot that is not positive"""
    A = K.wishart(n, False)
    bar = min(1e-13, 10 * K.chol_backward_error(K.lapack_upper(A), A))
    R, ok = K.left_looking_cholesky(A, 256)
    assert ok and K.chol_backward_error(R, A) < bar
    R, ok = K.left_looking_cholesky(A, 256, **{mistake: True})
    err = K.chol_backward_error(R, A) if ok else float("inf")
    print("n %d %s: ok %s backward error %.3g, bar %.3g" % (n, mistake, ok, err, bar))
    assert not ok or err > 1e6 * bar


@pytest.mark.parametrize("T,two_fields", K.ANALYTIC_CASES)
def test_analytic_fields_leave_modes_to_compare(T, two_fields):
    """the device test compares the vectors of the separated modes only: there must be some in the oracle alone"""
    fields = K.analytic_fields(T, two_fields)
    assert [f.shape for f in fields] == ([(T, 3 * T), (T, 2 * T)] if two_fields else [(T, 3 * T)])
    assert (K.fft_plan(T) is not None) == (T in (12, 35))
    sigma = O.OracleModel(*fields).solve(complexify=True)["singular_values"]
    m = K.analytic_m(T)
    sep = K.separated_modes(sigma, m)
    print("T %d fields %d: %d of %d modes separated" % (T, len(fields), len(sep), m))
    assert len(sep) >= K.ANALYTIC_MIN_MODES
    assert np.all(sigma[m:] < 1e-12 * sigma[0])
