"""The blocked Cholesky (csrc/cholesky.h, csrc/chol64.h) and the batched FFT (csrc/fft.h) at their panel, slice, stride and
option edges, through the C ABI (`Handle.cholesky`, `Handle.cholesky_ex`, `Handle.fft`, `Handle.fft_ex`), and the analytic
frame above both through the class.  References and sizes come from oracle/kernel_edges.py (tests/test_kernel_edges_oracle.py
checks them without a device); every bar is either one an older test of this project holds or is computed here from the
reference's own error:

* Cholesky: backward error max |R^H R - A| / max diag(A) under 10 x that of numpy.linalg.cholesky on the same matrices (largest
  over the sizes of the real / the complex group; 10: another summation order - MFMA chains of 4, up to 17 slices), never above
  1e-13; forward error against LAPACK's factor under 1e-11.  Sizes: cholesky_sizes(compute units of the device).
* FFT: error over max |truth| (scipy.fft in long double) under 3 x the larger of the float64 Stockham model's and pocketfft's
  own error on the same input (3: FMA contraction, a sincospi an ulp away), never above the bar of test_fft_matches_numpy.
* Analytic frame: singular values at 1e-10, vectors of the separated modes at 1e-8 of max |v| against the numpy oracle.

XMCA_CHOL_FFT_EDGES_RECORD=<file>: the largest device figure, the reference figure and the bar of every group are written there
(scripts/cholesky_fft_edges_accuracy.py -> profiles/cholesky_fft_edges_accuracy.json).

Measured on an MI355X (256 compute units; profiles/cholesky_fft_edges_accuracy.json):
  Cholesky backward error  real 1.13e-15 (n = 1089; LAPACK 5.4e-16, bar 5.4e-15), complex 1.94e-15 (n = 1089; 4.8e-16, 4.8e-15);
           graded 6.3e-16 / 7.2e-16; shifted 1.05e-15 / 1.46e-15; forward error 6.1e-16 / 1.04e-15
  FFT      plain transforms at most 7.0e-16, never above 0.65 of the bar of their length (closest: n = 2); options and call
           shapes at most 6.3e-16 (rows of the first pass) under bars of 1.0e-15 .. 1.8e-15
  analytic frame  sigma 6.2e-15, vectors 4.6e-11 (FFT route) and 5.3e-11 (explicit Fourier vectors)
The kernels passed all of it.  The first generator of the analytic fields spread sigma over a factor 1500 and two-field vectors
then differed by 1.3e-8 (T = 35) and 7.2e-8 (T = 33): the squared formulation of the two-field solve (HISTORY.md, accuracy of
small modes), not the frame - oracle/kernel_edges.py analytic_fields says what the generator keeps to since.

Three arithmetic mistakes, and what notices them.  They were not run on the device; their cost is shown on the CPU
restatements in tests/test_kernel_edges_oracle.py:
  1. the slab sum of chol64_rowupdate_kernel stopping at the last full group of four slices: left_looking_cholesky with the
     device's slices gives a backward error of 0.33 at n = 321 and 0.11 at n = 1089 against bars of 4e-15 -
     test_cholesky_backward_and_forward_error_at_every_size from n = 321 on, and every contract test that compares bits at a split size;
  2. the second operand set of its k-loop skipped when kchunk / 16 is odd: 0.13 at n = 1793, the one size with kchunk = 80 -
     the same test at that size, real and complex;
  3. FftRoots<7>::s[1] wrong in its 13th digit: the Stockham model gives 4e-14 .. 9e-14 at n = 7, 49, 343, 4375, 4802, 5040, 5103
     against bars of 4e-16 .. 2e-15 - test_fft_at_radix_and_loop_edges at those lengths.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import align_modes
from oracle import kernel_edges as K

pytestmark = pytest.mark.gpu

FIGURES = {}
CHOL_CEILING = 1e-13        # test_cholesky_matches_numpy, backward
CHOL_FORWARD = 1e-11        # test_cholesky_matches_numpy, against LAPACK's factor
SIGMA_BAR = 1e-10           # test_small_and_ragged_shapes_match_oracle
VECTOR_BAR = 1e-8           # test_analytic_subspace_path_equals_general_path


@pytest.fixture(scope="module", autouse=True)
def _record_figures():
    yield
    dst = os.environ.get("XMCA_CHOL_FFT_EDGES_RECORD")
    if dst:
        with open(dst, "w") as f:
            json.dump(FIGURES, f, indent=1, sort_keys=True)


def _note(group, device, reference, bar):
    row = FIGURES.setdefault(group, {"device": 0.0, "reference": 0.0, "bar": float(bar)})
    row["device"] = max(row["device"], float(device)) if np.isfinite(device) else float("nan")
    row["reference"] = max(row["reference"], float(reference))
    row["bar"] = float(bar)


@pytest.fixture(scope="module")
def hip():
    from xmca_amd import _hip
    h = _hip.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def plan():
    """The sizes for the compute units torch reports.  torch is asked in a process of its own: it carries its own HIP runtime,
    and in a process where the library's runtime already holds the device that second runtime finds none."""
    ask = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"
    cus = int(subprocess.run([sys.executable, "-c", ask], check=True, capture_output=True, text=True).stdout.split()[-1])
    got = K.cholesky_sizes(cus)
    got["cus"] = cus
    print("compute units %d: %s" % (cus, got))
    return got


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _name(cplx):
    return "complex" if cplx else "real"


# ------------------------------------------------------------------------------------------------
# 3.1 Cholesky, accuracy
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chol(hip, plan):
    """every size, real and complex, Wishart and graded, on the device and through LAPACK, once:
    (kind, cplx, n) -> dict(A, R, ok, e_dev, e_ref, fwd); bars[cplx] = min(1e-13, 10 max e_ref)"""
    out = {}
    for cplx in (False, True):
        for n in plan["sizes"]:
            for kind, make in (("wishart", K.wishart), ("graded", K.graded)):
                A = make(n, cplx)
                R, ok = hip.cholesky(A)
                ref = K.lapack_upper(A)
                out[kind, cplx, n] = dict(A=A, R=R, ok=ok, e_dev=K.chol_backward_error(R, A), e_ref=K.chol_backward_error(ref, A),
                                          fwd=float(np.max(np.abs(R - ref)) / np.max(np.abs(ref))))
    bars = {cplx: min(CHOL_CEILING, 10 * max(v["e_ref"] for (kind, c, n), v in out.items() if c == cplx)) for cplx in (False, True)}
    return out, bars


@pytest.mark.parametrize("cplx", [False, True])
def test_cholesky_backward_and_forward_error_at_every_size(chol, plan, cplx):
    cases, bars = chol
    assert not plan["skipped"] or all("no n <=" in why for why in plan["skipped"].values())
    for n in plan["sizes"]:
        c = cases["wishart", cplx, n]
        R = c["R"]
        print("n %d %s: device %.3g lapack %.3g bar %.3g forward %.3g" % (n, _name(cplx), c["e_dev"], c["e_ref"], bars[cplx], c["fwd"]))
        _note("cholesky_backward/" + _name(cplx), c["e_dev"], c["e_ref"], bars[cplx])
        _note("cholesky_forward/" + _name(cplx), c["fwd"], 0.0, CHOL_FORWARD)
        assert c["ok"], n
        assert R.dtype == c["A"].dtype and np.all(R[np.tril_indices(n, -1)] == 0), n
        d = R.diagonal()
        assert np.all(d.real > 0) and np.all(d.imag == 0), n
        assert c["e_dev"] < bars[cplx], (n, c["e_dev"], bars[cplx])
        assert c["fwd"] < CHOL_FORWARD, (n, c["fwd"])


@pytest.mark.parametrize("cplx", [False, True])
def test_cholesky_of_a_graded_matrix_backward_error(chol, plan, cplx):
    """pivots spread over 1e6 (what factor_by_cholesky accepts goes to 1e8): backward error only"""
    cases, bars = chol
    for n in plan["sizes"]:
        c = cases["graded", cplx, n]
        print("n %d %s graded: device %.3g lapack %.3g bar %.3g" % (n, _name(cplx), c["e_dev"], c["e_ref"], bars[cplx]))
        _note("cholesky_graded_backward/" + _name(cplx), c["e_dev"], c["e_ref"], bars[cplx])
        assert c["ok"] and np.all(c["R"][np.tril_indices(n, -1)] == 0), n
        assert c["e_dev"] < bars[cplx], (n, c["e_dev"], bars[cplx])


# ------------------------------------------------------------------------------------------------
# 3.2 Cholesky, contracts
# ------------------------------------------------------------------------------------------------
def _split_size(plan):
    return plan["edges"].get("nsplit_ge_5_not_multiple_of_4", 321)


def _chunk_size(plan):
    return plan["edges"].get("kchunk_odd_multiple_of_16", 1793)


@pytest.mark.parametrize("cplx", [False, True])
def test_cholesky_never_reads_the_lower_triangle(hip, chol, plan, cplx):
    cases, _ = chol
    for n in (65, 193, _chunk_size(plan)):
        c = cases["wishart", cplx, n]
        A = c["A"].copy()
        A[np.tril_indices(n, -1)] = complex(np.nan, np.nan) if cplx else np.nan
        R, ok = hip.cholesky(A)
        assert ok and np.array_equal(_bits(R), _bits(c["R"])), n


@pytest.mark.parametrize("cplx", [False, True])
def test_cholesky_of_an_offset_block_with_a_leading_dimension(hip, chol, plan, cplx):
    """the call of factor_by_cholesky: the block behind row / column `first`, ld = lda; everything around it is NaN before
    and has the same bits after, the block has the bits of the plain call"""
    cases, _ = chol
    nan = complex(np.nan, np.nan) if cplx else np.nan
    for nb in (65, 129, _split_size(plan)):
        c = cases["wishart", cplx, nb]
        for first, pad in ((1, 3), (0, 1)):
            n = nb + first
            buf = np.full((n, n + pad), nan, dtype=c["A"].dtype)
            buf[first:, first:n] = c["A"]
            out, ok = hip.cholesky_ex(buf, first=first)
            assert ok and out.shape == buf.shape, (nb, first)
            assert np.array_equal(_bits(out[first:, first:n]), _bits(c["R"])), (nb, first)
            inside = np.zeros(buf.shape, dtype=bool)
            inside[first:, first:n] = True
            assert np.array_equal(_bits(out)[np.repeat(~inside, 2, axis=1) if cplx else ~inside],
                                  _bits(buf)[np.repeat(~inside, 2, axis=1) if cplx else ~inside]), (nb, first)
    with pytest.raises(ValueError):
        hip.cholesky_ex(cases["wishart", cplx, 65]["A"], first=65)           # refused on the host


@pytest.mark.parametrize("cplx", [False, True])
def test_cholesky_slabs_and_tickets_serve_the_next_call(hip, chol, plan, cplx):
    """A, then B with more slices and tiles, then A again on one handle: the slabs of B lie where those of A are read from,
    and every ticket must have been left at zero"""
    cases, _ = chol
    a, b = _split_size(plan), plan["edges"].get("nsplit_gt_8", 577)
    assert max(p[2] for p in K.cholesky_schedule(b, plan["cus"])) > max(p[2] for p in K.cholesky_schedule(a, plan["cus"]))
    A, B = cases["wishart", cplx, a]["A"], cases["wishart", cplx, b]["A"]
    R1, ok1 = hip.cholesky(A)
    R2, ok2 = hip.cholesky(B)
    R3, ok3 = hip.cholesky(A)
    assert ok1 and ok2 and ok3
    assert np.array_equal(_bits(R1), _bits(R3)) and np.array_equal(_bits(R1), _bits(cases["wishart", cplx, a]["R"]))
    assert np.array_equal(_bits(R2), _bits(cases["wishart", cplx, b]["R"]))


@pytest.mark.parametrize("cplx", [False, True])
def test_cholesky_reports_a_pivot_that_is_not_positive(hip, chol, cplx):
    """n = 193: three panels and a last block of one row.  A negative diagonal entry in the first 16-block, in a later 16-block
    of the first panel, in the second panel and in the short last block; after each the handle factors a good matrix as before"""
    cases, _ = chol
    good = cases["wishart", cplx, 193]
    for at in (3, 40, 100, 192):
        A = good["A"].copy()
        A[at, at] = -A[at, at]
        R, ok = hip.cholesky(A)
        assert ok is False, at
        R, ok = hip.cholesky(good["A"])
        assert ok and np.array_equal(_bits(R), _bits(good["R"])), at


@pytest.mark.parametrize("cplx", [False, True])
def test_cholesky_reports_values_that_are_no_numbers(hip, chol, cplx):
    cases, _ = chol
    good = cases["wishart", cplx, 193]
    for at in ((5, 100), (70, 192), (10, 192)):               # a row panel; the last column from the second and the first panel
        A = good["A"].copy()
        A[at] = np.nan
        assert hip.cholesky(A)[1] is False, at
    A = good["A"]
    bad = good["A"].copy()
    bad[7, 7] = np.inf
    for M in (np.zeros_like(A), -A, bad):
        assert hip.cholesky(M)[1] is False
    R, ok = hip.cholesky(A)
    assert ok and np.array_equal(_bits(R), _bits(good["R"]))


@pytest.mark.parametrize("cplx", [False, True])
def test_cholesky_shift_makes_a_singular_gram_matrix_definite(hip, chol, plan, cplx):
    cases, bars = chol
    n = plan["edges"].get("nsplit_gt_8", 577)
    A = K.centred_gram(n, cplx)
    shift = 1e-13
    R, ok = hip.cholesky(A, rel_shift=shift)
    As = A + shift * np.max(A.diagonal().real) * np.eye(n)
    err = K.chol_backward_error(R, As)
    print("n %d %s shifted: device %.3g bar %.3g" % (n, _name(cplx), err, bars[cplx]))
    _note("cholesky_shifted_backward/" + _name(cplx), err, 0.0, bars[cplx])
    assert ok and np.all(R[np.tril_indices(n, -1)] == 0) and np.all(R.diagonal().real > 0)
    assert err < bars[cplx]


# ------------------------------------------------------------------------------------------------
# 3.3 FFT, accuracy at radix and loop edges
# ------------------------------------------------------------------------------------------------
def _numpy_fft(x, sign):
    return np.fft.fft(x) if sign < 0 else np.conj(np.fft.fft(np.conj(x)))


def _fft_bar(model, pocket, truth, n):
    e_model, e_pocket = K.fft_error(model, truth), K.fft_error(pocket, truth)
    return min(3 * max(e_model, e_pocket), K.fft_present_bar(n)), e_model, e_pocket


@pytest.mark.parametrize("n", K.FFT_LENGTHS)
def test_fft_at_radix_and_loop_edges(hip, n):
    for cplx in (True, False):
        for sign in (-1, 1):
            x = K.fft_input(3, n, cplx)
            truth = K.fft_truth(x, sign)
            bar, e_model, e_pocket = _fft_bar(K.stockham(x, sign), _numpy_fft(x, sign), truth, n)
            err = K.fft_error(hip.fft(x, sign=sign), truth)
            print("n %d complex %d sign %+d: device %.3g model %.3g pocketfft %.3g bar %.3g" % (n, cplx, sign, err, e_model, e_pocket, bar))
            _note("fft_plain/%d" % n, err, max(e_model, e_pocket), bar)
            assert err <= bar, (n, cplx, sign, err, bar)


# ------------------------------------------------------------------------------------------------
# 3.4 FFT, options
# ------------------------------------------------------------------------------------------------
def _fft_ex_case(hip, group, x, n, sign, in_bs, in_es, in_count, out_bs, out_es, out_count, n_keep=None, conj_in=False, sin=None,
                 sa=None, sb=None, scale=1.0, in_im_null=False):
    """x (batch, n_in): the elements that are read, placed at b * in_bs + t * in_es of NaN-filled planes of in_count elements;
    the outputs are NaN-filled planes of out_count elements.  Checks the n_keep outputs of every transform against the
    long-double definition and that every other output element is still NaN.  Returns the error."""
    batch, n_in = x.shape
    n_keep = n if n_keep is None else n_keep
    idx_in = (np.arange(batch)[:, None] * in_bs + np.arange(n_in)[None, :] * in_es).ravel()
    idx_out = (np.arange(batch)[:, None] * out_bs + np.arange(n_keep)[None, :] * out_es).ravel()
    assert len(set(idx_in)) == idx_in.size and len(set(idx_out)) == idx_out.size
    in_re, in_im = np.full(in_count, np.nan), (None if in_im_null else np.full(in_count, np.nan))
    in_re[idx_in] = x.real.ravel()
    if in_im_null:
        assert not np.iscomplexobj(x)
    else:
        in_im[idx_in] = x.imag.ravel() if np.iscomplexobj(x) else 0.0
    nan = np.full(out_count, np.nan)
    out_re, out_im = hip.fft_ex(in_re, in_im, batch, n, nan, nan, sign=sign, in_bs=in_bs, in_es=in_es, n_in=n_in, conj_in=conj_in,
                                sin=sin, out_bs=out_bs, out_es=out_es, n_keep=n_keep, sa=sa, sb=sb, scale=scale)
    rest = np.ones(out_count, dtype=bool)
    rest[idx_out] = False
    assert np.all(np.isnan(out_re[rest])) and np.all(np.isnan(out_im[rest])), group       # nothing written beside the outputs
    got = (out_re[idx_out] + 1j * out_im[idx_out]).reshape(batch, n_keep)
    truth = K.fft_ex_truth(x, n, sign, n_keep=n_keep, conj_in=conj_in, sin=sin, sa=sa, sb=sb, scale=scale)
    # the float64 model and pocketfft on the same input, with the factors applied the way the kernel applies them
    xs = np.conj(x) if conj_in else x
    xs = xs if sin is None else xs * np.asarray(sin)[None, :]
    full = np.zeros((batch, n), dtype=np.complex128)
    full[:, :n_in] = xs
    f = (scale * (np.ones(batch) if sb is None else np.asarray(sb)))[:, None] * (np.ones(n_keep) if sa is None else np.asarray(sa))[None, :]
    bar, e_model, e_pocket = _fft_bar(K.stockham(full, sign)[:, :n_keep] * f, _numpy_fft(full, sign)[:, :n_keep] * f, truth, n)
    err = K.fft_error(got, truth)
    print("%s n %d: device %.3g model %.3g pocketfft %.3g bar %.3g" % (group, n, err, e_model, e_pocket, bar))
    _note("fft_options/" + group, err, max(e_model, e_pocket), bar)
    assert err <= bar, (group, n, err, bar)        # (n_in = 1 is exact in every arithmetic: 0 <= 0)
    return err


def _hilbert_weights(T, m):
    h = np.full(m, 2.0)
    h[0] = 1.0
    if T % 2 == 0:
        h[-1] = 1.0
    return h


@pytest.mark.parametrize("T", [12, 35, 4374, 5000])
def test_fft_in_the_three_call_shapes_of_the_solver(hip, T):
    """analytic_gram: rows of a real T x T matrix, m outputs kept, rows m apart; then its columns, both strides m, scaled by
    h_k h_l / T.  analytic_project: m of T inputs, conjugated and weighted, 1 / sqrt(T)."""
    m = K.analytic_m(T)
    batch = {5000: 3, 4374: 32}.get(T)         # (the long-double truth and the float64 model of T rows of 4374 points take half a minute)
    h = _hilbert_weights(T, m)
    rng = np.random.default_rng(T)
    # first pass (solver.h: fft_batch(T rows of G, +1, n_keep = m, out_bs = m))
    b1 = batch or T
    _fft_ex_case(hip, "solver_rows", rng.standard_normal((b1, T)), T, +1, T, 1, b1 * T, m, 1, b1 * m, n_keep=m, in_im_null=True)
    # second pass (columns of the T x m result: in_bs = 1, in_es = m; output at the same strides; sa = sb = h; 1 / T)
    b2 = batch or m
    x = rng.standard_normal((b2, T)) + 1j * rng.standard_normal((b2, T))
    _fft_ex_case(hip, "solver_columns", x, T, -1, 1, m, T * m, 1, m, m * m, n_keep=m, sa=h, sb=h[:b2], scale=1.0 / T)
    # projection (nv rows of m coefficients, zero-padded to T, conj_in, sin = h, 1 / sqrt(T))
    x = rng.standard_normal((3, m)) + 1j * rng.standard_normal((3, m))
    _fft_ex_case(hip, "solver_projection", x, T, +1, m, 1, 3 * m, T, 1, 3 * T, conj_in=True, sin=h, scale=1.0 / np.sqrt(T))


@pytest.mark.parametrize("n,n_in", [(35, 1), (35, 35), (5120, 1), (5120, 4096), (5120, 4097), (5120, 5120)])
def test_fft_reads_n_in_elements_and_no_more(hip, n, n_in):
    """rows n apart: the n - n_in elements behind the ones that count are NaN (the load loop takes 4096 elements a trip)"""
    x = K.fft_input(3, n, True, seed=1)[:, :n_in]
    _fft_ex_case(hip, "n_in", x, n, -1, n, 1, 3 * n, n, 1, 3 * n)


@pytest.mark.parametrize("n,n_keep", [(35, 1), (35, 35), (5120, 1), (5120, 2048), (5120, 2049), (5120, 4097), (5120, 5120)])
def test_fft_writes_n_keep_elements_and_no_more(hip, n, n_keep):
    """outputs two elements apart in rows of 2 n + 3: what lies between them and behind n_keep stays NaN (the store loop takes
    2048 elements a trip)"""
    x = K.fft_input(3, n, True, seed=2)
    _fft_ex_case(hip, "n_keep", x, n, +1, n, 1, 3 * n, 2 * n + 3, 2, 3 * (2 * n + 3), n_keep=n_keep)


def test_fft_flags_and_factors(hip):
    n, batch, n_in, n_keep = 540, 3, 300, 271
    rng = np.random.default_rng(540)
    xc, xr = K.fft_input(batch, n, True, seed=3)[:, :n_in], K.fft_input(batch, n, False, seed=3)[:, :n_in]
    sin, sa, sb = rng.uniform(0.5, 2.0, n_in), rng.uniform(0.5, 2.0, n_keep), np.array([0.5, -1.25, 3.0])
    lay = dict(in_bs=n_in + 2, in_es=1, in_count=batch * (n_in + 2), out_bs=n_keep + 1, out_es=1, out_count=batch * (n_keep + 1),
               n_keep=n_keep)
    _fft_ex_case(hip, "conj_in_real_input", xr, n, -1, conj_in=True, in_im_null=True, **lay)
    _fft_ex_case(hip, "conj_in", xc, n, -1, conj_in=True, **lay)
    _fft_ex_case(hip, "sin", xc, n, -1, sin=sin, **lay)
    _fft_ex_case(hip, "sin_conj_in", xc, n, +1, sin=sin, conj_in=True, **lay)
    _fft_ex_case(hip, "sa", xc, n, -1, sa=sa, **lay)
    _fft_ex_case(hip, "sb", xc, n, -1, sb=sb, **lay)
    _fft_ex_case(hip, "scale", xc, n, +1, scale=1.0 / 7.0, **lay)
    _fft_ex_case(hip, "all", xc, n, +1, sin=sin, conj_in=True, sa=sa, sb=sb, scale=1.0 / 7.0, **lay)


def test_fft_ex_refuses_a_request_outside_its_buffers(hip):
    """the argument test of xmca_fft_ex alone: every request here is turned away on the host, nothing is launched"""
    n, batch = 12, 3
    x = np.zeros(batch * n)
    out = np.full(batch * n, np.nan)
    ok = dict(in_bs=n, in_es=1, out_bs=n, out_es=1)
    for bad in (dict(in_bs=n + 1), dict(in_es=2), dict(out_bs=n + 1), dict(out_es=2), dict(in_bs=-1), dict(out_es=-1), dict(n_in=0),
                dict(n_in=n + 1), dict(n_keep=0), dict(n_keep=n + 1)):
        with pytest.raises(ValueError):
            hip.fft_ex(x, x, batch, n, out, out, **dict(ok, **bad))
    with pytest.raises(ValueError):
        hip.fft_ex(x, x, batch + 1, n, out, out, **ok)
    with pytest.raises(NotImplementedError):
        hip.fft_ex(np.zeros(33), None, 3, 11, np.zeros(33), np.zeros(33))
    re, im = hip.fft_ex(x + 1.0, None, batch, n, out, out, **ok)              # and the handle is as good as before
    assert np.array_equal(re.reshape(batch, n)[:, 0], np.full(batch, float(n))) and np.all(np.abs(re.reshape(batch, n)[:, 1:]) < 1e-14)
    assert np.all(np.abs(im) < 1e-14)


# ------------------------------------------------------------------------------------------------
# 3.5 analytic frame end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,two_fields", K.ANALYTIC_CASES)
def test_analytic_frame_against_the_oracle(T, two_fields):
    """T = 12, 35: the FFT route; T = 22, 33: the explicit Fourier vectors (a prime factor above 7); even T adds the Nyquist row"""
    from oracle import ref_numpy as O
    from xmca_amd.array import MCA
    fields = K.analytic_fields(T, two_fields)
    ref = O.OracleModel(*fields).solve(complexify=True)
    model = MCA(*fields)
    model.solve(complexify=True)
    s, s_ref = model._singular_values, ref["singular_values"]
    m = K.analytic_m(T)
    assert len(s) == len(s_ref)
    keep = s_ref > 1e-8 * s_ref[0]
    e_sigma = float(np.max(np.abs(s[keep] - s_ref[keep]) / s_ref[keep]))
    assert np.all(s[m:] == 0.0)
    sep = K.separated_modes(s_ref, m)
    assert len(sep) >= K.ANALYTIC_MIN_MODES
    V = np.concatenate([model._V[k][:, sep] for k in model._keys], axis=0)
    V_ref = np.concatenate([v[:, sep] for v in ref["V"]], axis=0)
    mine, _ = align_modes(V, V_ref)                      # one phase per mode for both fields together
    e_vec = float(np.max(np.abs(mine - V_ref)) / np.max(np.abs(V_ref)))
    print("T %d fields %d: sigma %.3g vectors of %d modes %.3g" % (T, len(fields), e_sigma, len(sep), e_vec))
    _note("analytic_sigma/%s" % ("fft" if K.fft_plan(T) else "gemm"), e_sigma, 0.0, SIGMA_BAR)
    _note("analytic_vectors/%s" % ("fft" if K.fft_plan(T) else "gemm"), e_vec, 0.0, VECTOR_BAR)
    assert e_sigma < SIGMA_BAR, e_sigma
    assert e_vec < VECTOR_BAR, e_vec
