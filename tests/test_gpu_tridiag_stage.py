"""GPU: the two kernels that carry the tridiagonal eigensolver behind the Householder reduction, each alone on a chosen (d, e)
(DESIGN.md 3): `trd_bisect_kernel` through `Handle.tridiag_eigenvalues`, `trd_twisted_kernel` through `Handle.tridiag_vectors`.
Cases, truth (longdouble) and the float64 restatement of both kernels: tests/tridiag_stage_cases.py.

Every error is in units of eps * bnorm, bnorm = max_i(|d_i| + |e_{i-1}| + |e_i|) of the scaled matrix.  The device is held to
4 * max(r, 1), r the restatement's own error on the case: the device fuses the multiply-add of its recurrences and rescales by exact
powers of two, with the same number of roundings per row as the restatement - the factor covers fma against separate rounding and
nothing else.  Every vector bound is asserted on every column of every case.  The worst device figure per case, beside the
restatement's, is kept in profiles/tridiag_stage_accuracy.json (written again to the file named by XMCA_TRIDIAG_STAGE_ACCURACY)."""
import json
import os

import numpy as np
import pytest

import tridiag_stage_cases as C

pytestmark = pytest.mark.gpu

MARGIN = 4.0
RECORD = {}


def _note(name, **figures):
    RECORD.setdefault(name, {"n": C.case(name).n}).update({k: v if isinstance(v, int) else float(v) for k, v in figures.items()})


@pytest.fixture(scope="module")
def device_values(hip):
    """name -> what the device returns for the case (descending, the caller's scale), computed once"""
    return {c.name: hip.tridiag_eigenvalues(c.d, c.e) for c in C.cases()}


@pytest.fixture(scope="module")
def device_vectors(hip):
    """name -> the n x n plane of the nev = n call with lam = the truth rounded to double, computed once"""
    return {name: hip.tridiag_vectors(C.case(name).d, C.case(name).e, C.lam_for_vectors(name)) for name in C.names(vectors=True)}


# ---- values -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.names())
def test_eigenvalues_stay_within_four_times_the_restatement(name, device_values):
    c = C.case(name)
    lam = device_values[name]
    assert lam.shape == (c.n,) and lam.dtype == np.float64 and np.all(np.isfinite(lam))
    err = C.value_errors(name, C.device_values_scaled(name, lam))
    r = C.restated_value_error(name)
    print("%s: device %.3f, restatement %.3f eps bnorm" % (name, err.max(), r))
    _note(name, values_device=err.max(), values_restated=r)
    assert np.all(err <= MARGIN * max(r, 1.0)), (name, float(err.max()), r, int(np.argmax(err)))
    assert np.all(np.diff(lam) <= 0.0), name                                     # non-increasing


@pytest.mark.parametrize("name", ["random_n17", "random_n130", "wilkinson21_x10_glue1e-07", "random_n120_every_17th_e_zero",
                                  "random_n100_scale1e-150", "toeplitz_n4097"])
def test_eigenvalues_repeat_their_bits_and_do_not_see_the_sign_of_e(name, hip, device_values):
    c = C.case(name)
    assert np.array_equal(hip.tridiag_eigenvalues(c.d, c.e), device_values[name]), name
    assert np.array_equal(hip.tridiag_eigenvalues(c.d, -c.e), device_values[name]), name
    flip = np.where(np.arange(c.n - 1) % 3 == 0, -1.0, 1.0)
    assert np.array_equal(hip.tridiag_eigenvalues(c.d, flip * c.e), device_values[name]), name


def test_the_value_entry_scales_as_a_solve_does(hip):
    """f is an exact power of two: the bits of the mantissas do not depend on it.  A zero matrix has f = 1; the kernel counts on
    e^2 floored at 2^-200, a matrix whose eigenvalues lie within 2 * 2^-100 of zero, inside an interval widened by 1e-300"""
    c = C.case("random_n65")
    lam = hip.tridiag_eigenvalues(c.d, c.e)
    for p in (2.0 ** 40, 2.0 ** -300, 2.0 ** 500):
        assert np.array_equal(hip.tridiag_eigenvalues(p * c.d, p * c.e), p * lam), p
    zero = hip.tridiag_eigenvalues(np.zeros(9), np.zeros(8))
    assert np.all(np.abs(zero) <= 2.0 ** -99) and np.all(np.diff(zero) <= 0.0), zero
    assert np.array_equal(hip.tridiag_eigenvalues([-3.0], None), [-3.0])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("where", ["d", "e"])
def test_a_non_finite_entry_is_the_numeric_error_of_a_solve(hip, bad, where):
    c = C.case("random_n33")
    d, e = c.d.copy(), c.e.copy()
    (d if where == "d" else e)[11] = bad
    with pytest.raises(np.linalg.LinAlgError):
        hip.tridiag_eigenvalues(d, e)
    with pytest.raises(np.linalg.LinAlgError):
        hip.tridiag_vectors(d, e, C.lam_for_vectors(c.name))
    assert np.array_equal(hip.tridiag_eigenvalues(c.d, c.e), hip.tridiag_eigenvalues(c.d, c.e))     # (the handle is as before)


# ---- vectors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.names(vectors=True))
def test_vectors_stay_within_four_times_the_restatement_in_every_column(name, device_vectors):
    c = C.case(name)
    Y = device_vectors[name]
    assert Y.shape == (c.n, c.n) and np.all(np.isfinite(Y))
    fig = C.vector_figures(name, Y)
    res, ang = C.worst(fig)
    r_res, r_ang = C.restated_vector_figures(name)
    print("%s: residual: device %.3f, restatement %.3f; sin(angle) * gap: device %.3f, restatement %.3f eps bnorm; |norm - 1| %.2f eps"
          % (name, res, r_res, ang, r_ang, fig["nrm"].max()))
    _note(name, residual_device=res, residual_restated=r_res, angle_device=ang, angle_restated=r_ang, norm_device_eps=fig["nrm"].max(),
          columns_with_a_gap=int(np.count_nonzero(~np.isnan(fig["ang"]))))
    assert np.all(fig["res"] <= MARGIN * max(r_res, 1.0)), (name, res, r_res, int(np.argmax(fig["res"])))
    held = ~np.isnan(fig["ang"])
    assert np.all(fig["ang"][held] <= MARGIN * max(r_ang, 1.0)), (name, ang, r_ang)
    assert np.all(fig["nrm"] <= c.n / 2 + 3), (name, float(fig["nrm"].max()))


def test_an_exactly_zero_pivot_gives_the_closed_forms(hip):
    """[[0, 1], [1, 0]] at lam = -1, 1 and a diagonal matrix at its own entries: the floor stands in for the pivot"""
    for name, (lam, V) in C.exact_pivot_cases().items():
        c = C.case(name)
        Y = hip.tridiag_vectors(c.d, c.e, lam)
        _note(name, exact_pivot_device_eps=np.max(np.abs(Y - V)) / C.EPS)
        assert np.max(np.abs(Y - V)) <= 4 * C.EPS, (name, Y)


@pytest.mark.parametrize("nev", [1, 63, 64, 65, 130])
def test_the_partial_call_writes_its_columns_only_and_repeats_the_full_call(nev, hip, device_vectors):
    """n = 130, the nev largest eigenvalues in planes of ldy = nev + 5: columns past nev come back as sent, the others have the bits
    of the matching columns of the nev = n call"""
    name = "random_n130"
    c = C.case(name)
    lam = C.lam_for_vectors(name)
    rng = np.random.default_rng(nev)
    plane = rng.standard_normal((c.n, nev + 5))
    out = hip.tridiag_vectors(c.d, c.e, lam[c.n - nev:], out=plane)
    assert out.shape == plane.shape
    assert np.array_equal(out[:, nev:], plane[:, nev:])
    assert np.array_equal(out[:, :nev], device_vectors[name][:, c.n - nev:])
    tight = hip.tridiag_vectors(c.d, c.e, lam[c.n - nev:])
    assert np.array_equal(tight, out[:, :nev])


@pytest.mark.parametrize("name", ["random_n66", "permuted_ramp_n256_e_0.01", "wilkinson21_x6_glue0.001", "toeplitz_n300"])
def test_vectors_repeat_their_bits(name, hip, device_vectors):
    c = C.case(name)
    assert np.array_equal(hip.tridiag_vectors(c.d, c.e, C.lam_for_vectors(name)), device_vectors[name])


def test_zz_write_accuracy_record():
    """(last in the file) the worst device figure of every case beside the restatement's, for profiles/tridiag_stage_accuracy.json"""
    path = os.environ.get("XMCA_TRIDIAG_STAGE_ACCURACY")
    if path and RECORD:
        with open(path, "w") as f:
            json.dump({"unit": "eps * bnorm (norm_device_eps, exact_pivot_device_eps: eps)", "margin": MARGIN, "cases": RECORD}, f, indent=1,
                      sort_keys=True)
