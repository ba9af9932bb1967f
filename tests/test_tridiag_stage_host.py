"""CPU: the truth and the float64 restatement behind tests/test_gpu_tridiag_stage.py (tests/tridiag_stage_cases.py),
the two ABI entries, and the refusals of the binding, which reach no device.

  * the longdouble bisection against mpmath.eigsy at 50 digits for every case of order <= 40, and against the closed forms;
  * the longdouble twisted vectors against sin(i k pi / (n + 1)) for Toeplitz (2, -1), and their residual everywhere;
  * the restatement's own error against the truth on every case, printed: below 1 eps bnorm in the values, and in the vectors what
    the twisted factorisation is known for."""
import numpy as np
import pytest

import tridiag_stage_cases as C
from abi_cases import check_entry, check_types, header_abi_version
from xmca_amd import _hip

LD = C.LD
EPS_LD = float(np.finfo(LD).eps)
NEW = {"xmca_tridiag_eigenvalues": 5, "xmca_tridiag_vectors": 8}


class _NoDevice:
    """a handle that fails the test when anything reaches it"""

    def __getattr__(self, name):
        raise AssertionError("device touched: " + name)


# ---- the cases ----------------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_orders_at_which_the_loops_change_shape():
    orders = [c.n for c in C.cases() if c.name.startswith("random_n") and "_" not in c.name[len("random_n"):]]
    assert orders == [1, 2, 3, 8, 9, 15, 16, 17, 24, 25, 33, 63, 64, 65, 66, 127, 128, 129, 130, 257]
    by = {c.name: c for c in C.cases()}
    assert by["toeplitz_n4097"].n == 4097 and not by["toeplitz_n4097"].vectors
    assert all(c.vectors for c in C.cases() if c.n <= 300)
    assert np.count_nonzero(by["random_n120_every_17th_e_zero"].e == 0.0) == 7
    c = by["ramp_n200_e_1e-120"]
    assert (c.es * c.es).max() < C.E2_FLOOR                    # (e^2 lies below the floor of the Sturm kernel)
    for c in C.cases():
        m = max(np.abs(c.ds).max(), np.abs(c.es).max() if c.n > 1 else 0.0)
        assert 0.5 <= m < 1.0 and np.array_equal(c.ds / c.f, c.d) and np.array_equal(c.es / c.f, c.e), c.name   # (the scaling is exact)
    assert C.scale_factor(np.zeros(3), np.zeros(2)) == 1.0


# ---- truth of the eigenvalues -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in C.cases() if c.n <= 40])
def test_the_longdouble_bisection_agrees_with_mpmath_at_50_digits(name):
    """90 halvings end at neighbouring longdoubles; the recurrence's own error is a few longdouble eps of bnorm"""
    import mpmath
    c = C.case(name)
    with mpmath.workdps(50):
        T = mpmath.zeros(c.n)
        for i in range(c.n):
            T[i, i] = mpmath.mpf(float(c.ds[i]))
        for i in range(c.n - 1):
            T[i, i + 1] = T[i + 1, i] = mpmath.mpf(float(c.es[i]))
        ref = sorted(mpmath.eigsy(T, eigvals_only=True))
        got = C.bisect_longdouble(c.ds, c.es)
        # (a longdouble is the exact sum of two doubles)
        err = max(abs(mpmath.mpf(float(g)) + mpmath.mpf(float(g - LD(float(g)))) - r) for g, r in zip(got, ref))
    print("%s: bisection - mpmath = %.2g longdouble eps of bnorm" % (name, float(err) / (EPS_LD * c.bnorm)))
    assert float(err) <= 8 * EPS_LD * c.bnorm


@pytest.mark.parametrize("name,kind", [("toeplitz_n300", "toeplitz"), ("clement_n200", "clement"), ("identity_n100", "diagonal"),
                                       ("diagonal_n7", "diagonal")])
def test_the_longdouble_bisection_agrees_with_the_closed_forms(name, kind):
    """where a midpoint makes a pivot exactly zero (Toeplitz, Clement) the pivmin guard is what keeps the count.  Clement: the
    integers belong to the matrix with exact square roots; e rounded to double moves an eigenvalue by at most 2 max |delta e|
    <= eps max |e| <= eps bnorm / 2 (eps of float64)"""
    c = C.case(name)
    err = float(np.max(np.abs(C.bisect_longdouble(c.ds, c.es) - C.closed_form(kind, c))))
    print("%s: bisection - closed form = %.3g float64 eps of bnorm" % (name, err / (C.EPS * c.bnorm)))
    assert err <= (0.5 * C.EPS if kind == "clement" else 8 * EPS_LD) * c.bnorm


def test_the_closed_form_of_the_large_toeplitz_case_is_a_sturm_sequence_away_from_the_bisection():
    """n = 4097 has no bisection in the tests; here a sample of its closed-form eigenvalues is bracketed by two counts each"""
    c = C.case("toeplitz_n4097")
    t = C.truth_values(c.name)
    d, e2 = c.ds.astype(LD), (c.es * c.es).astype(LD)
    k = np.array([0, 1, 17, 1000, 2048, 3333, 4095, 4096])
    w = LD(64 * EPS_LD * c.bnorm)
    for shift, want in ((-w, k), (w, k + 1)):
        x = t[k] + shift
        q = d[0] - x
        cnt = (q < 0).astype(np.int64)
        for i in range(1, c.n):
            q = (d[i] - x) - e2[i - 1] / q
            cnt += q < 0
        assert np.array_equal(cnt, want), (shift, cnt, want)


# ---- truth of the vectors -----------------------------------------------------------------------------------------------
def test_the_longdouble_twisted_vectors_are_the_sines_for_toeplitz():
    """sin(angle) * gap / bnorm stays at a few longdouble eps"""
    c = C.case("toeplitz_n300")
    Z, S = C.truth_vectors(c.name), C.toeplitz_vectors(c.n)
    s = np.where(np.sum(Z * S, axis=0) < 0, LD(-1), LD(1))
    fig = np.sqrt(np.sum((Z * s - S) ** 2, axis=0)) * C.gaps(c.name) / LD(c.bnorm)
    print("toeplitz_n300: truth vectors - sines, times gap: %.3g longdouble eps" % (float(fig.max()) / EPS_LD))
    assert float(fig.max()) <= 64 * EPS_LD


@pytest.mark.parametrize("name", C.names(vectors=True))
def test_the_truth_vectors_have_a_longdouble_residual(name):
    """|| T z - lam z || at the longdouble eigenvalue, unit length: what makes them a truth for float64 (2^-11 float64 eps per
    longdouble eps)"""
    c = C.case(name)
    Z, lam = C.truth_vectors(name), C.truth_values(name)
    d, e = c.ds.astype(LD), c.es.astype(LD)
    R = d[:, None] * Z - Z * lam[None, :]
    if c.n > 1:
        R[:-1] += e[:, None] * Z[1:]
        R[1:] += e[:, None] * Z[:-1]
    res = float(np.max(np.sqrt(np.sum(R * R, axis=0)))) / (EPS_LD * c.bnorm)
    nrm = float(np.max(np.abs(np.sqrt(np.sum(Z * Z, axis=0)) - 1))) / EPS_LD
    print("%s: truth vectors: residual %.3g, |norm - 1| %.3g longdouble eps" % (name, res, nrm))
    assert res <= 64 and nrm <= c.n / 2 + 3


# ---- the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.names())
def test_the_restated_multisection_stays_below_one_eps_of_bnorm(name):
    """17^14 = 1.7e17 shrinks the widened Gershgorin interval below eps bnorm / 2; the count is backward stable"""
    r = C.restated_value_error(name)
    print("%s: restated values: %.3f eps bnorm" % (name, r))
    assert r <= 1.0


@pytest.mark.parametrize("name", C.names(vectors=True))
def test_the_restated_twisted_vectors_have_the_residual_of_the_method(name):
    """residual of a few eps bnorm given a correctly rounded eigenvalue, sin(angle) * gap well below one, unit length to the
    (n / 2 + 3) eps the GPU test asks of the device"""
    c = C.case(name)
    fig = C.vector_figures(name, C.restated_vectors(name))
    r_res, r_ang = C.worst(fig)
    print("%s: restated vectors: residual %.3f, sin(angle) * gap %.3f eps bnorm, |norm - 1| %.2f eps" % (name, r_res, r_ang, fig["nrm"].max()))
    assert r_res <= 4.0 and r_ang <= 1.0 and fig["nrm"].max() <= c.n / 2 + 3
    assert (r_res, r_ang) == C.restated_vector_figures(name)


def test_the_restatement_gives_the_closed_forms_where_a_pivot_is_exactly_zero():
    for name, (lam, V) in C.exact_pivot_cases().items():
        c = C.case(name)
        assert np.array_equal(lam, C.lam_for_vectors(name)), name
        Y = C.restate_vectors(c.ds, c.es, lam * c.f)
        assert np.max(np.abs(Y - V)) <= 4 * C.EPS, name


def test_the_restated_twist_index_jumps_across_the_permuted_ramp():
    """neighbouring eigenvalues k, k + 1 of the permuted ramp sit at the rows holding k, k + 1: anywhere in the matrix"""
    c = C.case("permuted_ramp_n256_e_0.01")
    r = np.argmax(np.abs(C.restated_vectors(c.name)), axis=0)
    assert np.array_equal(c.d[r], np.arange(1.0, 257.0))
    assert r[:64].max() - r[:64].min() > 192 and np.abs(np.diff(r)).max() > 192


# ---- ABI and binding ----------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_bound():
    for name, n_args in NEW.items():
        check_entry(name, n_args)
        check_types(name, *_hip.SIGNATURES[name])
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version() == 16
    for method in ("tridiag_eigenvalues", "tridiag_vectors"):
        assert callable(getattr(_hip.Handle, method))


def test_the_library_refuses_bad_arguments_before_it_looks_at_the_handle():
    """n < 1, a NULL pointer, nev outside [1, n], ldy < nev: XMCA_ERR_INVALID with no handle at all, so no device was asked"""
    lib = _hip.load_library()
    d, e, lam, Y = np.ones(4), np.ones(3), np.ones(4), np.ones((4, 4))
    p = _hip._ptr
    assert lib.xmca_tridiag_eigenvalues(None, p(d), p(e), 0, p(lam)) == _hip.ERR_INVALID
    assert lib.xmca_tridiag_eigenvalues(None, None, p(e), 4, p(lam)) == _hip.ERR_INVALID
    assert lib.xmca_tridiag_eigenvalues(None, p(d), None, 4, p(lam)) == _hip.ERR_INVALID
    assert lib.xmca_tridiag_eigenvalues(None, p(d), p(e), 4, None) == _hip.ERR_INVALID
    for n, nev, ldy in ((0, 1, 1), (4, 0, 4), (4, 5, 5), (4, 3, 2)):
        assert lib.xmca_tridiag_vectors(None, p(d), p(e), n, p(lam), nev, p(Y), ldy) == _hip.ERR_INVALID
    assert lib.xmca_tridiag_vectors(None, p(d), p(e), 4, None, 4, p(Y), 4) == _hip.ERR_INVALID
    assert lib.xmca_tridiag_vectors(None, p(d), p(e), 4, p(lam), 4, None, 4) == _hip.ERR_INVALID


@pytest.mark.parametrize("d,e", [(np.ones(4), np.ones(4)), (np.ones(4), np.ones(2)), (np.ones(0), np.ones(0)), (np.ones((2, 2)), np.ones(3)),
                                 (np.ones(4), None)])
def test_the_binding_refuses_bad_shapes_without_touching_a_device(d, e):
    stub = _NoDevice()
    with pytest.raises(ValueError):
        _hip.Handle.tridiag_eigenvalues(stub, d, e)
    with pytest.raises(ValueError):
        _hip.Handle.tridiag_vectors(stub, d, e, np.ones(1))


@pytest.mark.parametrize("lam,out", [(np.ones(0), None), (np.ones(5), None), (np.ones((2, 2)), None), (np.ones(3), np.ones((4, 2))),
                                     (np.ones(3), np.ones((3, 3))), (np.ones(3), np.ones(12))])
def test_the_vector_binding_refuses_bad_lam_and_planes_without_touching_a_device(lam, out):
    with pytest.raises(ValueError):
        _hip.Handle.tridiag_vectors(_NoDevice(), np.ones(4), np.ones(3), lam, out=out)


# ---- the record -------------------------------------------------------------------------------------------------------------
def test_the_accuracy_record_holds_every_case_within_its_allowance():
    """profiles/tridiag_stage_accuracy.json (MI355X): every case is there, the restatement's figures are the ones formed here, and
    the device figures lie within the margin of the GPU test"""
    import json
    import os
    from abi_cases import REPO
    rec = json.load(open(os.path.join(REPO, "profiles", "tridiag_stage_accuracy.json")))
    assert rec["margin"] == 4.0 and sorted(rec["cases"]) == sorted(C.names())
    for name, row in rec["cases"].items():
        c = C.case(name)
        assert row["n"] == c.n
        assert row["values_restated"] == pytest.approx(C.restated_value_error(name), rel=1e-6, abs=1e-9), name
        assert row["values_device"] <= 4.0 * max(row["values_restated"], 1.0), name
        if c.vectors:
            r_res, r_ang = C.restated_vector_figures(name)
            assert row["residual_restated"] == pytest.approx(r_res, rel=1e-6, abs=1e-9), name
            assert row["angle_restated"] == pytest.approx(r_ang, rel=1e-6, abs=1e-9), name
            assert row["residual_device"] <= 4.0 * max(r_res, 1.0) and row["angle_device"] <= 4.0 * max(r_ang, 1.0), name
            assert row["norm_device_eps"] <= c.n / 2 + 3, name
