"""The leading-eigenvector stage of the eigensolver - hermitian_evd(n_lead): guard, trd_eigenvectors_partial, and every way
back to the full stage or the Jacobi sweeps (csrc/jacobi.h, csrc/tridiag_vec.h) - at kernel level through
xmca_eigh_lead, against numpy.linalg.eigh in float64 on the same matrix.  tests/test_gpu_partial_solve.py reaches the stage
through MCA only and compares it with the full solve of the same device, which shares reduction, multisection and twisted
kernel with it.

Matrices and stated routes: tests/partial_eigh_cases.py (checked against the guard model without a device by
tests/test_partial_solve_host.py).  Bars: those tests/test_gpu_tridiag.py holds the full stage to.  The entry point hands the
solver planes of k + 1 rows with padded rows, sentinel-filled: nothing may be written outside the k x n result."""
import numpy as np
import pytest

import partial_eigh_cases as E

pytestmark = pytest.mark.gpu

_FULL = {}


def _route_env(monkeypatch, vec_min_n):
    if vec_min_n is None:
        monkeypatch.delenv("XMCA_TRIDIAG_VEC_MIN_N", raising=False)
    else:
        monkeypatch.setenv("XMCA_TRIDIAG_VEC_MIN_N", vec_min_n)


def _full_call(hip, case):
    """hip.eigh(A) without n_lead, once per matrix: (lam, tridiag)"""
    if case.matrix not in _FULL:
        lam, _ = hip.eigh(E.matrix(case))
        _FULL[case.matrix] = (lam, hip.last_eigh_info["tridiag"])
    return _FULL[case.matrix]


def _check_figures(name, m, bars):
    print("%s: eig %.2e (%.0e) orth %.2e (%.0e) res %.2e (%.0e) proj %s vec %s" % (
        name, m["eig"], bars[0], m["orth"], bars[1], m["res"], bars[2],
        "%.2e (%.2e)" % (m["proj"], m["proj_bound"]) if "proj" in m else "-",
        "%.2e (%.2e)" % (m["vec"], m["vec_bound"]) if "vec" in m else "-"))
    assert m["eig"] < bars[0], m
    assert m["orth"] < bars[1], m
    assert m["res"] < bars[2], m
    if "proj" in m:
        assert m["proj"] <= m["proj_bound"], m
    if "vec" in m:
        assert m["vec"] <= m["vec_bound"], m


@pytest.mark.parametrize("case", E.CASES, ids=repr)
def test_leading_vectors_match_lapack(hip, monkeypatch, case):
    _route_env(monkeypatch, case.vec_min_n)
    A = E.matrix(case)
    lam_ref, U_ref, res_ref = E.reference(case)
    n = A.shape[0]
    lam, U = hip.eigh(A, n_lead=case.k)
    info = dict(hip.last_eigh_info)
    assert lam.shape == (n,) and U.shape == (n, case.k)
    m = E.measure(A, lam_ref, U_ref, res_ref, lam, U, case.hard)
    print(case.name, info)
    _check_figures(case.name, m, E.bars(case))
    assert info["guard_rows_clean"], info
    assert case.k <= info["n_eigvec"] <= n
    if not case.route_free:
        assert info["n_eigvec"] == case.n_eigvec, info
        if case.tridiag is not None:
            assert info["tridiag"] == case.tridiag, info
    if case.name in ("cutpair_k11", "cutpairc_k11", "bitequal_k2"):
        assert "proj" in m                                   # (the cut behind the returned set is clear: the projector was compared)
    lam_full, full_tridiag = _full_call(hip, case)
    if info["tridiag"] == 1 and full_tridiag == 1:
        assert np.array_equal(lam, lam_full)                 # the same reduction and multisection: the same bits


def test_full_call_of_a_low_rank_matrix_takes_the_sweeps_the_partial_one_does_not(hip, monkeypatch):
    """a null space of dimension 580 behind the cut: `repeated` sends the full solve to the Jacobi sweeps, the k leading vectors
    never meet it"""
    case = E.BY_NAME["lowrank_k10"]
    _route_env(monkeypatch, case.vec_min_n)
    assert _full_call(hip, case)[1] == 0
    hip.eigh(E.matrix(case), n_lead=case.k)
    assert hip.last_eigh_info["tridiag"] == 1 and hip.last_eigh_info["n_eigvec"] == case.k


def test_nan_input_with_n_lead_raises_like_gesdd(hip, monkeypatch):
    monkeypatch.setenv("XMCA_TRIDIAG_VEC_MIN_N", "2")
    G = np.array(E.gram(300, False))
    G[17, 40] = G[40, 17] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        hip.eigh(G, n_lead=10)
    monkeypatch.delenv("XMCA_TRIDIAG_VEC_MIN_N")
    with pytest.raises(np.linalg.LinAlgError):
        hip.eigh(G, n_lead=10)                               # the sweeps


def test_n_lead_arguments(hip):
    G = E.gram(130, False)
    for bad in (0, -1, 131, 2.5, True):
        with pytest.raises(ValueError):
            hip.eigh(G, n_lead=bad)
    with pytest.raises(ValueError):
        hip.eigh(G, vectors=False, n_lead=3)


def test_all_vectors_through_the_lead_entry_point(hip, monkeypatch):
    """n_lead == n is the call without the argument (the planes keep their padding and the extra row)"""
    monkeypatch.setenv("XMCA_TRIDIAG_VEC_MIN_N", "2")
    G = E.gram(130, False)
    lam, U = hip.eigh(G)
    assert hip.last_eigh_info["tridiag"] == 1 and hip.last_eigh_info["n_eigvec"] == 130 and hip.last_eigh_info["guard_rows_clean"] is None
    lam2, U2 = hip.eigh(G, n_lead=130)
    assert hip.last_eigh_info["tridiag"] == 1 and hip.last_eigh_info["n_eigvec"] == 130 and hip.last_eigh_info["guard_rows_clean"]
    assert np.array_equal(lam, lam2) and np.array_equal(U, U2)


def test_sequences_on_one_handle_give_the_bits_of_fresh_handles(monkeypatch):
    """Full, partial, partial with more vectors, the pairs at 1e-14 and at 3e-15 (refused by the clean-up or not: either way the
    state of the workspace has to survive it), the first partial call again, then another order in full and in part - on ONE handle: the
    compact-WY factors are built on the second stream from the second call on, the planes grow and are re-used, the tile plan
    is rebuilt for the new order, and `prepared` / `joined` pass from the partial stage to the full one after a refusal.  Every
    result has the bits of the same call made first on a fresh handle, and stands against LAPACK."""
    from xmca_amd import _hip
    monkeypatch.setenv("XMCA_TRIDIAG_VEC_MIN_N", "2")
    G600, G514 = E.gram(600, False), E.gram(514, False)
    P14, P15 = E.matrix(E.BY_NAME["pairs_1e-14"]), E.matrix(E.BY_NAME["pairs_3e-15_n160"])
    steps = [("full600", G600, None), ("part600_k10", G600, 10), ("part600_k65", G600, 65), ("pairs1e-14_k20", P14, 20),
             ("pairs3e-15_n160_k20", P15, 20), ("part600_k10", G600, 10), ("full514", G514, None), ("part514_k10", G514, 10)]
    fresh = {}
    for name, A, k in steps:
        if name not in fresh:
            h = _hip.Handle(0)
            fresh[name] = h.eigh(A, n_lead=k) + (dict(h.last_eigh_info),)
            h.close()
    one = _hip.Handle(0)
    refs = {}
    for name, A, k in steps:
        lam, U = one.eigh(A, n_lead=k)
        info = dict(one.last_eigh_info)
        print(name, info)
        assert info == fresh[name][2], (name, info, fresh[name][2])
        assert np.array_equal(lam, fresh[name][0]) and np.array_equal(U, fresh[name][1]), name
        assert info["guard_rows_clean"] in (True, None)
        if id(A) not in refs:
            w, V = np.linalg.eigh(A)
            refs[id(A)] = (w[::-1], V[:, ::-1], float(np.max(np.linalg.norm(A @ V - V * w, axis=0)) / np.max(np.abs(w))))
        _check_figures(name, E.measure(A, *refs[id(A)], lam, U, True), E.BARS[True])
    one.close()
