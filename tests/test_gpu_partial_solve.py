"""`MCA.solve(n_modes=k)`: the model `solve()` + `truncate(k)` leaves, with the vectors of k modes formed, back-projected and kept
on the device only (csrc/jacobi.h hermitian_evd n_lead, csrc/tridiag_vec.h trd_eigenvectors_partial).

The reference of every comparison is the existing path on the same device in the same test: `solve()` (+ `truncate(k)`).
  * state: every `_analysis` entry and the value getters, to the bit (the same reduction and multisection produce them; two
    fields are solved as without the request).  One exception, at the bars of tests/test_gpu_solve.py: inputs of numerical rank
    far below T (k = 64, 65), whose FULL solve falls back to the Jacobi sweeps;
  * vectors: phase-aligned eofs(k) / pcs(k) against the full solve's and the orthonormality defect of the k vectors, both
    allowed 4 x what the full solve itself measures against oracle/ref_numpy.py (float64 SVD) on the same input, and never
    less than the tolerance of tests/test_gpu_configs.py for the dtype (1e-5 / 1e-3 on vectors, 1e-9 / 1e-4 on V^H V - I; 1e-6
    for two fields).  The margin: a k' x k' clean-up sees less of the space than an n x n one, and each of two products rounds
    once more.  profiles/partial_solve_accuracy.json (scripts/partial_solve_accuracy.py) records the measured values;
  * route: `solve_info()[0]['n_eigvec']`, the resident planes' size (`result_info()`).
Inputs: tests/partial_solve_cases.py."""
import os
import sys

import numpy as np
import pytest

try:
    import torch                                            # (before the first device call of the session, as the other torch tests do)
except Exception:                                           # the tensor test then fails where it needs it
    torch = None

from partial_solve_cases import (JACOBI_CASE, ONE_FIELD_CASES, TWO_FIELD_CASE, TWO_FIELD_CPLX_CASE, case_fields as _fields, flat,
                                 mode_error, model_state as _state, oracle as _oracle, orth_defect, planted_fields,
                                 run_case as _run)
from xmca_amd.array import MCA

pytestmark = pytest.mark.gpu

ONE_FIELD_PARAMS = [(c[0], k) for c in ONE_FIELD_CASES for k in c[5]]
VEC_FLOOR = {np.dtype(np.float64): 1e-5, np.dtype(np.float32): 1e-3}
ORTH_FLOOR = {np.dtype(np.float64): 1e-9, np.dtype(np.float32): 1e-4}


def _assert_planes(kib, need_bytes, planes):
    """`result_info()['vector_kib']` is what the handle has ALLOCATED for the planes of one side: at least the planes, and no
    more than the pool's rule for handing out a kept block allows (csrc/common.h DevPool::take: 5/4 of the request + 1 MiB), per
    plane, plus the 256-byte granule."""
    assert kib * 1024 >= need_bytes, (kib, need_bytes)
    assert kib <= (need_bytes * 5 // 4) / 1024 + planes * (1024 + 1), (kib, need_bytes)


def _assert_state(a, b, exact, n=0):
    """exact: to the bit.  Otherwise the bars of tests/test_gpu_solve.py for float64: 1e-5 relative on every value above 1e-6 of
    the largest, 1e-8 on the totals - and, on the singular values, 8 n eps of the largest absolutely: two backward-stable
    eigensolvers of an order-n problem each leave n eps ||G||."""
    assert a["analysis"].keys() == b["analysis"].keys()
    for key, va in a["analysis"].items():
        vb = b["analysis"][key]
        if exact or not isinstance(va, (float, np.floating)):
            assert va == vb, (key, va, vb)
        else:
            assert abs(va - vb) <= 1e-8 * abs(vb), (key, va, vb)
    for key in a:
        if key == "analysis":
            continue
        x, y = np.asarray(a[key], dtype=np.float64), np.asarray(b[key], dtype=np.float64)
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, key
        if exact:
            assert np.array_equal(a[key], b[key]), (key, np.max(np.abs(x - y)))
        else:
            keep = np.abs(y) > 1e-6 * np.max(np.abs(y))
            assert np.max(np.abs(x[keep] - y[keep]) / np.abs(y[keep])) < 1e-5, key
            if key == "singular_values":
                assert np.max(np.abs(x - y)) <= 8 * n * 2.220446049250313e-16 * np.max(np.abs(y)), key


def _assert_vectors(r, k, orth_floor):
    for key in r["keys"]:
        for what in ("eofs", "pcs"):
            full_err = mode_error(np.asarray(r["full_" + what][key]), r["oracle_" + what][key])
            err = mode_error(np.asarray(r["part_" + what][key]), np.asarray(r["full_" + what][key]))
            tol = max(4.0 * full_err, VEC_FLOOR[r["dtype"]])
            print("%s %s k=%d: full vs oracle %.3e, partial vs full %.3e (tol %.3e)" % (what, key, k, full_err, err, tol))
            assert err <= tol, (what, key, err, tol)
        full_def, part_def = orth_defect(r["full_eofs"][key]), orth_defect(r["part_eofs"][key])
        tol = max(4.0 * full_def, orth_floor)
        print("orthonormality %s k=%d: full %.3e, partial %.3e (tol %.3e)" % (key, k, full_def, part_def, tol))
        assert part_def <= tol, (key, part_def, tol)


@pytest.mark.parametrize("name,k", ONE_FIELD_PARAMS)
def test_state_is_that_of_solve_then_truncate(hip, name, k):
    r = _run(hip, name, k)
    # The values of both models come from the same reduction and multisection: the same bits.  The exception:
    # a field of numerical rank far below T (k = 64, 65: noise at 1e-20 of the leading sigma^2) sends the FULL solve to the
    # Jacobi sweeps - its null space is a cluster no twisted vector resolves - while the k leading vectors never meet it.
    same_solver = r["full_info"][0]["tridiag"] == 1
    print("%s k=%d: full solve by %s" % (name, k, "the tridiagonal route" if same_solver else "Jacobi sweeps"))
    assert same_solver or k >= 64
    _assert_state(r["part_state"], r["full_state"], exact=same_solver, n=r["T"])
    a = r["part_state"]["analysis"]
    assert a["is_truncated"] is True and a["is_truncated_at"] == k and a["rank"] == r["T"]
    assert r["part_state"]["singular_values"].shape == (k,)


@pytest.mark.parametrize("name,k", ONE_FIELD_PARAMS)
def test_vectors_match_the_full_solve(hip, name, k):
    r = _run(hip, name, k)
    _assert_vectors(r, k, ORTH_FLOOR[r["dtype"]])


@pytest.mark.parametrize("name,k", ONE_FIELD_PARAMS)
def test_partial_route_forms_k_vectors_and_keeps_k_modes(hip, name, k):
    r = _run(hip, name, k)
    n = r["T"] // 2 + 1 if r["cplx"] else r["T"]             # order of the eigenproblem (analytic-signal subspace: T / 2 + 1)
    assert r["full_info"][0]["n_eigvec"] == n
    assert r["part_info"][0]["tridiag"] == 1 and r["part_info"][0]["n_eigvec"] == k
    # the vectors were neither fetched nor dropped on the host: k modes, all still on the device after eofs / pcs
    assert r["part_lazy"] == k and r["still_resident"]
    # device memory of the result scales with k - on a handle that held all T modes just before (run_case)
    planes = 2 if r["cplx"] else 1
    item = (4 if r["dtype"] == np.float32 else 8) * planes
    N, T = r["Ns"][0], r["T"]
    assert r["part_result"]["n_vec"] == k and r["full_result"]["n_vec"] == T
    assert r["part_result"]["vector_kib"][1] == 0
    assert r["full_result"]["vector_kib"][0] * 1024 >= T * N * item      # (the plain solve keeps whatever larger block it had)
    _assert_planes(r["part_result"]["vector_kib"][0], k * N * item, planes)
    assert r["part_result"]["vector_kib"][0] * 3 < r["full_result"]["vector_kib"][0]


@pytest.mark.parametrize("case", [TWO_FIELD_CASE, TWO_FIELD_CPLX_CASE], ids=lambda c: c[0])
def test_two_fields_keep_their_route_and_back_project_k_modes(hip, case):
    name, k = case[0], case[5][0]
    r = _run(hip, name, k)
    # solved as without the request, the planes behind mode k given back (csrc/solver.h Solver::solve, solve_analytic): the same
    # bits - in time space and in the analytic-signal frame of two wide complexified fields
    _assert_state(r["part_state"], r["full_state"], exact=True)
    _assert_vectors(r, k, 1e-6)
    assert r["part_info"] == r["full_info"]                                   # the small problems are solved as before
    assert r["part_result"]["n_vec"] == k and r["part_lazy"] == k
    planes = 2 if r["cplx"] else 1
    for side, N in enumerate(r["Ns"]):
        _assert_planes(r["part_result"]["vector_kib"][side], k * N * 8 * planes, planes)
        assert r["full_result"]["vector_kib"][side] * 1024 >= r["full_result"]["n_vec"] * N * 8 * planes


def test_below_the_threshold_all_vectors_are_formed_and_k_back_projected(hip):
    name, k = JACOBI_CASE[0], JACOBI_CASE[5][0]
    r = _run(hip, name, k)
    _assert_state(r["part_state"], r["full_state"], exact=True)
    _assert_vectors(r, k, ORTH_FLOOR[r["dtype"]])
    assert r["part_info"][0]["tridiag"] == 0 and r["part_info"][0]["n_eigvec"] == r["T"]
    assert r["part_result"]["n_vec"] == k and r["part_lazy"] == k


@pytest.mark.parametrize("k", [300, 1000])
def test_k_at_or_above_the_rank_is_the_plain_solve(hip, k):
    name = JACOBI_CASE[0]
    fields = _fields(name, 10)
    a, b = MCA(*fields, handle=hip), MCA(*fields, handle=hip)
    a.solve()
    sa = _state(a)
    b.solve(n_modes=k)
    assert hip.result_info()["n_vec"] == 300 and b._V._rank == 300
    _assert_state(_state(b), sa, exact=True)
    assert b._analysis["is_truncated"] is False and b._analysis["is_truncated_at"] == 300


def test_guard_keeps_a_close_pair_together(hip):
    """amplitudes k and k + 1 differ by 1e-9 relative: the eigenvalue behind the cut is no neighbour to leave out"""
    name, k = "t800", 10
    fields = _fields(name, k, tie=(k - 1, 1e-9))
    full = MCA(*fields, handle=hip)
    full.solve()
    Vf = flat(full.eofs(k + 1)["left"])
    part = MCA(*fields, handle=hip)
    part.solve(n_modes=k)
    info = hip.solve_info()[0]
    assert info["tridiag"] == 1 and k < info["n_eigvec"] < 800, info
    assert hip.result_info()["n_vec"] == k and flat(part.eofs(k)["left"]).shape == (1000, k)
    part.solve(n_modes=k + 1)
    assert hip.solve_info()[0]["n_eigvec"] == k + 1
    Vp = flat(part.eofs(k + 1)["left"])
    # the pair is one invariant subspace: the projectors onto the leading k + 1 modes agree, the two vectors need not
    Vo = _oracle(fields, False, k + 1)[0][0]
    proj = lambda V: V @ V.conj().T                                           # noqa: E731
    full_err = float(np.max(np.abs(proj(Vf) - proj(Vo))))
    err = float(np.max(np.abs(proj(Vp) - proj(Vf))))
    print("projector k+1: full vs oracle %.3e, partial vs full %.3e" % (full_err, err))
    assert err <= max(4.0 * full_err, 1e-5)
    assert orth_defect(Vp) <= max(4.0 * orth_defect(Vf), 1e-9)


def _workflow(m, k, other=None):
    """the calls of a session on k modes; returns their results as numpy arrays"""
    out = {}
    n_rot = min(k, 10)
    for power in (1, 4):
        m.rotate(n_rot, power)
        tag = "p%d_" % power
        out[tag + "n_iter"] = m._varimax_iterations
        out[tag + "R"] = np.asarray(m.rotation_matrix())
        out[tag + "eofs"] = m.eofs(n_rot)["left"]
        out[tag + "pcs"] = m.pcs(n_rot)["left"]
        out[tag + "predict"] = m.predict(other)["left"]
        out[tag + "rec"] = m.reconstructed_fields(n_rot)["left"]
        hom = m.homogeneous_patterns(n_rot)
        out[tag + "hom_r"], out[tag + "hom_p"] = hom[0]["left"], hom[1]["left"]
    return out


def _as_numpy(v):
    if hasattr(v, "detach"):                                                  # tensor
        v = v.detach().cpu().numpy()
    elif hasattr(v, "coords"):                                                # DataArray
        v = v.values
    return np.asarray(v)


def _assert_workflow(a, b, tol):
    assert a.keys() == b.keys()
    for key in a:
        if key.endswith("n_iter"):
            assert a[key] == b[key], (key, a[key], b[key])                    # equal Varimax iteration counts
            continue
        x, y = _as_numpy(a[key]), _as_numpy(b[key])
        assert x.shape == y.shape and x.dtype == y.dtype, (key, x.shape, y.shape, x.dtype, y.dtype)
        ok = np.isfinite(y)
        assert np.array_equal(ok, np.isfinite(x)), key
        scale = np.max(np.abs(y[ok]))
        if key.endswith("hom_p"):
            continue                                                          # (p-values of r ~ 1 are 1e-300: pinned through r)
        assert np.max(np.abs(x[ok] - y[ok])) <= tol * scale, (key, float(np.max(np.abs(x[ok] - y[ok])) / scale))


def _rotate_outcome(m, n_rot):
    try:
        m.rotate(n_rot)
    except Exception as err:      # noqa: BLE001 - whatever the existing path raises is the contract
        return type(err)
    return None


def test_workflow_after_partial_solve_matches_truncate(hip):
    name, k = "t800", 10
    fields = _fields(name, k)
    new = planted_fields(40, (1000,), k, 77)[0]
    full = MCA(*fields, handle=hip)
    full.solve()
    full.truncate(k)
    ref = _workflow(full, k, new)
    part = MCA(*fields, handle=hip)
    part.solve(n_modes=k)
    got = _workflow(part, k, new)
    _assert_workflow(got, ref, 1e-5)
    # rotate(k + 1) asks for a mode that is not there: whatever truncate(k) makes of it, solve(n_modes=k) makes too
    a, b = MCA(*fields, handle=hip), MCA(*fields, handle=hip)
    a.solve()
    a.truncate(k)
    want = _rotate_outcome(a, k + 1)
    b.solve(n_modes=k)
    assert _rotate_outcome(b, k + 1) is want
    if want is None:
        assert a._varimax_iterations == b._varimax_iterations
        assert np.max(np.abs(np.asarray(a.rotation_matrix()) - np.asarray(b.rotation_matrix()))) <= 1e-5


def test_workflow_with_tensor_input_and_torch_output(hip):
    assert torch is not None, "torch is part of the GPU test environment"
    name, k = "t800", 10
    x = torch.from_numpy(_fields(name, k)[0]).to("cuda:0")
    new = torch.from_numpy(planted_fields(40, (1000,), k, 77)[0]).to("cuda:0")
    full = MCA(x, handle=hip, output="torch")
    full.solve()
    full.truncate(k)
    ref = _workflow(full, k, new)
    part = MCA(x, handle=hip, output="torch")
    part.solve(n_modes=k)
    assert part._vectors_resident() and part._V._rank == k
    got = _workflow(part, k, new)
    assert all(hasattr(v, "detach") == hasattr(ref[key], "detach") for key, v in got.items())
    _assert_workflow(got, ref, 1e-5)


def test_workflow_through_the_xarray_facade(hip):
    try:
        import xarray as xr
    except Exception:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
        import xarray as xr
    from xmca_amd.xarray import xMCA
    name, k = "t800", 10
    T, nlat, nlon = 800, 25, 40
    lat, lon = np.linspace(-60.0, 60.0, nlat), np.linspace(0.0, 195.0, nlon)

    def da(v):
        return xr.DataArray(v.reshape(v.shape[0], nlat, nlon), dims=["time", "lat", "lon"],
                            coords={"time": np.arange(v.shape[0]), "lat": lat, "lon": lon})
    field, new = da(_fields(name, k)[0]), da(planted_fields(40, (1000,), k, 77)[0])
    full = xMCA(field)
    full.solve()
    full.truncate(k)
    ref = _workflow(full, k, new)
    part = xMCA(field)
    part.solve(n_modes=k)
    got = _workflow(part, k, new)
    _assert_workflow(got, ref, 1e-5)
    # coordinates of results with k modes
    assert list(part.singular_values().coords["mode"].values) == list(range(1, k + 1))
    assert list(part.singular_values().coords["mode"].values) == list(full.singular_values().coords["mode"].values)
    e = part.eofs()["left"]
    assert e.shape == (nlat, nlon, k) and list(e.coords["mode"].values) == list(range(1, k + 1))
    assert part.pcs()["left"].shape == (T, k)


def test_two_partial_solves_give_the_same_bits(hip):
    name, k = "t800", 10
    fields = _fields(name, k)
    out = []
    for _ in range(2):
        m = MCA(*fields, handle=hip)
        m.solve(n_modes=k)
        out.append((m.singular_values(), flat(m.eofs(k)["left"]), m.pcs(k)["left"]))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_more_than_a_quarter_of_the_modes_forms_all_vectors_from_the_same_reduction(hip):
    """k > n / 4 is no thin set: all vectors are formed by the full stage - from the reduction and the eigenvalues already at
    hand - and k rows handed out.  The values are the full solve's bits; the vectors differ by the back-projection's rounding."""
    name, k = "t800", 300
    fields = _fields(name, 10)
    full = MCA(*fields, handle=hip)
    full.solve()
    Vf = flat(full.eofs(16)["left"])
    full.truncate(k)
    ref = _state(full)
    part = MCA(*fields, handle=hip)
    part.solve(n_modes=k)
    info = hip.solve_info()[0]
    assert info["tridiag"] == 1 and info["n_eigvec"] == 800, info
    assert hip.result_info()["n_vec"] == k and part._V._rank == k
    _assert_state(_state(part), ref, exact=True)
    assert mode_error(flat(part.eofs(16)["left"]), Vf) <= 1e-9          # the 16 planted modes (the rest is noise: tiny gaps)
