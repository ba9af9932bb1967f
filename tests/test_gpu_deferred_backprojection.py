"""xmca_solve on one field leaves the back-projection of the modes >= H in flight on a second stream (csrc/solver.h
DeferredTail) and every reader joins.  The deferred form must give every element of every vector the bits of
the single launch (XMCA_DEFER_BACKPROJECT=0), in whatever order the entry points are called.

The switch is read once per process, so each form runs in a child process of its own; H is forced to one row tile
(XMCA_DEFER_HEAD=128) so that models small enough for a test defer.  The child reports through XMCA_TRACE=solve whether a
solve deferred: a comparison in which nothing was deferred would pass for nothing."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from xmca_amd import _hip

dst, T, N, dtype, cplx = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), np.dtype(sys.argv[5]), sys.argv[6] == "1"
n_rot = 10


def field(seed):
    # a signal weak enough that every mode but the null one of the centering is scaled in the GEMM's epilogue (solver.h: lambda_k
    # above 1e-4 lambda_0 for float32 fields): the conditions for deferring hold for both dtypes
    rng = np.random.default_rng(seed)
    k = 12
    X = (rng.standard_normal((T, k)) * np.linspace(1.5, 0.5, k)) @ rng.standard_normal((k, N)) + rng.standard_normal((T, N))
    return (X - X.mean(axis=0)).astype(dtype)


def solve(h):
    if cplx:
        h.complexify(T)
    return h.solve(1)


A, B, C = field(1), field(2), field(3)
h = _hip.Handle(0)
out = {}

# two solves back to back without any reader (the first solve of a handle is serial: the second stream is made on the second), then all modes
h.set_field(0, A)
solve(h)
rank = solve(h)
out["sigma_A"] = h.singular_values(rank)
out["V_A"] = h.vectors(0, rank, N, dtype)

# model B of the same shape on the same handle, the readers of a rotation, then at once all modes: complete rows of B (a row the
# tail had not written yet would be a row of A)
h.set_field(0, B)
rank = solve(h)
sig = h.singular_values(rank)
Vt = h.vectors(0, n_rot, N, dtype)
L = Vt.T * np.sqrt(sig[:n_rot])
rot = h.rotate_loadings(L, n_left=N, power=1, tol=1e-8)
out["V_B"] = h.vectors(0, rank, N, dtype)
out["V_B_head"] = Vt
out["R_B"] = rot["R"]
out["n_iter_B"] = np.array([rot["n_iter"]])
out["eofs_B"] = h.eofs(0, N, rank, None, dtype)          # another reader of every mode, through its own entry point

# new data directly behind a solve, then the OLD result: complete and correct, or the state error - never rows from the new field.
# xmca_set_field invalidates the result, so the read returns the state error and shows no more than that nothing breaks; what would
# catch a set_field that did not join (a tail reading the new field) is V_C below: same shape, solved at once, compared bit for bit
solve(h)
h.set_field(0, C)
try:
    out["V_B_after_set_field"] = h.vectors(0, rank, N, dtype)
    out["after_set_field_error"] = np.array([0])
except _hip.HipError as e:
    out["after_set_field_error"] = np.array([e.code])
rank = solve(h)
out["V_C"] = h.vectors(0, rank, N, dtype)
h.close()
np.savez(dst, **out)
"""


def run_child(tmp, name, T, N, dtype, cplx, defer, extra_env=None):
    dst = os.path.join(tmp, name + ".npz")
    env = dict(os.environ, XMCA_DEFER_BACKPROJECT="1" if defer else "0", XMCA_DEFER_HEAD="128", XMCA_TRACE="solve")
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, dst, str(T), str(N), dtype, "1" if cplx else "0"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(dst)), r.stderr.count("deferred to the second stream")


# (the complexified model takes the analytic-signal route by default, which has a back-projection of its own and does not defer;
#  with XMCA_ANALYTIC=0 the imaginary plane is formed and the complex one-field route - four real products per launch - defers)
CASES = [
    ("f64", 600, 3000, "float64", False, None, True),
    ("f32", 600, 3000, "float32", False, None, True),
    ("cplx", 400, 2000, "float64", True, {"XMCA_ANALYTIC": "0"}, True),
    ("cplx_analytic", 400, 2000, "float64", True, None, False),
]


@pytest.mark.parametrize("name,T,N,dtype,cplx,extra_env,defers", CASES, ids=[c[0] for c in CASES])
def test_deferred_tail_gives_the_bits_of_the_single_launch(name, T, N, dtype, cplx, extra_env, defers):
    with tempfile.TemporaryDirectory() as tmp:
        on, n_on = run_child(tmp, "on", T, N, dtype, cplx, True, extra_env)
        off, n_off = run_child(tmp, "off", T, N, dtype, cplx, False, extra_env)
    assert n_off == 0
    # five solves per child; the first one of a handle stays serial
    assert n_on == (4 if defers else 0), n_on
    assert sorted(on) == sorted(off)
    for key in sorted(on):
        assert on[key].dtype == off[key].dtype and on[key].shape == off[key].shape, key
        assert np.array_equal(on[key], off[key]), key               # bit for bit (no NaN anywhere: array_equal would fail)
    # all T modes, the null mode of the centering (normalised by what it is, behind the product) included
    assert on["V_A"].shape == (T, N) and on["V_B"].shape == (T, N)
    # (a row the tail never wrote would be zero or stale: every row of the one-field route is a unit vector, far from norm 0.5;
    #  the analytic-signal route leaves its null modes zero, with the switch on or off)
    if defers:
        norms = np.linalg.norm(on["V_B"].astype(np.complex128 if cplx else np.float64), axis=1)
        assert np.all(np.abs(norms - 1.0) < 0.5), (norms.min(), norms.max())
    assert np.array_equal(on["V_B"][:10], on["V_B_head"])
    # model B is not model A, and what came back behind set_field is the documented state error or the old model
    assert not np.array_equal(on["V_A"][200], on["V_B"][200])
    code = int(on["after_set_field_error"][0])
    if code == 0:
        assert np.array_equal(on["V_B_after_set_field"], on["V_B"])
    else:
        from xmca_amd import _hip
        assert code == _hip.ERR_STATE
