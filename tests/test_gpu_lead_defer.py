"""The lead route of the one-field solve (csrc/solver.h back_project_lead): from the second xmca_solve of a handle
on, a real float64 model whose vectors come from the tridiagonal route gets its first 16 modes from the skinny kernel, and the
second stream runs the eigensolver's last n x n product and the whole back-projection.  The deferred form must give the bits of
the in-line one (XMCA_DEFER_BACKPROJECT=0), before and after the join, through every reader that does not join.

The switch is read once per process: each form runs in a child of its own (the pattern of test_gpu_deferred_backprojection.py).
The child marks its phases on stderr, and XMCA_TRACE=solve says which route every solve took."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N, N_ROT, LOW_RANK = 800, 1000, 10, 60       # T above XMCA_TRIDIAG_VEC_MIN_N = 768

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from xmca_amd import _hip
from xmca_amd.array import MCA

dst, T, N, n_rot, low_rank = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])


def phase(name):
    sys.stderr.write("@phase %s\n" % name)
    sys.stderr.flush()


def field(seed, dtype, rows=T):
    rng = np.random.default_rng(seed)
    k = 12
    X = (rng.standard_normal((rows, k)) * np.linspace(1.5, 0.5, k)) @ rng.standard_normal((k, N)) + rng.standard_normal((rows, N))
    return (X - X.mean(axis=0)).astype(dtype)


out = {}
h = _hip.Handle(0)

phase("main")                       # solved twice: the first solve of a handle is serial
A = field(1, np.float64)
h.set_field(0, A)
h.solve(1)
rank = h.solve(1)
sig = h.singular_values(rank)
lead = h.vectors(0, n_rot, N, np.float64)                   # no join: the leading modes
rot = h.rotate_loadings(lead.T * np.sqrt(sig[:n_rot]), n_left=N, power=1, tol=1e-8)
res = h.rotate_solved(n_rot, power=1, tol=1e-8)             # no join either
out["sigma"] = sig
out["lead_before"] = lead
out["V"] = h.vectors(0, rank, N, np.float64)                # joins
out["lead_after"] = h.vectors(0, n_rot, N, np.float64)
out["loadings_R"], out["loadings_iter"] = rot["R"], np.array([rot["n_iter"]])
out["solved_R"], out["solved_Phi"], out["solved_norm"], out["solved_iter"] = res["R"], res["Phi"], res["norm_left"], np.array([res["n_iter"]])

phase("class")                      # MCA.rotate on an unread float64 model: xmca_rotate_solved
m = MCA(A, handle=h)
m.solve()
m.rotate(n_rot, power=1)
out["class_R"], out["class_variance"] = m.rotation_matrix(), np.asarray(m._variance)
out["class_V"] = np.asarray(m._get_V(n_rot, rotated=False)["left"])

phase("lowrank")                    # repeated rows: a wide null space, bit-equal eigenvalues -> the Jacobi sweeps
rng = np.random.default_rng(5)
base = rng.standard_normal((low_rank, N)) * np.linspace(3.0, 1.0, low_rank)[:, None]
L = base[rng.integers(0, low_rank, T)]
L = L - L.mean(axis=0)
h.set_field(0, L)
rank = h.solve(1)
out["low_field"], out["low_sigma"] = L, h.singular_values(rank)
out["low_V"] = h.vectors(0, rank, N, np.float64)

phase("headtail")                   # T below XMCA_TRIDIAG_VEC_MIN_N: the sweeps, so the head / tail route; rotate_solved reads the head rows
h.set_field(0, field(3, np.float64, 600))
rank = h.solve(1)
res = h.rotate_solved(n_rot, power=1, tol=1e-8)             # no join
out["headtail_V"] = h.vectors(0, rank, N, np.float64)       # joins
out["headtail_R_before"], out["headtail_R_after"] = res["R"], h.rotate_solved(n_rot, power=1, tol=1e-8)["R"]

phase("f32")                        # a float32 field keeps the head / tail route, its vectors resident in float32
h32 = _hip.Handle(0)
h32.set_field(0, field(2, np.float32))
h32.solve(1)
rank = h32.solve(1)
res = h32.rotate_solved(n_rot, power=1, tol=1e-8)           # no join
out["f32_V"] = h32.vectors(0, rank, N, np.float32)          # joins
out["f32_R_before"], out["f32_R_after"] = res["R"], h32.rotate_solved(n_rot, power=1, tol=1e-8)["R"]
h32.close()
h.close()
np.savez(dst, **out)
"""


def _run(tmp, defer):
    dst = os.path.join(tmp, "on.npz" if defer else "off.npz")
    env = dict(os.environ, XMCA_DEFER_BACKPROJECT="1" if defer else "0", XMCA_DEFER_HEAD="128", XMCA_TRACE="solve")
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, dst, str(T), str(N), str(N_ROT), str(LOW_RANK)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    phases, name = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@phase "):
            name = line.split()[1]
            phases[name] = []
        elif name:
            phases[name].append(line)
    return dict(np.load(dst)), {k: "\n".join(v) for k, v in phases.items()}


@pytest.fixture(scope="module")
def runs():
    with tempfile.TemporaryDirectory() as tmp:
        return _run(tmp, True), _run(tmp, False)


LEAD, TAIL = "by the skinny kernel", "deferred to the second stream"


def test_the_deferred_child_took_the_lead_route_and_the_inline_one_deferred_nothing(runs):
    (_, on), (_, off) = runs
    assert on["main"].count(LEAD) == 1 and on["main"].count(TAIL) == 1, on["main"]      # the second solve; the first is serial
    assert on["class"].count(LEAD) == 1, on["class"]
    assert off["main"].count(LEAD) == 1 and off["class"].count(LEAD) == 1, off["main"]      # the same kernel, in line
    for text in off.values():
        assert TAIL not in text


def test_leading_modes_before_the_join_are_the_modes_behind_it_and_the_inline_ones(runs):
    (on, _), (off, _) = runs
    assert np.array_equal(on["lead_before"], on["lead_after"])
    assert np.array_equal(on["lead_before"], on["V"][:N_ROT])
    assert np.array_equal(on["lead_before"], off["lead_before"])
    assert np.array_equal(off["lead_before"], off["V"][:N_ROT])
    norms = np.linalg.norm(on["V"], axis=1)
    assert on["V"].shape == (T, N) and np.all(np.abs(norms - 1.0) < 1e-6), (norms.min(), norms.max())


def test_every_array_agrees_between_the_modes_bit_for_bit(runs):
    (on, _), (off, _) = runs
    assert sorted(on) == sorted(off)
    for key in sorted(on):
        assert on[key].dtype == off[key].dtype and on[key].shape == off[key].shape, key
        assert np.array_equal(on[key], off[key]), key               # vectors, singular values, both rotations, the class


def test_rotate_solved_rotates_what_rotate_loadings_gets_from_the_leading_modes(runs):
    (on, _), _ = runs
    # (the same loadings up to how the device and numpy round sqrt(sigma): a rotation of a stale or unwritten buffer is far off)
    assert np.allclose(on["solved_R"], on["loadings_R"], rtol=0, atol=1e-8)


def test_repeated_eigenvalues_still_go_to_the_sweeps_and_match_numpy(runs):
    (on, trace), _ = runs
    assert LEAD not in trace["lowrank"], trace["lowrank"]
    X = on["low_field"]
    U, s, Vh = np.linalg.svd(X, full_matrices=False)
    sig_ref = s ** 2 / (T - 1)
    k = LOW_RANK - 1                                              # the centred field has rank LOW_RANK - 1
    assert np.max(np.abs(on["low_sigma"][:k] - sig_ref[:k]) / sig_ref[:k]) < 1e-5
    lead = 5                                                      # well separated by the graded rows
    ph = np.sign(np.sum(Vh[:lead] * on["low_V"][:lead], axis=1))
    assert np.max(np.abs(on["low_V"][:lead] * ph[:, None] - Vh[:lead])) < 1e-5


def test_a_float32_field_keeps_the_head_and_tail_route(runs):
    (on, trace), _ = runs
    assert trace["f32"].count(TAIL) == 1 and LEAD not in trace["f32"], trace["f32"]
    assert "modes [128, %d)" % T in trace["f32"]
    assert on["f32_V"].dtype == np.float32 and on["f32_V"].shape == (T, N)


@pytest.mark.parametrize("name,rows", [("headtail", 600), ("f32", T)])
def test_rotate_solved_beside_a_head_and_tail_solve_reads_complete_rows(runs, name, rows):
    """xmca_rotate_solved skips the join on the head / tail route as well (float64 plane, float32-resident plane): the rotation of
    the head rows before the join is the rotation behind it, and the in-line mode's (compared by the test of every array)."""
    (on, trace), (off, _) = runs
    assert trace[name].count(TAIL) == 1 and LEAD not in trace[name] and "modes [128, %d)" % rows in trace[name], trace[name]
    assert np.array_equal(on[name + "_R_before"], on[name + "_R_after"])
    assert np.array_equal(on[name + "_R_before"], off[name + "_R_before"])
    assert on[name + "_V"].shape == (rows, N)
    assert np.all(np.isfinite(on[name + "_R_before"])) and abs(abs(np.linalg.det(on[name + "_R_before"])) - 1.0) < 1e-6
