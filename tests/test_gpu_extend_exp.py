"""solve(complexify=True, extend='exp', period=theta) on the device against the REAL reference
(scripts/make_extend_goldens.py -> tests/golden/extend_exp_cases.npz).

The fore/back-cast analytic signal is a fixed linear operator along time, X~ = X + i G X (`_hip.extended_imag_parts`,
tests/test_extend_operator.py): the device assembles G and forms G X with its GEMM, in float64 also for float32 input (the
reference extends in float64).  Tolerance: 1e-5 relative as tests/test_gpu_configs.py, the promoted float32 cases included;
singular vectors and PCs phase-aligned per mode (tests/test_gpu_mca.py, gauge note).
"""
import os

import numpy as np
import pytest

from conftest import align_modes
from golden_inputs import GOLDEN_DIR, make_input
from xmca_amd import _hip
from xmca_amd.array import MCA

pytestmark = pytest.mark.gpu
TOL = 1e-5

SOLVE_CASES = ["wide_both", "wide_left", "small_both", "wide_odd", "sst_prcp_p1", "sst_prcp_p6", "sst_prcp_p12", "wide_rot"]
BOOT_CASES = {
    "boot_small": (None, dict(on_left=True, on_right=True, block_size=2)),
    "boot_wide_rot": ((4, 1), dict(on_left=True, on_right=False, block_size=1)),
}


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN_DIR, "extend_exp_cases.npz"))
    return {k: z[k] for k in z.files}


def _fields(gold, case):
    fields = make_input(str(gold[case + "/input"]))
    if case + "/n_fields" in gold:
        fields = fields[:int(gold[case + "/n_fields"])]
    rows = int(gold.get(case + "/rows", -1))
    if rows > 0:
        fields = tuple(f[:rows] for f in fields)
    return fields


def _check_against_gold(m, gold, case, tol=TOL):
    n = gold[case + "/singular_values"].shape[0]
    s = m.singular_values(n)
    assert s.dtype == np.float64                                  # the reference's dtype (complex128 fields), also for float32 input
    assert _rel(s, gold[case + "/singular_values"]) < tol
    pcs = m.pcs(n, rotated=False)
    for k in m._keys:
        V = m._V[k][:, :n]
        assert V.dtype == np.complex128
        Va, ph = align_modes(V, gold[case + "/V_" + k])
        assert _rel(Va, gold[case + "/V_" + k]) < tol, (case, k)
        assert pcs[k].dtype == np.complex128
        assert _rel(pcs[k] / ph, gold[case + "/pcs_" + k]) < tol, (case, k)


@pytest.mark.parametrize("preprocess", ["host", "device"])
@pytest.mark.parametrize("case", SOLVE_CASES)
def test_extend_exp_matches_reference(gold, case, preprocess):
    m = MCA(*_fields(gold, case), preprocess=preprocess)
    m.solve(complexify=True, extend='exp', period=float(gold[case + "/period"]))
    _check_against_gold(m, gold, case)
    if case + "/rot" in gold:
        n_rot, power = (int(v) for v in gold[case + "/rot"])
        m.rotate(n_rot, power)
        assert _rel(m._variance, gold[case + "/rot_variance"]) < TOL
        assert _rel(np.abs(m._rotation_matrix), np.abs(gold[case + "/R"])) < TOL     # R = D^H R_ref D: moduli are gauge-free


def test_no_host_extension_or_hilbert_transform(gold, monkeypatch):
    """The whole flow of an extended model - solve, rotate, pcs, eofs, bootstrapping - without the host procedure."""
    import scipy.signal

    def boom(*a, **k):
        raise AssertionError("host extension / Hilbert transform called")
    monkeypatch.setattr(MCA, "_complexify", boom)
    monkeypatch.setattr(MCA, "_extend", boom)
    monkeypatch.setattr(scipy.signal, "hilbert", boom)
    for preprocess in ("host", "device"):
        m = MCA(*_fields(gold, "wide_rot"), preprocess=preprocess)
        m.solve(complexify=True, extend='exp', period=12)
        _check_against_gold(m, gold, "wide_rot")
        m.rotate(4, 1)
        assert _rel(m._variance, gold["wide_rot/rot_variance"]) < TOL
        assert m.pcs(4)['left'].shape == (64, 4) and m.eofs(4)['right'].shape == (200, 4)
        np.random.seed(5)
        out = m.bootstrapping(3, n_modes=4, **BOOT_CASES["boot_wide_rot"][1])
        assert _rel(out, gold["boot_wide_rot/bootstrap"]) < TOL


@pytest.mark.parametrize("inp", ["wide_both", "small_both"])
def test_device_route_equals_host_route(inp):
    """`_extend_on_host=True` keeps the reference's procedure (host extension, scipy.signal.hilbert, complex upload)."""
    fields = make_input(inp)
    m = MCA(*fields)
    m.solve(complexify=True, extend='exp', period=12)
    h = MCA(*fields)
    h._extend_on_host = True
    h.solve(complexify=True, extend='exp', period=12)
    n = 4
    assert _rel(m.singular_values(n), h.singular_values(n)) < 1e-8
    pm, ph_ = m.pcs(n, rotated=False), h.pcs(n, rotated=False)
    for k in m._keys:
        Va, ph = align_modes(m._V[k][:, :n], h._V[k][:, :n])
        assert _rel(Va, h._V[k][:, :n]) < 1e-8
        assert _rel(pm[k] / ph, ph_[k]) < 1e-8
    # the lazily materialised host copy is the reference's complexified field
    assert _rel(m._fields['left'], h._fields['left']) < 1e-12


@pytest.mark.parametrize("preprocess", ["host", "device"])
def test_handle_reused_by_other_models(gold, preprocess):
    """Another model's solve and a rule_n in between: the extended model uploads again and restores ITS operator."""
    handle = _hip.Handle(0)
    m = MCA(*_fields(gold, "sst_prcp_p6"), handle=handle, preprocess=preprocess)
    m.solve(complexify=True, extend='exp', period=6)
    other = MCA(*make_input("wide_both"), handle=handle, preprocess=preprocess)
    other.solve(complexify=True)
    other.rule_n(2, seed=1)
    _check_against_gold(m, gold, "sst_prcp_p6")
    other.solve(complexify=True)
    n = 4
    pcs = m.pcs(n, rotated=False)
    for k in m._keys:
        _, ph = align_modes(m._V[k][:, :n], gold["sst_prcp_p6/V_" + k])
        assert _rel(pcs[k] / ph, gold["sst_prcp_p6/pcs_" + k]) < TOL
    # a plain complex solve of the same (float32) model afterwards is the float32 path of before
    m.solve(complexify=True)
    assert m.singular_values(2).dtype == np.float32


@pytest.mark.parametrize("case", list(BOOT_CASES))
def test_bootstrapping_on_the_device_runner(gold, case, monkeypatch):
    rot, kw = BOOT_CASES[case]
    m = MCA(*make_input(str(gold[case + "/input"])))
    m.solve(complexify=True, extend='exp', period=12)
    if rot:
        m.rotate(*rot)
    dev = m._device()
    calls = []
    orig = dev.bootstrap_runs

    def spy(*a, **k):
        calls.append(k.get("extend_period"))
        return orig(*a, **k)
    monkeypatch.setattr(dev, "bootstrap_runs", spy)
    np.random.seed(5)
    out = m.bootstrapping(3, n_modes=4, **kw)
    assert calls == [12]
    assert _rel(out, gold[case + "/bootstrap"]) < TOL
    # the reference's loop (one model and solve per replicate) on the same draws
    monkeypatch.setattr(dev, "bootstrap_runs", orig)
    m._bootstrap_on_host = True
    np.random.seed(5)
    host = m.bootstrapping(3, n_modes=4, **kw)
    assert _rel(out, host) < 1e-7
