"""The fore/back-cast analytic signal of solve(complexify=True, extend='exp') as one linear operator along time (no GPU).

`_hip.extended_imag_parts(T, period)` returns the O(T) parts of G with X~ = X + i G X (the device assembles G from them,
csrc/kernels.h extended_operator_kernel).  Assembled here in numpy, G X must equal the imaginary part of the host procedure
`MCA._complexify` (the reference's xmca/array.py:378-472: regression, exponential forecast and backcast, scipy.signal.hilbert
of the 3T-long series, trim, remove_mean) for any centered field.
"""
import numpy as np
import pytest

from xmca_amd import _hip
from xmca_amd.array import MCA


def _assemble(T, period):
    col3, hbar, U, W = _hip.extended_imag_parts(T, period)
    assert col3.shape == (3 * T,) and hbar.shape == (T,) and U.shape == W.shape == (T, 4)
    idx = (np.arange(T)[:, None] - np.arange(T)[None, :]) % (3 * T)
    return col3[idx] - hbar[None, :] + U @ W.T


def _host_model(T, period):
    """a bare MCA carrying just what `_complexify` reads"""
    m = MCA.__new__(MCA)
    m._keys = ['left']
    m._n_observations = {'left': T}
    m._analysis = {'extend': 'exp', 'theta_period': period}
    return m


@pytest.mark.parametrize("T", [40, 63, 64, 492, 1000])
@pytest.mark.parametrize("period", [1, 6, 12])
def test_operator_equals_host_extension(T, period):
    rng = np.random.default_rng(T + 100 * period)
    t = np.arange(T)[:, None]
    X = rng.standard_normal((T, 9)) + 0.02 * t * rng.standard_normal((1, 9)) + np.cos(2 * np.pi * t / 37.0)   # trends: the edge case
    X = X - X.mean(axis=0)
    ref = _host_model(T, period)._complexify({'left': X})['left']
    G = _assemble(T, period)
    rel = np.max(np.abs(G @ X - ref.imag)) / np.max(np.abs(ref.imag))
    assert rel < 1e-12, rel
    assert np.max(np.abs(ref.real - X)) < 1e-12 * np.max(np.abs(X))


def test_operator_structure():
    """Row means of G X vanish (remove_mean), and on centered input the extensions add rank 3 to the centered middle block."""
    T, period = 64, 12
    G = _assemble(T, period)
    assert np.max(np.abs(G.sum(axis=0))) < 1e-12 * T
    col3 = _hip.hilbert_imag_column(3 * T)
    idx = (np.arange(T)[:, None] - np.arange(T)[None, :]) % (3 * T)
    P = np.eye(T) - 1.0 / T
    low = P @ (G - P @ col3[idx]) @ P
    s = np.linalg.svd(low, compute_uv=False)
    assert np.sum(s > 1e-10 * s[0]) == 3


def test_parts_are_linear_in_time():
    """T = 5000 stays O(T): the parts are vectors and T x 4 blocks, nothing T x T."""
    col3, hbar, U, W = _hip.extended_imag_parts(5000, 12)
    assert col3.nbytes + hbar.nbytes + U.nbytes + W.nbytes < 64 * 5000 * 8
    with pytest.raises(ValueError):
        _hip.extended_imag_parts(1, 12)
