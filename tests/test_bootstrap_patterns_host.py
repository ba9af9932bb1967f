"""CPU: `bootstrap_eofs` without a device - the row indices of the moving-block bootstrap, the argument errors and the forwarding
of `indices` (a recorder stands in for the handle), the three ABI entries, and the numpy twin against its definition."""
import numpy as np
import pytest

import bootstrap_patterns_cases as B
from abi_cases import check_entry, header_abi_version
from xmca_amd import _hip
from xmca_amd.array import MCA, bootstrap_row_indices

NEW = {"xmca_bootstrap_patterns": 16, "xmca_pattern_stats": 21, "xmca_pattern_tile": 0}


# ---- bootstrap_row_indices ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,b", [(1, 1), (7, 1), (7, 7), (10, 3), (36, 5), (100, 4)])
def test_row_indices_are_runs_of_consecutive_steps(T, b):
    idx = bootstrap_row_indices(6, T, block_size=b, seed=3)
    assert idx.shape == (6, T) and idx.dtype == np.int64 and idx.flags.c_contiguous
    assert idx.min() >= 0 and idx.max() < T
    for row in idx:
        for start in range(0, T, b):
            block = row[start:start + b]
            assert np.array_equal(block, block[0] + np.arange(block.size))
            assert block[0] + b <= T                                   # a whole block fits where it was drawn, also the cut last one


def test_row_indices_follow_the_seed_and_the_global_generator():
    a, b = bootstrap_row_indices(5, 40, 4, seed=11), bootstrap_row_indices(5, 40, 4, seed=11)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, bootstrap_row_indices(5, 40, 4, seed=12))
    rng = np.random.default_rng(11)                                    # the documented recipe
    starts = rng.integers(0, 40 - 4 + 1, (5, 10))
    assert np.array_equal(a, (starts[..., None] + np.arange(4)).reshape(5, 40)[:, :40])
    np.random.seed(5)
    c = bootstrap_row_indices(3, 20)
    np.random.seed(5)
    assert np.array_equal(c, bootstrap_row_indices(3, 20))
    assert len({tuple(r) for r in bootstrap_row_indices(8, 50, 1, seed=1)}) == 8      # independent draws, one per run


@pytest.mark.parametrize("b", [0, -1, 11])
def test_row_indices_refuse_a_block_that_does_not_fit(b):
    with pytest.raises(ValueError):
        bootstrap_row_indices(3, 10, block_size=b)


# ---- MCA.bootstrap_eofs: errors and forwarding ------------------------------------------------------------------------------
class _Recorder:
    """stands in for the handle: records every call"""
    device = 0

    def __init__(self):
        self.calls = []

    def set_field(self, side, field):
        self.calls.append(('set_field', side, np.array(field)))

    def bootstrap_begin(self, n_fields):
        self.calls.append(('bootstrap_begin', n_fields))

    def bootstrap_patterns(self, T, complexify, idx, n_runs, k, v0_left, v0_right=None):
        self.calls.append(('bootstrap_patterns', T, complexify, np.array(idx), n_runs, k, v0_left, v0_right))
        sides = [v for v in (v0_left, v0_right) if v is not None]
        return ([np.array(v) for v in sides], [np.zeros(v.shape) for v in sides], np.ones((n_runs, k)), np.ones((n_runs, k)),
                np.ones(n_runs, dtype=bool))


def _solved_stand_in(handle, n_modes=4):
    """a 12 x (3 x 2) field, one point masked: the state `solve` leaves, with vectors on the host"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((12, 3, 2))
    x[:, 1, 0] = np.nan
    m = MCA(x, preprocess='host')
    m._handle_override = handle
    m._singular_values = np.arange(float(n_modes), 0.0, -1.0)
    m._analysis['rank'] = 5
    m._V = {'left': np.linalg.qr(rng.standard_normal((5, 5)))[0][:, :n_modes]}
    return m


def test_argument_errors_come_before_any_device_call():
    rec = _Recorder()
    unsolved = MCA(np.random.default_rng(4).standard_normal((12, 6)), preprocess='host')
    unsolved._handle_override = rec
    with pytest.raises(RuntimeError, match="solve"):
        unsolved.bootstrap_eofs(4, 2)
    m = _solved_stand_in(rec)
    for bad in (1, 0, -3, 2.5, True):
        with pytest.raises(ValueError, match="n_runs"):
            m.bootstrap_eofs(bad, 2)
    for bad in (0, 5, 2.0):                                            # 4 modes are held (solve(n_modes=4) of a rank-5 model)
        with pytest.raises(ValueError, match="n_modes"):
            m.bootstrap_eofs(4, bad)
    with pytest.raises(ValueError, match="block_size"):
        m.bootstrap_eofs(4, 2, block_size=13)
    for bad in (np.zeros((4, 11), dtype=int), np.zeros((3, 12), dtype=int), np.zeros((4, 12)), np.full((4, 12), 12), np.full((4, 12), -1)):
        with pytest.raises(ValueError, match="indices"):
            m.bootstrap_eofs(4, 2, indices=bad)
    m._analysis['is_rotated'] = True
    with pytest.raises(ValueError, match="rotated"):
        m.bootstrap_eofs(4, 2)
    m._analysis['is_rotated'] = False
    for extend in ('exp', 'theta'):
        m._analysis['extend'] = extend
        with pytest.raises(ValueError, match="extend"):
            m.bootstrap_eofs(4, 2)
    assert rec.calls == []


def test_indices_are_forwarded_and_the_results_take_the_layout_of_eofs():
    rec = _Recorder()
    m = _solved_stand_in(rec)
    idx = bootstrap_row_indices(4, 12, block_size=3, seed=2)
    out = m.bootstrap_eofs(4, 2, indices=idx)
    names = [c[0] for c in rec.calls]
    assert names == ['set_field', 'bootstrap_begin', 'bootstrap_patterns']
    assert rec.calls[0][2].shape == (12, 5) and np.isrealobj(rec.calls[0][2])          # the kept columns of the centred field
    _, T, cplx, got, n_runs, k, v0_left, v0_right = rec.calls[2]
    assert (T, cplx, n_runs, k) == (12, False, 4, 2) and v0_right is None and np.array_equal(got, idx)
    assert np.array_equal(v0_left, m._V['left'][:, :2])
    assert sorted(out) == ['congruence', 'mean', 'singular_values', 'std']
    assert out['congruence'].shape == (2, 4) and out['singular_values'].shape == (2, 4)
    for name in ('mean', 'std'):
        a = out[name]['left']
        assert a.shape == (3, 2, 2) and np.all(np.isnan(a[1, 0])) and np.isnan(a).sum() == 2
    keep = ~np.isnan(out['mean']['left'][..., 0].reshape(-1))
    assert np.array_equal(out['mean']['left'].reshape(6, 2)[keep], m._V['left'][:, :2])
    # without `indices` the draw of bootstrap_row_indices(seed=) is what reaches the device
    m.bootstrap_eofs(4, 2, block_size=3, seed=2)
    assert np.array_equal(rec.calls[-1][3], idx)


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_bound_and_the_abi_number_stays():
    for name, n_args in NEW.items():
        check_entry(name, n_args)
    assert header_abi_version() == _hip.ABI_VERSION == _hip.load_library().xmca_abi_version()


def test_the_tile_is_a_constant_of_the_build_known_without_a_device():
    tile = _hip.pattern_tile()
    assert isinstance(tile, int) and tile >= 64 and tile % 64 == 0 and tile == _hip.pattern_tile()


# ---- the twin against its definition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("N", [(9,), (9, 6)])
def test_twin_of_replicates_equal_to_the_model_is_the_model(cplx, N):
    fields = B.case_fields(20, N if len(N) == 2 else N[0], 2)
    idx = np.tile(np.arange(20), (3, 1))                               # every replicate is the original
    t = B.twin(fields, idx, 2, cplx)
    for s in range(len(N)):
        assert np.allclose(t['mean'][s], t['v0'][s], rtol=0, atol=1e-14) and np.all(t['std'][s] <= 1e-14)
    assert np.allclose(t['congruence'], 1.0, rtol=0, atol=1e-14)


@pytest.mark.parametrize("cplx", [False, True])
def test_twin_does_not_see_the_sign_or_phase_of_a_replicate(cplx):
    rng = np.random.default_rng(8)
    v0, reps = B.random_replicates(rng, (33, 12), 3, 5, cplx)
    mean, std, g = B.pattern_stats(v0, reps)
    flip = np.exp(2j * np.pi * rng.random((5, 3))) if cplx else rng.choice([-1.0, 1.0], (5, 3))
    mean2, std2, g2 = B.pattern_stats(v0, [[f * v for v in rep] for f, rep in zip(flip, reps)])
    # (the last run has c = 0: it is taken as it comes, so it is left alone here)
    mean3, std3, g3 = B.pattern_stats(v0, [[(f if r < 4 else 1.0) * v for v in rep] for r, (f, rep) in enumerate(zip(flip, reps))])
    for s in range(2):
        assert np.allclose(mean3[s], mean[s], rtol=0, atol=1e-14) and np.allclose(std3[s], std[s], rtol=0, atol=1e-14)
    assert np.allclose(g2, g, rtol=0, atol=1e-14) and g[:, 4].max() == 0.0 and g[:, :4].min() > 0.5


@pytest.mark.parametrize("cplx", [False, True])
def test_twin_is_mean_and_std_of_the_aligned_replicates(cplx):
    """the accumulated form Q - |S|^2 / R against np.mean / np.std(ddof=1) of the aligned vectors themselves"""
    rng = np.random.default_rng(9)
    v0, reps = B.random_replicates(rng, (21,), 2, 6, cplx)
    mean, std, _ = B.pattern_stats(v0, reps)
    aligned = []
    for rep in reps:
        c = (v0[0].conj() * rep[0]).sum(axis=0)
        u = np.where(np.abs(c) > 0, np.conj(c) / np.where(np.abs(c) > 0, np.abs(c), 1), 1.0)
        aligned.append(u * rep[0])
    aligned = np.array(aligned)
    assert np.allclose(mean[0], aligned.mean(axis=0), rtol=0, atol=1e-14)
    assert np.allclose(std[0], np.std(aligned, axis=0, ddof=1), rtol=0, atol=1e-13) and np.isrealobj(std[0])
