"""CPU: the entry points of the device bootstrap of extend='theta' models (xmca_bootstrap_runs_theta,
xmca_bootstrap_runs_columns_theta) are declared, exported and bound without a new ABI number, and `dist.sharded_bootstrap` hands
`theta_period` to the device's `bootstrap_runs` only when it is set - a device without that parameter keeps working - with the
same result on the two ranks of a gloo job as in a single process."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from abi_cases import check_entry, header_abi_version, header_arguments

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xmca_bootstrap_runs_theta", "xmca_bootstrap_runs_columns_theta")
N_ARGS = 15                     # of either


def test_header_declares_both_entries_and_keeps_the_abi_number():
    from xmca_amd import _hip
    assert header_abi_version() == _hip.ABI_VERSION
    for name in NEW:
        args = header_arguments(name)
        assert len(args) == N_ARGS
        assert [a.split()[-1].lstrip("*") for a in args[:5]] == ["h", "col3", "hbar", "B", "period"]
        assert args[4] == "int period" and args[-1] == "int64_t n_out"


def test_library_exports_and_binding_declares_both_entries():
    from xmca_amd import _hip
    assert _hip.load_library().xmca_abi_version() == _hip.ABI_VERSION
    for name in NEW:
        check_entry(name, N_ARGS)
    assert _hip.SIGNATURES[NEW[0]] == _hip.SIGNATURES[NEW[1]]


# ---- dist.sharded_bootstrap with stub devices ------------------------------------------------------------------------------------
def _stub_spectra(idx, n_runs, n_out, shift):
    """a deterministic function of the composed row indices of each replicate: independent of how the replicates are dealt"""
    spec = np.stack([idx[r][:n_out] * 3.0 + idx[r].sum() % 11 + shift for r in range(n_runs)]) if n_runs else np.zeros((0, n_out))
    kept = np.array([int(idx[r][0]) % 4 != 1 for r in range(n_runs)], dtype=bool)
    return spec.astype(np.float64), kept


class ThetaStub:
    """a device with the `theta_period` parameter; it records what reached it"""
    device = 0

    def __init__(self):
        self.seen = []

    def bootstrap_runs(self, T, complexify, idx_left, idx_right, n_runs, rotated, p, power, tol, n_out, **kw):
        self.seen.append(dict(kw))
        return _stub_spectra(idx_left, n_runs, n_out, 100.0 * kw.get("theta_period", 0))


class PlainStub:
    """a device from before the parameter existed (the stub of tests/test_dist_gloo.py has this signature)"""
    device = 0

    def bootstrap_runs(self, T, complexify, idx_left, idx_right, n_runs, rotated, p, power, tol, n_out):
        return _stub_spectra(idx_left, n_runs, n_out, 0.0)


def _sharded(dev, idx, **kw):
    sys.path.insert(0, REPO)
    from xmca_amd import dist
    return dist.sharded_bootstrap(dev, len(idx), T=12, complexify=True, idx_left=idx, idx_right=None, rotated=False, p=0, power=1,
                                  tol=1e-8, n_out=5, **kw)


def test_theta_period_reaches_the_device_as_that_keyword():
    idx = np.random.default_rng(100).integers(0, 12, size=(5, 12))
    dev = ThetaStub()
    sp, kept = _sharded(dev, idx, theta_period=4)
    assert dev.seen == [{"theta_period": 4}]
    e_sp, e_kept = _stub_spectra(idx, 5, 5, 400.0)
    assert np.array_equal(sp, e_sp) and np.array_equal(kept, e_kept)
    dev = ThetaStub()
    _sharded(dev, idx, theta_period=4, axis=1)
    assert dev.seen == [{"theta_period": 4, "axis": 1}]


def test_no_theta_period_passes_no_such_keyword():
    idx = np.random.default_rng(100).integers(0, 12, size=(5, 12))
    dev = ThetaStub()
    _sharded(dev, idx, theta_period=None)
    _sharded(dev, idx)
    assert dev.seen == [{}, {}]
    sp, kept = _sharded(PlainStub(), idx, theta_period=None)            # a device without the parameter is called successfully
    e_sp, e_kept = _stub_spectra(idx, 5, 5, 0.0)
    assert np.array_equal(sp, e_sp) and np.array_equal(kept, e_kept)


def _worker(rank, world, port, n_runs, q):
    sys.path.insert(0, REPO)
    import torch.distributed as td
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    rng = np.random.default_rng(100 + rank)          # the ranks draw DIFFERENT indices: rank 0's must be used everywhere
    idx = rng.integers(0, 12, size=(n_runs, 12))
    dev = ThetaStub()
    sp, kept = _sharded(dev, idx, theta_period=4)
    q.put((rank, sp, kept, dev.seen))
    td.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("n_runs", [5, 1])
def test_two_rank_theta_bootstrap_equals_single_process(n_runs):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_runs, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    idx0 = np.random.default_rng(100).integers(0, 12, size=(n_runs, 12))
    e_sp, e_kept = _sharded(ThetaStub(), idx0, theta_period=4)
    for rank, sp, kept, seen in results:
        assert np.array_equal(sp, e_sp) and np.array_equal(kept, e_kept) and kept.dtype == bool
        assert all(kw == {"theta_period": 4} for kw in seen)          # (a rank without replicates does not call the device)
