"""GPU: xmca_get_maps (scaled / masked EOFs, amplitude and phase maps in their final layout) against numpy at the edges of its
kernels, its column statistics against an extended-precision truth, and eofs() / spatial_amplitude() / spatial_phase() of the class
on the device route against the numpy route (`_maps_on_host`).

Bounds: a value is within 1e-12 (float64 output) or 2e-6 (float32 output) of the largest finite magnitude of the expected array - the
bounds test_gpu_mca.py holds for the eofs; a divisor (`stat_out`) within 1e-12 relative.  A phase is judged where it is defined:
amplitude * exp(i phase) against the complex value to the same bound, and the angle itself, by circular distance, to 1e3 x that bound
where |z| >= 1e-3 max |z| (an error eps in z turns the angle of such an element by at most 1e3 eps / max |z|)."""
import itertools
import os
import sys

import numpy as np
import pytest

from golden_inputs import gen_C, make_input
from xmca_amd import _hip
from xmca_amd.array import MCA

pytestmark = pytest.mark.gpu

EOF, AMP, PHASE = _hip.MAP_EOF, _hip.MAP_AMPLITUDE, _hip.MAP_PHASE
NONE, MAX, STD = _hip.SCALE_NONE, _hip.SCALE_MAX, _hip.SCALE_STD
VALID = [(EOF, NONE), (EOF, MAX), (EOF, STD), (AMP, NONE), (AMP, MAX), (PHASE, NONE)]
T = 12

_HANDLES = []


def _handle(i=0):
    while len(_HANDLES) <= i:
        _HANDLES.append(_hip.Handle(0))
    return _HANDLES[i]


def _tol(dtype):
    return 2e-6 if np.dtype(dtype) in (np.float32, np.complex64) else 1e-12


def _solve(h, N, cplx, f32, seed, t=T):
    """a seeded random (uncentered: full rank) t x N field solved on `h` -> (rank, N x rank vectors as resident, in float64)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((t, N)).astype(np.float32 if f32 else np.float64)
    h.set_field(0, X)
    if cplx:
        h.complexify(t)
    else:
        h.decomplexify()
    rank = h.solve(1)
    assert rank == min(t, N)
    return rank, np.array(h.vectors(0, rank, N, np.float64).T)


def _masks(N):
    """(keep_idx, N_full): no mask, first and last row masked, every second row masked, all but one row masked (one kept point; for
    more kept points: six of seven rows masked)"""
    rows = np.arange(N, dtype=np.int64)
    return [(None, N), (rows + 1, N + 2), (2 * rows, 2 * N), (np.array([3]), 5) if N == 1 else (7 * rows + 3, 7 * N + 5)]


def _expected(Z, kind, scaling):
    """the reference's formulas (xmca/array.py:690-712, :1090-1093, :1122) on the compact float64 / complex128 values Z"""
    stat = None
    with np.errstate(all="ignore"):
        if kind == EOF:
            e = Z
            if scaling == MAX:
                stat = np.nanmax(abs(e.real), axis=0)
            elif scaling == STD:
                stat = np.nanstd(e.real, axis=0)
        elif kind == AMP:
            e = np.sqrt(Z * Z.conjugate()).real
            if scaling == MAX:
                stat = np.nanmax(e, axis=0)
        else:
            e = np.arctan2(Z.imag, Z.real).real
        if stat is not None:
            e = e / stat
    return e, stat


def _check_values(got, want, tol, what):
    """same NaN and inf pattern; finite values within tol of the largest finite magnitude expected"""
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(np.isinf(got), np.isinf(want)), what
    ok = np.isfinite(want)
    if ok.any():
        scale = max(float(np.max(np.abs(want[ok]))), 1e-300)
        err = float(np.max(np.abs(got[ok].astype(want.dtype) - want[ok])))
        assert err <= tol * scale, (what, err / scale)


def _check_phase(got, z, tol, what):
    """phases `got` against the complex (or real) values z they belong to"""
    assert np.array_equal(np.isnan(got), np.isnan(z)), what
    ok = ~np.isnan(z)
    if not ok.any():
        return
    z, a = np.asarray(z[ok], dtype=np.complex128), got[ok].astype(np.float64)
    assert np.all(np.abs(a) <= np.pi * (1 + 1e-6)), what
    big = float(np.max(np.abs(z)))
    assert np.max(np.abs(np.abs(z) * np.exp(1j * a) - z)) <= tol * max(big, 1e-300), what
    sel = np.abs(z) >= 1e-3 * big
    # circular distance: values next to +-pi are neighbours, whichever side of the cut each landed on
    assert np.max(np.abs(np.angle(np.exp(1j * (a[sel] - np.angle(z[sel])))))) <= 1e3 * tol, what


# ----------------------------------------------------------------------------------------------
# the entry point against numpy
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 773, 2049])
def test_maps_entry_against_numpy(N, cplx, f32):
    """N' below, at and beyond a wave and one, several, odd numbers of workgroups; q at the 8-column register group and (with a
    mixing matrix) the 32-wide tile; every W / factor / (kind, scaling) / mask combination; both output types on either residency."""
    h = _handle()
    rank, V = _solve(h, N, cplx, f32, seed=100 * N + 2 * cplx + f32)
    if f32 and not cplx and N > T:
        assert h.vectors_are_f32(0)                     # the float32-resident route (real float32 field, dual side)
    rng = np.random.default_rng(N)
    masks = _masks(N)
    seen = set()
    for wk, fk, (ki, (kind, scaling)), mi in itertools.product(range(3), range(3), enumerate(VALID), range(4)):
        a = 3 * wk + fk
        q = [1, 8, 9, 33][(a + ki) % 4]                 # (every q with every W kind: ki runs over six values)
        if wk == 0:
            q = min(q, rank)                            # (no mixing matrix: the first q vectors)
        odt = [np.float32, np.float64][(int(not f32) + a // 2) % 2]
        W = None if wk == 0 else rng.standard_normal((rank, q)) + (1j * rng.standard_normal((rank, q)) if wk == 2 else 0)
        f = None if fk == 0 else rng.uniform(0.5, 2.0, q) * (np.exp(1j * rng.uniform(-np.pi, np.pi, q)) if fk == 2
                                                            else rng.choice([-1.0, 1.0], q))
        keep_idx, N_full = masks[mi]
        seen.update({("ks-mask", kind, scaling, mi), ("ks-dtype", kind, scaling, odt), ("ks-f", kind, scaling, fk),
                     ("ks-w", kind, scaling, wk), ("q-w", q, wk)})
        what = dict(N=N, cplx=cplx, f32=f32, q=q, W=wk, factor=fk, kind=kind, scaling=scaling, mask=mi, dtype=odt.__name__)
        m = q if W is None else rank
        got, stat = h.maps(0, N, m, W, f, keep_idx, N_full, kind, scaling, odt, want_stats=True)
        Z = V[:, :q] if W is None else V @ W
        if f is not None:
            Z = Z * f
        want, want_stat = _expected(Z, kind, scaling)
        o_cplx = kind == EOF and (cplx or wk == 2 or fk == 2)
        assert got.dtype == (np.result_type(odt, np.complex64) if o_cplx else np.dtype(odt)), what
        assert got.shape == (N_full, q), what
        rows = np.arange(N) if keep_idx is None else keep_idx
        gone = np.setdiff1d(np.arange(N_full), rows)
        assert np.isnan(got.real[gone]).all() and (not o_cplx or np.isnan(got.imag[gone]).all()), what
        tol = _tol(odt)
        if kind == PHASE:
            _check_phase(got[rows], Z, tol, what)
        else:
            _check_values(got[rows], np.asarray(want), tol, what)
        if scaling == NONE:
            assert np.isnan(stat).all(), what            # (not written)
        else:
            ok = want_stat > 0
            assert np.array_equal(stat > 0, ok) and np.all(np.abs(stat[ok] - want_stat[ok]) <= 1e-12 * want_stat[ok]), (what, stat, want_stat)
        if (kind, scaling) == (EOF, NONE) and f is None:
            assert np.array_equal(got[rows], h.eofs(0, N, m, W, odt)), what          # bit for bit xmca_get_eofs
        if (kind, scaling) == (EOF, STD):
            again, stat2 = h.maps(0, N, m, W, f, keep_idx, N_full, kind, scaling, odt, want_stats=True)
            assert np.array_equal(got, again, equal_nan=True) and np.array_equal(stat, stat2), what
    for ks in VALID:
        assert all(("ks-mask",) + ks + (mi,) in seen for mi in range(4))
        assert all(("ks-dtype",) + ks + (dt,) in seen for dt in (np.float32, np.float64))
        assert all(("ks-f",) + ks + (k,) in seen and ("ks-w",) + ks + (k,) in seen for k in range(3))
    assert all(("q-w", q, wk) in seen for q in (1, 8, 9, 33) for wk in (1, 2))
    assert all(("q-w", min(q, rank), 0) in seen for q in (1, 8, 9, 33))


@pytest.mark.parametrize("cplx", [False, True])
def test_maps_of_33_unmixed_vectors(cplx):
    """W == NULL beyond one 32-wide tile of eof_transpose_kernel (needs rank >= 33: 40 rows here)"""
    h = _handle()
    N, q = 65, 33
    rank, V = _solve(h, N, cplx, False, seed=7, t=40)
    keep_idx, N_full = _masks(N)[2]
    for kind, scaling in VALID:
        got, stat = h.maps(0, N, q, None, None, keep_idx, N_full, kind, scaling, np.float64, want_stats=True)
        want, want_stat = _expected(V[:, :q], kind, scaling)
        if kind == PHASE:
            _check_phase(got[keep_idx], V[:, :q], 1e-12, (kind, scaling))
        else:
            _check_values(got[keep_idx], want, 1e-12, (kind, scaling))
        if scaling != NONE:
            assert np.all(np.abs(stat - want_stat) <= 1e-12 * want_stat)
    assert np.array_equal(h.maps(0, N, q, None, None, keep_idx, N_full, EOF, NONE, np.float64)[keep_idx], h.eofs(0, N, q, None, np.float64))


@pytest.mark.parametrize("N", [773, 41472])
def test_std_of_an_offset_dominated_column(N):
    """First EOF proportional to 1 + 1e-3 g (mean / std = 1000): the divisor of STD within 1e-12 relative of a long-double two-pass
    value on the fetched vector.  The two-pass and merged-moment forms stay within 2e-15 (numpy's nanstd is checked here too); the
    difference of moments E[x^2] - E[x]^2 errs by 6e-12 to 4e-10 on such vectors (printed)."""
    h = _handle()
    rng = np.random.default_rng(N)
    a = 1.0 + 0.5 * rng.uniform(-1, 1, T)
    X = a[:, None] * (1.0 + 1e-3 * rng.standard_normal(N))[None, :]
    X = X + 1e-6 * np.abs(X).max() * rng.standard_normal((T, N))
    h.set_field(0, X)
    h.decomplexify()
    h.solve(1)
    v = h.vectors(0, 1, N, np.float64)[0]
    assert abs(v.mean()) > 500 * v.std()
    x = v.astype(np.longdouble)
    truth = float(np.sqrt(np.mean((x - np.mean(x)) ** 2)))
    out, stat = h.maps(0, N, 1, None, None, None, N, EOF, STD, np.float64, want_stats=True)
    naive = np.sqrt(np.mean(v * v) - np.mean(v) ** 2)
    print("N' = %d: device %.3g, numpy nanstd %.3g, difference of moments %.3g (relative to the long-double value)"
          % (N, abs(stat[0] - truth) / truth, abs(np.nanstd(v) - truth) / truth, abs(naive - truth) / truth))
    assert abs(np.nanstd(v) - truth) <= 1e-12 * truth
    assert abs(stat[0] - truth) <= 1e-12 * truth
    assert np.max(np.abs(out[:, 0] - v / truth)) <= 1e-12 * np.max(np.abs(v / truth))
    again, stat2 = h.maps(0, N, 1, None, None, None, N, EOF, STD, np.float64, want_stats=True)
    assert np.array_equal(out, again) and np.array_equal(stat, stat2)


def test_maps_errors_leave_the_handle_as_it_was():
    h = _handle()
    N = 65
    rank, V = _solve(h, N, True, False, seed=3)
    keep_idx, N_full = _masks(N)[1]
    before = h.maps(0, N, 5, None, None, keep_idx, N_full, EOF, MAX, np.float64)
    eofs = h.eofs(0, N, 5, None, np.float64)
    for kind, scaling in [(AMP, STD), (PHASE, MAX), (PHASE, STD), (EOF, 3), (3, NONE), (-1, NONE)]:
        with pytest.raises(ValueError):
            h.maps(0, N, 5, None, None, keep_idx, N_full, kind, scaling, np.float64)
    bad = keep_idx.copy()
    bad[[10, 11]] = bad[[11, 10]]
    for idx, n_full in [(bad, N_full), (keep_idx, N), (None, N_full), (keep_idx - 2, N_full)]:
        with pytest.raises(ValueError):
            h.maps(0, N, 5, None, None, idx, n_full, EOF, NONE, np.float64)
    with pytest.raises(ValueError):
        h.maps(0, N, rank + 1, None, None, keep_idx, N_full, EOF, NONE, np.float64)       # more modes than were back-projected
    fresh = _hip.Handle(0)
    with pytest.raises(_hip.HipError) as err:
        fresh.maps(0, N, 5, None, None, None, N, EOF, NONE, np.float64)
    assert err.value.code == _hip.ERR_STATE
    assert np.array_equal(h.maps(0, N, 5, None, None, keep_idx, N_full, EOF, MAX, np.float64), before, equal_nan=True)
    assert np.array_equal(h.eofs(0, N, 5, None, np.float64), eofs)
    assert np.array_equal(np.array(h.vectors(0, rank, N, np.float64).T), V)


# ----------------------------------------------------------------------------------------------
# through the class: device route against the numpy route
# ----------------------------------------------------------------------------------------------
def _fields(name):
    if name == "c5_scaled":
        C = gen_C(1200, 144, 288).copy()
        C[:, 3:7, 10:20] = np.nan                        # land points: masked columns
        return (C,)
    return make_input(name)


def _two_models(fields, cplx, rot):
    """the same model twice, device route and numpy route, each on a handle of its own (neither evicts the other's result)"""
    out = []
    for on_host in (False, True):
        m = MCA(*fields, handle=_handle(1 + on_host))
        m._maps_on_host = on_host
        m.solve(complexify=cplx)
        if rot:
            m.rotate(*rot)
        out.append(m)
    return out


def _calls(cplx):
    shift = 0.7 if cplx else 0
    return [("eofs", dict(n=3, scaling='None', phase_shift=shift)), ("eofs", dict(n=3, scaling='max')),
            ("eofs", dict(n=3, scaling='max', phase_shift=shift)), ("eofs", dict(n=2, scaling='std', phase_shift=shift)),
            ("eofs", dict(n=3, scaling='eigen', phase_shift=shift)), ("eofs", dict(n=slice(2, 4), scaling='std')),
            ("eofs", dict(n=4, scaling='max', rotated=False)), ("eofs", dict(n=3)),
            ("spatial_amplitude", dict(n=3, scaling='None')), ("spatial_amplitude", dict(n=3, scaling='max')),
            ("spatial_phase", dict(n=3, phase_shift=shift)), ("spatial_phase", dict(n=slice(2, 3)))]


def _compare_routes(dev, host, cplx):
    """every call of `_calls` on both routes"""
    for fn, kw in _calls(cplx):
        d, s = getattr(dev, fn)(**kw), getattr(host, fn)(**kw)
        plain = host.eofs(**{k: v for k, v in kw.items() if k != 'scaling'})
        assert set(d) == set(s) == set(dev._keys)
        for k in dev._keys:
            what = (fn, kw, k)
            assert d[k].shape == s[k].shape and d[k].dtype == s[k].dtype, (what, d[k].dtype, s[k].dtype)
            assert d[k].flags['C_CONTIGUOUS'], what
            tol = _tol(d[k].dtype)
            if np.iscomplexobj(d[k]):
                assert np.array_equal(np.isnan(d[k].real), np.isnan(d[k].imag)), what        # both planes NaN at masked points
            if fn == "spatial_phase":
                _check_phase(d[k], plain[k], tol, what)
            else:
                _check_values(d[k], s[k], tol, what)
    assert set(dev._V._pending) == set(dev._keys)               # nothing was fetched


@pytest.mark.parametrize("rot", [None, (6, 1), (6, 2)])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name", ["sst_prcp", "wide_both", "wide_both_f32", "c5_scaled"])
def test_class_device_route_matches_numpy_route(name, cplx, rot):
    """Every getter on the device route against a second model with `_maps_on_host`, bounds as in the module docstring.  A float32
    result scaled by 'std' comes from the numpy code on either model: the reference's float32 `np.nanstd` adds the 41 472 squares of
    an unrotated c5_scaled column one after the other in float32 and is 2.5e-5 to 3.4e-5 away from the float64 sums of the device
    (measured on the MI355X), so the class does not hand those out; the entry point itself is held to float64 accuracy above."""
    dev, host = _two_models(_fields(name), cplx, rot)
    _compare_routes(dev, host, cplx)
    # the resident state still serves everything else
    r, p = dev.homogeneous_patterns(3)
    rh, ph = host.homogeneous_patterns(3)
    for k in dev._keys:
        assert np.array_equal(r[k], rh[k], equal_nan=True) and np.array_equal(p[k], ph[k], equal_nan=True)
    dev.rotate(4, 1)
    host.rotate(4, 1)
    for k in dev._keys:
        _check_values(dev.eofs(4, scaling='max')[k], host.eofs(4, scaling='max')[k], _tol(dev._V._dtype), (name, "after rotate", k))
    assert dev._device().holds_result_of(dev) and set(dev._V._pending) == set(dev._keys)


def _refuse(name):
    def refuse(*args, **kwargs):
        raise AssertionError("numpy.%s called" % name)
    return refuse


def test_device_route_makes_no_host_pass(monkeypatch):
    dev, host = _two_models(make_input("sst_prcp"), True, (6, 2))
    want = {i: getattr(host, fn)(**kw) for i, (fn, kw) in enumerate(_calls(True))}
    for name in ("nanmax", "nanstd", "arctan2"):
        monkeypatch.setattr(np, name, _refuse(name))
    for i, (fn, kw) in enumerate(_calls(True)):
        got = getattr(dev, fn)(**kw)
        for k in dev._keys:
            assert got[k].shape == want[i][k].shape and got[k].dtype == want[i][k].dtype
    for fn, kw, called in (("eofs", dict(n=3, scaling='max'), "nanmax"), ("eofs", dict(n=3, scaling='std'), "nanstd"),
                           ("spatial_amplitude", dict(n=3, scaling='max'), "nanmax"), ("spatial_phase", dict(n=3), "arctan2")):
        with pytest.raises(AssertionError, match="numpy.%s called" % called):
            getattr(host, fn)(**kw)


def test_facade_maps_equal_the_plain_class(monkeypatch):
    """the xarray facade's amplitude / phase getters reach the device route through `_NumpyView` and return the plain class's numbers"""
    try:
        import xarray as xr                      # the real package, where it exists
    except Exception:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
        import xarray as xr
    from xmca_amd.xarray import xMCA
    rng = np.random.default_rng(12)
    t, nlat, nlon = 72, 9, 14
    pcs = rng.standard_normal((t, 4)) * np.array([6.0, 4.0, 2.5, 1.5])
    a = (pcs @ rng.standard_normal((4, nlat * nlon)) + 0.4 * rng.standard_normal((t, nlat * nlon))).reshape(t, nlat, nlon)
    a[:, 2, 3] = np.nan                                        # a masked grid point
    a[:, 5, 7:9] = np.nan
    left = xr.DataArray(a, dims=['time', 'lat', 'lon'],
                        coords={'time': np.arange(t), 'lat': np.linspace(-60, 60, nlat), 'lon': np.linspace(0, 130, nlon)})
    xm = xMCA(left, handle=_handle(1))
    m = MCA(a, handle=_handle(2))
    for model in (xm, m):
        model.solve(complexify=True)
        model.rotate(4, 2)
    want_amp, want_phase = m.spatial_amplitude(3, scaling='max'), m.spatial_phase(3, phase_shift=0.4)
    for name in ("nanmax", "nanstd", "arctan2"):
        monkeypatch.setattr(np, name, _refuse(name))
    amp, phase = xm.spatial_amplitude(3, scaling='max'), xm.spatial_phase(3, phase_shift=0.4)
    assert amp['left'].dims == phase['left'].dims == ('lat', 'lon', 'mode')
    assert np.isnan(amp['left'].values[2, 3]).all() and np.isnan(phase['left'].values[5, 7:9]).all()
    assert np.array_equal(amp['left'].values, want_amp['left'], equal_nan=True)
    assert np.array_equal(phase['left'].values, want_phase['left'], equal_nan=True)
    assert np.nanmax.__name__ == "refuse" and set(xm._V._pending) == {'left'}
