"""GPU: `xmca_amd.lagged.lead_lag_maps` - the four kernels of csrc/lead_lag.h.  The numpy restatement, the longdouble
truth and the cases: tests/lead_lag_cases.py (T around the R = 8 rows of a piece, N in {1, C - 1, C, C + 1, 4 C + 1} around the
C = 256 columns of a workgroup, q in {1, 2, 3, 5, 8}, lag lists of length {1, G - 1, G, G + 1, 2 G + 1} around the group G(q), nine gap
patterns, both dtypes, both dof modes).

Bounds.  `pairs`, `dof` and the NaN positions of r, slope and p equal the restatement's exactly, every entry: no decision of a
committed case sits on a threshold (tests/test_lead_lag_host.py).  r and slope stay within the allowance `lead_lag_cases.bounds`
computes per entry in longdouble from the truth's own sums, nothing of it measured: with u = 2^-53 and n pairs,
d(Cab) = 2 (n + 6) u [sum |a' b'| + sum |a'| sum |b'| / n], dr = dCxy / sqrt(Cxx Cyy) + (|r| / 2) (dCxx / Cxx + dCyy / Cyy) + 2 u |r|,
dslope = dCxy / Cyy + |slope| dCyy / Cyy + 2 u |slope|, allowance 2 d, plus half a float32 spacing at the value for a float32
field.  p is compared with scipy at the device's own rounded r and dof, within the allowance of tests/test_gpu_patterns.py: the
p-value kernel's bound 64 * 2^-52 (1 + a |ln(x (1 - x))|) p plus scipy's own error (1e-12 relative where p >= 1e-250, 1e-8 between
1e-290 and 1e-250, absolute 1e-289 below).  Worst error / bound measured on an MI355X: profiles/lead_lag_accuracy.json, written by
scripts/lead_lag_accuracy.py."""
import numpy as np
import pytest

try:
    import torch                                            # (before the first device call of the session, as the other torch tests do)
except Exception:
    torch = None

import lead_lag_cases as C
from xmca_amd import _hip
from xmca_amd.array import MCA, _two_sided_p
from xmca_amd.lagged import center_index, lag1_index, lead_lag_maps

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
KEYS = ("r", "slope", "p", "dof", "pairs")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in KEYS) and ("lag1" in a) == ("lag1" in b) \
        and ("lag1" not in a or np.array_equal(_bits(a["lag1"]), _bits(b["lag1"])))


def _call(hip, case, dtype, dof, lags=None):
    return lead_lag_maps(C.case_field(case, dtype), C.case_index(case), case[4] if lags is None else lags, min_pairs=case[6], dof=dof, handle=hip)


def p_ratio(p, r, dof):
    """the worst |p - scipy| / allowance over the entries with a p-value (those below 1e-290 are compared absolutely)"""
    ok = ~np.isnan(p)
    assert np.array_equal(ok, ~np.isnan(r) & (dof >= 3))
    if not ok.any():
        return 0.0
    p, r, n_obs = p[ok], np.asarray(r, dtype=np.float64)[ok], dof[ok].astype(np.float64)
    ref = _two_sided_p(r, n_obs)
    assert np.all((p >= 0) & (p <= 1))
    low = ref < 1e-290
    assert np.all(np.abs(p[low] - ref[low]) <= 1e-289)
    p, r, n_obs, ref = p[~low], r[~low], n_obs[~low], ref[~low]
    a, x = n_obs / 2 - 1, (1.0 - np.abs(r)) / 2
    allow = 64 * EPS * (1 + a * np.abs(np.log(x) + np.log1p(-x))) * ref + np.where(ref >= 1e-250, 1e-12, 1e-8) * ref
    return float(np.max(np.abs(p - ref) / allow)) if p.size else 0.0


def _truth(X, y, lags, min_pairs=8, dof="n"):
    """(longdouble truth, allowance of r, allowance of slope) of a call"""
    truth = C.restate(X, y, lags, min_pairs, dof, real=np.longdouble)
    br, bs = C.bounds(truth, str(np.asarray(X).dtype))
    return truth, br, bs


def test_the_cases_know_the_tile_of_the_library():
    cols, rows, groups = _hip.lead_lag_tile()
    assert (cols, rows, groups) == (C.C, C.R, C.GROUPS)
    Ts, Ns = ({c[i] for c in C.CASES} for i in (1, 2))
    assert {rows - 1, rows, rows + 1, 2 * rows + 1} <= Ts and {1, cols - 1, cols, cols + 1, 4 * cols + 1} <= Ns
    for q in (1, 2, 3, 5, 8):
        G = groups[q - 1]
        lengths = {len(c[4]) for c in C.CASES if c[3] == q}
        assert lengths <= {1, G - 1, G, G + 1, 2 * G + 1}, (q, lengths)
        assert any(n % G for n in lengths) and any(n >= G for n in lengths), (q, lengths)          # a partial group and a whole one


# ---- against the restatement and the longdouble truth ------------------------------------------------------------------------------
@pytest.mark.parametrize("dof", C.DOFS)
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("case", C.CASES, ids=C.case_name)
def test_against_the_restatement(hip, case, dtype, dof):
    name, T, N, q, lags, pattern, min_pairs = case
    L = len(lags)
    got = _call(hip, case, dtype, dof)
    rest, truth, br, bs = C.reference(name, dtype, dof)
    assert set(got) == set(KEYS) | {"lags"} | ({"lag1"} if dof == "bretherton" else set())
    assert all(isinstance(got[k], np.ndarray) for k in got)
    assert got["r"].dtype == got["slope"].dtype == np.dtype(dtype) and got["p"].dtype == np.float64
    assert got["dof"].dtype == got["pairs"].dtype == np.int32 and got["lags"].dtype == np.int64 and tuple(got["lags"]) == tuple(lags)
    assert got["r"].shape == got["slope"].shape == got["p"].shape == got["dof"].shape == (L, N, q) and got["pairs"].shape == (L, N)
    live = rest["live"]
    assert np.array_equal(got["pairs"], rest["pairs"])                                 # every entry, exactly
    assert np.array_equal(got["dof"], rest["dof"])
    assert np.array_equal(np.isnan(got["r"]), ~live) and np.array_equal(np.isnan(got["slope"]), ~live)
    assert np.array_equal(np.isnan(got["p"]), ~live | (rest["dof"] < 3))
    assert not np.isinf(got["r"]).any() and not np.isinf(got["slope"]).any()
    assert np.all(np.abs(got["r"][live]) <= 1)
    wr, ws = C.worst_ratio(got["r"], truth["r"], br, live), C.worst_ratio(got["slope"], truth["slope"], bs, live)
    wp = p_ratio(got["p"], got["r"], got["dof"])
    print(name, dtype, dof, "live %d of %d" % (live.sum(), live.size), "error / bound: r %.3g slope %.3g p %.3g" % (wr, ws, wp))
    assert wr <= 1.0 and ws <= 1.0 and wp <= 1.0
    if dof == "bretherton":
        assert got["lag1"].shape == (N,) and got["lag1"].dtype == np.float64
        assert np.array_equal(got["lag1"] == 0.0, rest["lag1"] == 0.0)
        # rho = (sp / |P|) / (sq / n0): two chains of at most T products and three divisions.  sum_P |x'_t x'_{t+1}| <= sq, so the
        # first-order error of rho is at most (T + 4) 2^-53 (n0 / |P| + |rho|); the allowance is twice that.
        present = ~np.isnan(C.case_field(case, dtype))
        n0, np_ = present.sum(axis=0), (present[1:] & present[:-1]).sum(axis=0)
        allow = 2 * (T + 4) * C.U * (n0 / np.maximum(np_, 1) + np.abs(truth["lag1"]))
        assert np.all(np.abs(got["lag1"] - truth["lag1"]) <= allow)


# ---- checks that need no reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
def test_a_column_used_as_its_own_index_gives_one(hip, dtype):
    rng = np.random.default_rng(4)
    T, N = 97, 257
    X = (10.0 + rng.standard_normal((T, N))).astype(dtype)
    y = X[:, [5, 200]].astype(np.float64)
    out = lead_lag_maps(X, y, [0], handle=hip)
    truth, br, bs = _truth(X, y, [0])
    for j, n in enumerate((5, 200)):
        assert abs(np.longdouble(out["r"][0, n, j]) - 1) <= br[0, n, j] and abs(np.longdouble(out["slope"][0, n, j]) - 1) <= bs[0, n, j]
        assert out["p"][0, n, j] == 0.0 and out["dof"][0, n, j] == T
    assert np.all(out["p"][0, :, 0][np.arange(N) != 5] > 0)


@pytest.mark.parametrize("d", [0, 3, -7])
def test_a_delayed_index_peaks_at_its_delay(hip, d):
    rng = np.random.default_rng(9)
    T, N = 120, 6
    y = rng.standard_normal(T) + 2.0
    X = 10.0 + rng.standard_normal((T, N))
    X[:, 2] = np.nan
    lo, hi = max(0, d), min(T, T + d)
    X[lo:hi, 2] = 3.0 * y[lo - d:hi - d] - 4.0          # x[t] = 3 y[t - d] - 4 where that step exists
    lags = list(range(-9, 10))
    out = lead_lag_maps(X, y, lags, handle=hip)
    truth, br, bs = _truth(X, y, lags)
    at = lags.index(d)
    r = out["r"][:, 2, 0]
    assert np.argmax(r) == at and out["pairs"][at, 2] == T - abs(d)
    assert abs(np.longdouble(r[at]) - 1) <= br[at, 2, 0] and abs(np.longdouble(out["slope"][at, 2, 0]) - 3) <= bs[at, 2, 0]
    assert np.all(np.delete(r, at) < 0.9)


def test_swapping_field_and_index_mirrors_the_lag(hip):
    """r(x, y; l) pairs (y[s], x[s + l]); with the roles swapped and the lag -l the pairs are the same ones.  Each call stays within its
    own allowance of its own truth, and the truths are one number: the difference is at most the sum of the two."""
    case = C.case_by_name("long-lags")          # gap-free
    X, y = C.case_field(case)[:, :40], C.case_index(case)[:, 0]
    lags = [0, 5, -17, 150, -292]
    a = lead_lag_maps(X, y, lags, handle=hip)
    ta, bra, _ = _truth(X, y, lags)
    for n in (0, 7, 39):
        b = lead_lag_maps(y[:, None].copy(), X[:, n], [-l for l in lags], handle=hip)
        tb, brb, _ = _truth(y[:, None], X[:, n], [-l for l in lags])
        assert np.array_equal(a["pairs"][:, n], b["pairs"][:, 0]) and np.array_equal(a["dof"][:, n, 0], b["dof"][:, 0, 0])
        assert np.all(np.abs(a["r"][:, n, 0].astype(np.longdouble) - b["r"][:, 0, 0]) <= bra[:, n, 0] + brb[:, 0, 0])


@pytest.mark.parametrize("dof", C.DOFS)
def test_an_affine_change_of_units_scales_the_slope_and_keeps_r(hip, dof):
    """x -> a x + b, y -> c y + d with dyadic a, c: mathematically r is multiplied by sign(a c) and slope by a / c; pairs and dof do not
    move (the conditions of tests/test_lead_lag_host.py keep n f away from an integer).  Each call stays within its own allowance of
    its own truth; the two truths differ by the rounding of the transformed inputs, one 2^-53 per element of x' and y', which moves
    Cab by at most 2 * 2^-53 sum |a' b'| - less than 1 / (n + 6) of the first-order part of an allowance that is twice that part."""
    case = C.case_by_name("q3-wide")
    X, y, lags = C.case_field(case), C.case_index(case), list(case[4])
    a, b, c, d = -4.0, 8.0, np.array([0.5, -2.0, 8.0]), np.array([-2.0, 1.0, 0.25])
    one = lead_lag_maps(X, y, lags, min_pairs=case[6], dof=dof, handle=hip)
    two = lead_lag_maps(a * X + b, c * y + d, lags, min_pairs=case[6], dof=dof, handle=hip)
    t1, br1, bs1 = _truth(X, y, lags, case[6], dof)
    t2, br2, bs2 = _truth(a * X + b, c * y + d, lags, case[6], dof)
    assert np.array_equal(one["pairs"], two["pairs"]) and np.array_equal(one["dof"], two["dof"])
    live = t1["live"]
    assert np.array_equal(np.isnan(two["r"]), ~live) and live.any()
    sign, scale = np.sign(a * c)[None, None, :], (a / c)[None, None, :]
    r1, r2 = one["r"].astype(np.longdouble), two["r"].astype(np.longdouble)
    s1, s2 = one["slope"].astype(np.longdouble), two["slope"].astype(np.longdouble)
    assert np.all(np.abs(r2 - sign * r1)[live] <= (br1 + br2)[live])
    assert np.all(np.abs(s2 - scale * s1)[live] <= (np.abs(scale) * bs1 + bs2)[live])


def test_lag_zero_on_a_pc_is_the_homogeneous_pattern(hip):
    """Lag 0, gap-free, dof = 'n', index = the PCs: r is what `homogeneous_patterns` returns, which forms the same centred moments by
    a GEMM - sums of the same T products in another order, under the same first-order bound: twice the allowance."""
    rng = np.random.default_rng(21)
    T, N, k = 60, 300, 3
    F = rng.standard_normal((T, 5)) @ rng.standard_normal((5, N)) + 0.3 * rng.standard_normal((T, N)) + 10.0
    m = MCA(F, handle=hip)
    m.solve()
    pcs = m.pcs(k)["left"]
    want_r, want_p = (res["left"] for res in m.homogeneous_patterns(k))
    out = lead_lag_maps(F, pcs, [0], min_pairs=8, dof="n", handle=hip)
    truth, br, _ = _truth(F, pcs, [0])
    assert np.all(out["dof"] == T) and not np.isnan(out["r"]).any() and want_r.shape == (N, k)
    assert np.all(np.abs(out["r"][0].astype(np.longdouble) - want_r) <= 2 * br[0])
    assert p_ratio(out["p"][0], out["r"][0], out["dof"][0]) <= 1.0 and p_ratio(want_p, want_r, np.full((N, k), T)) <= 1.0
    moved = np.abs(_two_sided_p(out["r"][0], T) - _two_sided_p(want_r, T))          # what the difference of the two r's moves p by
    ref = _two_sided_p(out["r"][0], T)
    x = (1.0 - np.abs(out["r"][0])) / 2
    allow = 64 * EPS * (1 + (T / 2 - 1) * np.abs(np.log(x) + np.log1p(-x))) * ref + 1e-12 * ref + 1e-289
    assert np.all(np.abs(out["p"][0] - want_p) <= 2 * allow + moved)


# ---- bits --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("name", ["run", "q3-wide", "q8-plus", "long-lags"])
def test_a_call_repeats_its_bits_and_a_lag_does_not_see_the_other_lags(hip, name, dtype):
    case = C.case_by_name(name)
    lags = list(case[4])
    G = C.GROUPS[case[3] - 1]
    for dof in C.DOFS:
        whole = _call(hip, case, dtype, dof)
        assert _same_bits(whole, _call(hip, case, dtype, dof))                             # a repeated call
        cut = G + 1 if len(lags) > G + 1 else 1                                            # the first call ends inside a lag group
        first, rest = _call(hip, case, dtype, dof, lags[:cut]), _call(hip, case, dtype, dof, lags[cut:])
        for k in KEYS:                                                                     # a lag list split in two calls
            assert np.array_equal(_bits(np.concatenate([first[k], rest[k]])), _bits(whole[k])), (dof, k)
        order = np.random.default_rng(len(lags)).permutation(len(lags))
        mixed = _call(hip, case, dtype, dof, [lags[i] for i in order])                     # a permuted lag list
        assert tuple(mixed["lags"]) == tuple(lags[i] for i in order)
        for k in KEYS:
            assert np.array_equal(_bits(mixed[k]), _bits(whole[k][order])), (dof, k)
        if dof == "bretherton":
            assert np.array_equal(_bits(first["lag1"]), _bits(whole["lag1"])) and np.array_equal(_bits(mixed["lag1"]), _bits(whole["lag1"]))


# ---- tensors -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("layout", ["contiguous", "transposed", "column slice", "three dimensions"])
def test_a_gpu_tensor_gives_gpu_tensors_with_the_bits_of_the_numpy_route(hip, layout, dtype):
    case = C.case_by_name("q8-group")
    name, T, N, q, lags, pattern, min_pairs = case
    X, y = C.case_field(case, dtype), C.case_index(case)
    dev = torch.device("cuda", hip.device)
    if layout == "contiguous":
        t = torch.from_numpy(X.copy()).to(dev)
    elif layout == "transposed":
        t = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev).T
        assert t.stride() == (1, T)
    elif layout == "column slice":
        wide = torch.full((T, N + 30), 7.0, dtype=getattr(torch, dtype), device=dev)
        wide[:, 10:10 + N] = torch.from_numpy(X.copy()).to(dev)
        t = wide[:, 10:10 + N]
        assert t.stride() == (N + 30, 1)
    else:
        t = torch.from_numpy(X.copy()).to(dev).reshape(T, 16, 16)
    before = t.clone()
    S = tuple(t.shape[1:])
    for dof in C.DOFS:
        want = lead_lag_maps(X, y, lags, min_pairs=min_pairs, dof=dof, handle=hip)
        out = lead_lag_maps(t, y, lags, min_pairs=min_pairs, dof=dof, handle=hip)
        kinds = dict(r=t.dtype, slope=t.dtype, p=torch.float64, dof=torch.int32, pairs=torch.int32)
        for k in KEYS:
            assert isinstance(out[k], torch.Tensor) and out[k].device == dev and out[k].dtype == kinds[k] and out[k].is_contiguous(), k
            assert tuple(out[k].shape) == (len(lags),) + S + ((q,) if k != "pairs" else ())
            assert np.array_equal(_bits(out[k].cpu().numpy().reshape(want[k].shape)), _bits(want[k])), k
        assert isinstance(out["lags"], np.ndarray) and tuple(out["lags"]) == tuple(lags)
        if dof == "bretherton":
            assert isinstance(out["lag1"], torch.Tensor) and tuple(out["lag1"].shape) == S
            assert np.array_equal(_bits(out["lag1"].cpu().numpy().reshape(-1)), _bits(want["lag1"]))
    assert torch.equal(torch.nan_to_num(t, nan=-1.0), torch.nan_to_num(before, nan=-1.0))          # the input is unchanged
    index = torch.from_numpy(y).to(dev)                                                              # an index on the GPU is fetched
    again = lead_lag_maps(t, index, lags, min_pairs=min_pairs, handle=hip)
    assert np.array_equal(_bits(again["r"].cpu().numpy().reshape(want["r"].shape)), _bits(want["r"]))


def test_a_tensor_with_an_inf_is_refused(hip):
    t = torch.ones(20, 4, dtype=torch.float64, device=torch.device("cuda", hip.device))
    t[3, 1] = float("inf")
    with pytest.raises(ValueError, match="Inf"):
        lead_lag_maps(t, np.arange(20.0), [0], handle=hip)


# ---- state -----------------------------------------------------------------------------------------------------------------------------
def test_a_solved_rotated_model_on_the_handle_keeps_its_result_to_the_bit(hip):
    rng = np.random.default_rng(11)
    F = rng.standard_normal((40, 6)) @ rng.standard_normal((6, 90)) + 0.1 * rng.standard_normal((40, 90))
    m = MCA(F, handle=hip)
    m.solve()
    m.rotate(3)
    before = (m.singular_values().copy(), m.eofs(3)['left'].copy(), m.pcs(3)['left'].copy())
    case = C.case_by_name("run")
    hip.reset_timings()
    _call(hip, case, "float64", "n")
    assert {"lead_lag_center", "lead_lag_moments", "lead_lag_finish"} <= set(hip.timings()) and "lead_lag_lag1" not in set(hip.timings())
    _call(hip, case, "float32", "bretherton")
    assert {"lead_lag_center", "lead_lag_lag1", "lead_lag_moments", "lead_lag_finish"} <= set(hip.timings())
    for a, b in zip(before, (m.singular_values(), m.eofs(3)['left'], m.pcs(3)['left'])):
        assert np.array_equal(_bits(a), _bits(b))
    out = lead_lag_maps(F, m.pcs(3)['left'], range(-3, 4), handle=hip)          # the documented two-line route
    assert out["r"].shape == (7, 90, 3) and np.isfinite(out["r"]).all()


# ---- the C entry -----------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_bad_arguments_before_any_launch(hip):
    """XMCA_ERR_INVALID from the C entry itself (the Python layer checks the same things earlier); the handle stays usable"""
    T, N, q = 20, 3, 2
    rng = np.random.default_rng(0)
    X = rng.standard_normal((T, N)) + 10.0
    Y, _ = center_index(rng.standard_normal((T, q)))
    wide, _ = center_index(rng.standard_normal((T, 9)))
    rho = lag1_index(Y)
    lags = np.array([0, 1, -2], dtype=np.int32)
    many = np.arange(-600, 600, dtype=np.int32)
    r, slope, pv = np.empty((3, N, q)), np.empty((3, N, q)), np.empty((3, N, q))          # (a refused call writes nothing)
    dof, pairs, lag1 = np.zeros((3, N, q), dtype=np.int32), np.zeros((3, N), dtype=np.int32), np.empty(N)
    p = _hip._ptr

    def call(T=T, N=N, stride_t=N, stride_n=1, dtype=_hip.XMCA_F64, Y=Y, q=q, lags=lags, L=3, min_pairs=8, mode=_hip.DOF_N, rho_y=None,
             lag1_out=None, where=_hip.HOST, out_where=_hip.HOST):
        return hip._lib.xmca_lead_lag_maps(hip._h, p(X), where, T, N, stride_t, stride_n, dtype, p(Y), q, p(lags), L, min_pairs, mode, p(rho_y),
                                           p(r), p(slope), p(pv), p(dof), p(pairs), p(lag1_out), out_where)
    assert call() == 0 and np.all(pairs == np.array([20, 19, 18])[:, None]) and np.all(dof == pairs[:, :, None]) and np.isfinite(r).all()
    bad_y = Y.copy()
    bad_y[4, 1] = np.nan
    for bad in (dict(q=0), dict(q=9, Y=wide), dict(L=0), dict(L=-1), dict(lags=many, L=513), dict(lags=np.array([1, 0, 1], dtype=np.int32)),
                dict(lags=np.array([0, 20, 1], dtype=np.int32)), dict(lags=np.array([0, -20, 1], dtype=np.int32)), dict(min_pairs=2),
                dict(Y=bad_y), dict(dtype=7), dict(where=5), dict(out_where=5), dict(stride_t=-1), dict(stride_n=-1), dict(mode=2), dict(mode=-1),
                dict(T=0), dict(N=0), dict(mode=_hip.DOF_BRETHERTON), dict(mode=_hip.DOF_BRETHERTON, rho_y=rho),
                dict(mode=_hip.DOF_BRETHERTON, rho_y=np.array([0.5, 1.5]), lag1_out=lag1)):
        assert call(**bad) == _hip.ERR_INVALID, bad
    with pytest.raises(ValueError, match="T x q"):
        hip.lead_lag_maps(X, Y[:10], lags, 8)
    assert call(mode=_hip.DOF_BRETHERTON, rho_y=rho, lag1_out=lag1) == 0 and np.all(np.abs(lag1) <= 1)
    again = r.copy()
    assert call() == 0 and np.array_equal(_bits(again), _bits(r))


# ---- xarray ----------------------------------------------------------------------------------------------------------------------------
def test_the_xarray_wrapper_returns_the_maps_over_the_dims_of_the_input(hip):
    import os
    import sys
    try:
        import xarray as xr
    except Exception:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_xarray"))
        import xarray as xr
    from xmca_amd import xarray as facade
    case = C.case_by_name("run")
    name, T, N, q, lags, pattern, min_pairs = case
    X, y = C.case_field(case)[:, :65], C.case_index(case)
    da = xr.DataArray(X.reshape(T, 5, 13), dims=["time", "lat", "lon"],
                      coords={"time": np.arange(T), "lat": np.arange(5.0), "lon": np.arange(13.0)}, name="sst", attrs={"units": "K"})
    index = xr.DataArray(y, dims=["time", "mode"], coords={"time": np.arange(T)})
    out = facade.lead_lag_maps(da, index, list(lags), dof="bretherton", handle=hip)
    want = lead_lag_maps(X, y, list(lags), dof="bretherton", handle=hip)
    for k in ("r", "slope", "p", "dof"):
        assert tuple(out[k].dims) == ("lag", "lat", "lon", "index")
        assert np.array_equal(_bits(np.asarray(out[k].values).reshape(want[k].shape)), _bits(want[k]))
        assert np.array_equal(np.asarray(out[k].coords["lag"].values), lags)
    assert tuple(out["pairs"].dims) == ("lag", "lat", "lon") and tuple(out["lag1"].dims) == ("lat", "lon")
