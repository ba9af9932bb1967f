"""GPU: the twisted-vector stage as four kernels (csrc/tridiag_vec.h, `trd_twisted_vectors`): pivots, twist-index scan over row
segments of TRD_TW_SEG = 64 rows, vector recurrences, scaling - and the Sturm kernel queued in front of the compact-WY
preparation (csrc/jacobi.h).  Through `Handle.tridiag_vectors` / `Handle.eigh`, with the truth, the float64 restatement and the
bars of tests/test_gpu_tridiag_stage.py: every figure in units of eps * bnorm, the device held to 4 * max(r, 1), r the restatement's
own figure on the case.

What the split could get wrong and the single kernel could not: a segment's first or last row, a last segment of one row, the
order in which the segments' minima are combined (the FIRST smallest |gamma| wins, across segments as inside one), columns past
nev, and results that depend on what was queued when."""
import numpy as np
import pytest

import tridiag_stage_cases as C

pytestmark = pytest.mark.gpu

MARGIN = 4.0
SEG = 64                                  # TRD_TW_SEG: rows per segment of the index and the scaling kernel


def _extra_cases():
    out = []
    for n in (191, 192, 193, 255, 256):   # (the other orders around a segment edge are cases of the stage test)
        rng = np.random.default_rng(1000 + n)
        out.append(C.Case("random_n%d" % n, rng.standard_normal(n), rng.standard_normal(n - 1)))
    out.append(C.Case("toeplitz_n65", *C.toeplitz(65), closed="toeplitz"))
    # every vector sits at the row of its own diagonal entry; the last segment is the single row 192
    out.append(C.Case("permuted_ramp_n193_e_0.01", np.random.default_rng(193).permutation(np.arange(1.0, 194.0)), np.full(192, 0.01)))
    # a palindromic matrix: D+_i = D-_{n-1-i} to the last bit, so |gamma_i| = |gamma_{n-1-i}| in every column - in the restatement
    # and on the device alike (both run the same recurrence from either end) - and rows 0 .. 64 tie with rows 129 .. 65
    half = np.random.default_rng(130).permutation(np.arange(1.0, 66.0))
    out.append(C.Case("mirrored_ramp_n130_e_0.01", np.concatenate((half, half[::-1])), np.full(129, 0.01)))
    return {c.name: c for c in out}


EXTRA = _extra_cases()


@pytest.fixture(scope="module", autouse=True)
def cases_of_this_file():
    """the helpers of tridiag_stage_cases look a case up by name: while this module runs they find the cases above as well"""
    stage_case = C.case
    mp = pytest.MonkeyPatch()
    mp.setattr(C, "case", lambda name: EXTRA[name] if name in EXTRA else stage_case(name))
    yield
    mp.undo()


def _abs_gamma(c, lam_scaled):
    """|gamma| (n x m) of the float64 restatement: the pivots as C._twisted forms them"""
    d, e, lam = c.ds, c.es, np.asarray(lam_scaled, dtype=np.float64)
    n, piv = c.n, C.twisted_pivot_floor(c.es)
    Dp, Dm = np.empty((n, lam.size)), np.empty((n, lam.size))
    with np.errstate(all="ignore"):
        x = d[0] - lam
        for i in range(n - 1):
            x = C._floor(x, piv)
            Dp[i] = x
            x = (d[i + 1] - lam) - (e[i] * (1.0 / x)) * e[i]
        Dp[n - 1] = C._floor(x, piv)
        x = C._floor(d[n - 1] - lam, piv)
        Dm[n - 1] = x
        for i in range(n - 2, -1, -1):
            x = C._floor((d[i] - lam) - (e[i] * (1.0 / x)) * e[i], piv)
            Dm[i] = x
    return np.abs((Dp + Dm) - (d[:, None] - lam[None, :]))


def _hold_to_the_bars(name, Y, first=0):
    c = C.case(name)
    lam = C.lam_for_vectors(name)[first:first + Y.shape[1]]
    fig = C.vector_figures(name, Y, first)
    res, ang = C.worst(fig)
    r_res, r_ang = C.worst(C.vector_figures(name, C.restate_vectors(c.ds, c.es, lam * c.f), first))
    print("%s: residual: device %.3f, restatement %.3f; sin(angle) * gap: device %.3f, restatement %.3f eps bnorm; |norm - 1| %.2f eps"
          % (name, res, r_res, ang, r_ang, fig["nrm"].max()))
    assert np.all(np.isfinite(Y)), name
    assert np.all(fig["res"] <= MARGIN * max(r_res, 1.0)), (name, res, r_res, int(np.argmax(fig["res"])))
    held = ~np.isnan(fig["ang"])
    assert np.all(fig["ang"][held] <= MARGIN * max(r_ang, 1.0)), (name, ang, r_ang)
    assert np.all(fig["nrm"] <= c.n / 2 + 3), (name, float(fig["nrm"].max()))


@pytest.mark.parametrize("n", [1, 2, 3, SEG - 1, SEG, SEG + 1, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1, 3 * SEG - 1, 3 * SEG, 3 * SEG + 1,
                               4 * SEG - 1, 4 * SEG, 4 * SEG + 1])
def test_orders_at_and_next_to_a_segment_edge_stay_within_four_times_the_restatement(n, hip):
    """n = 4 * SEG + 1 is also the first order whose index and scaling kernels have a second row of workgroups (four segments each)"""
    name = "random_n%d" % n
    c = C.case(name)
    Y = hip.tridiag_vectors(c.d, c.e, C.lam_for_vectors(name))
    assert Y.shape == (n, n)
    _hold_to_the_bars(name, Y)
    assert np.array_equal(hip.tridiag_vectors(c.d, c.e, C.lam_for_vectors(name)), Y), name


@pytest.fixture(scope="module")
def full_n130(hip):
    c = C.case("random_n130")
    return hip.tridiag_vectors(c.d, c.e, C.lam_for_vectors(c.name))


@pytest.mark.parametrize("nev", [1, 63, 64, 65])
def test_a_partial_call_in_padded_planes_has_the_bits_of_the_full_call(nev, hip, full_n130):
    c = C.case("random_n130")
    lam = C.lam_for_vectors(c.name)
    plane = np.random.default_rng(nev).standard_normal((c.n, nev + 5))
    out = hip.tridiag_vectors(c.d, c.e, lam[c.n - nev:], out=plane)
    assert np.array_equal(out[:, nev:], plane[:, nev:])                              # (neither the scan nor the scaling went past nev)
    assert np.array_equal(out[:, :nev], full_n130[:, c.n - nev:])


def test_a_tie_across_segments_goes_to_the_lower_row(hip):
    """Toeplitz (2, -1), n = 65, at its exact middle eigenvalue 2: d - lam = 0, the pivots alternate between the floor and
    -e^2 / floor from either end, and |gamma| has the same value in every even row 0, 2, .., 64 - the last one in the second
    segment.  The restatement's argmin (the first occurrence) is row 0.  The rows tell which row the device took: below the
    twist row r an odd row has the sign of the row above it, above r the sign of the row below it, and the even rows alternate -
    the signs of ALL rows agree with the restatement's exactly when r = 0."""
    name = "toeplitz_n65"
    c = C.case(name)
    assert C.lam_for_vectors(name)[32] == 2.0
    g = _abs_gamma(c, [2.0 * c.f])[:, 0]
    assert int(np.argmin(g)) == 0 and np.array_equal(np.nonzero(g == g[0])[0], np.arange(0, 65, 2)), g      # a tie indeed, on the CPU
    Yr = C.restate_vectors(c.ds, c.es, [2.0 * c.f])
    Y = hip.tridiag_vectors(c.d, c.e, [2.0])
    assert np.all(Y != 0.0) and np.all(Yr != 0.0)
    assert np.array_equal(np.signbit(Y), np.signbit(Yr)), np.nonzero(np.signbit(Y) != np.signbit(Yr))[0]
    _hold_to_the_bars(name, Y, first=32)


def test_ties_between_mirrored_rows_go_to_the_lower_row_in_every_column(hip):
    """A palindromic matrix: |gamma_i| = |gamma_{129 - i}| to the last bit in every column, rows 0 .. 64 against rows 129 .. 65 -
    two or one segment apart, and rows 64 | 65 inside one.  The vector of a twist row r has z(r) = +1; of a mirrored pair of
    eigenvalues one vector is odd about the middle, so taking row 129 - r instead of r flips its sign, and a vector that stays
    in one half of the matrix then sits in the wrong one."""
    name = "mirrored_ramp_n130_e_0.01"
    c = C.case(name)
    lam = C.lam_for_vectors(name)
    g = _abs_gamma(c, lam * c.f)
    r = np.argmin(g, axis=0)
    col = np.arange(c.n)
    assert np.array_equal(g, g[::-1]) and np.all(r <= 64) and np.array_equal(g[r, col], g[c.n - 1 - r, col])   # ties indeed, on the CPU
    assert {0, SEG - 1, SEG}.issubset(set(r.tolist()))
    Yr = C.restate_vectors(c.ds, c.es, lam * c.f)
    odd = Yr[r, col] * Yr[c.n - 1 - r, col] < -0.25
    local = np.abs(Yr[c.n - 1 - r, col]) < 1e-3                                     # (the vector stays in the half of its twist row)
    assert np.count_nonzero(odd) >= 1 and np.count_nonzero(local) >= 100, (np.count_nonzero(odd), np.count_nonzero(local))
    Y = hip.tridiag_vectors(c.d, c.e, lam)
    assert np.all(Y[r, col] > 0.0), np.nonzero(~(Y[r, col] > 0.0))[0]
    assert np.all(np.abs(Y[r, col]) >= 0.5 * np.max(np.abs(Y), axis=0))
    assert np.all(Y[c.n - 1 - r[odd], col[odd]] < 0.0)
    _hold_to_the_bars(name, Y)


def test_twist_rows_on_the_first_and_last_row_of_a_segment_and_of_the_matrix(hip):
    name = "permuted_ramp_n193_e_0.01"
    c = C.case(name)
    lam = C.lam_for_vectors(name)
    r = np.argmin(_abs_gamma(c, lam * c.f), axis=0)
    assert {0, SEG - 1, SEG, 2 * SEG - 1, 2 * SEG, 3 * SEG - 1, 3 * SEG}.issubset(set(r.tolist())) and 3 * SEG == c.n - 1
    Y = hip.tridiag_vectors(c.d, c.e, lam)
    assert np.array_equal(np.argmax(np.abs(Y), axis=0), r)
    assert np.all(Y[r, np.arange(c.n)] > 0.9)
    _hold_to_the_bars(name, Y)


def test_eigenvalues_do_not_depend_on_what_is_queued_beside_the_sturm_kernel(monkeypatch):
    """A fresh handle: its first decomposition with vectors has no second stream (the compact-WY factors are queued on the
    caller's stream, behind the Sturm kernel), from the second one on they run beside it.  The same bits either way."""
    from xmca_amd import _hip
    monkeypatch.setenv("XMCA_TRIDIAG_VEC_MIN_N", "2")
    n = 257
    rng = np.random.default_rng(257)
    X = rng.standard_normal((n, n + 40))
    G = X @ X.T
    h = _hip.Handle(0)
    lam, U = h.eigh(G)
    assert h.last_eigh_info["tridiag"] == 1
    ref = np.linalg.eigvalsh(G)[::-1]
    assert np.max(np.abs(lam - ref)) < 1e-13 * ref[0]
    for _ in range(2):
        lam2, U2 = h.eigh(G)
        assert h.last_eigh_info["tridiag"] == 1
        assert np.array_equal(lam, lam2) and np.array_equal(U, U2)
