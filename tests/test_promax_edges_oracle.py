"""The inputs of tests/test_gpu_promax_edges.py on the CPU oracle alone: every case stops with a margin, is well enough
conditioned for the tail comparison, and the tail restated in oracle/promax_edges.py is the tail of ref_numpy.promax."""
import numpy as np
import pytest

from oracle import promax_edges as E
from oracle import ref_numpy as O

SMALL = list(E.CASES)          # every case, the long grids included (a few seconds of host time in all)


@pytest.fixture(scope="module")
def refs():
    return {c: E.oracle_case(c) for c in SMALL}


def test_every_case_stops_with_a_margin_and_bounds_the_tail(refs):
    worst = 0.0
    for case, ref in refs.items():
        at, before = E.stop_margin(ref["ratios"])
        assert at <= E.STOP_BELOW and before >= E.STOP_ABOVE, (case, at, before)
        assert len(ref["ratios"]) == ref["n_iter"]
        noise, cond = E.tail_noise(ref["Bv"], ref["Rv"], case[3], case[4])
        assert cond < 10.0, (case, cond)
        worst = max(worst, noise)
    bound = E.tail_bound(worst)
    assert bound is not None and E.TAIL_FLOOR <= bound <= E.TAIL_CAP


def test_the_slow_input_crosses_one_batch_of_launches():
    ref = E.oracle_case(E.SLOW_CASE, E.wide_loadings)
    assert 32 < ref["n_iter"] < 64 and E.stop_is_clear(ref["ratios"])


def test_restated_tail_is_the_tail_of_the_oracle(refs):
    for case, ref in refs.items():
        B, R, Phi, nl, nr, _ = E.promax_tail(ref["Bv"], ref["Rv"], case[3], case[4])
        assert np.array_equal(B, ref["B"]) and np.array_equal(R, ref["R"]) and np.array_equal(Phi, ref["Phi"]), case
        assert np.array_equal(nl, ref["norm_left"]) and np.array_equal(nr, ref["norm_right"])


def test_extended_tail_agrees_and_tail_bound_is_floored_and_capped(refs):
    case = SMALL[5]
    ref = refs[case]
    a = E.promax_tail(ref["Bv"], ref["Rv"], case[3], case[4])
    b = E.promax_tail(ref["Bv"], ref["Rv"], case[3], case[4], extended=True)
    for x, y in zip(a[:5], b[:5]):
        assert E.rel(x, y) < 1e-13
    assert E.tail_bound(1e-17) == E.TAIL_FLOOR and E.tail_bound(2e-14) == pytest.approx(2e-12) and E.tail_bound(2e-12) is None


def test_ratios_do_not_change_the_oracle():
    A = E.edge_loadings(50, 13, False, 300)
    r = []
    got, ref = O.varimax(A, ratios=r), O.varimax(A)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2] == len(r)
    assert r[-1] < 1e-8 <= r[-2]
