"""The numpy restatement of the chunked column pass (tests/column_pass_cases.py) against exact sums, and its cut."""
import math

import numpy as np
import pytest

import column_pass_cases as P


@pytest.mark.parametrize("rows", (1,) + P.ROWS + (1000,))
def test_chunked_sum_against_exact_sums(rows):
    """a float64 sum of `rows` terms in any order is within rows eps max|x| of the exact one"""
    X = P.field(rows, 7, np.float64, 11)
    got = P.chunked_sum(X)
    exact = np.array([math.fsum(X[:, c]) for c in range(X.shape[1])])
    assert np.all(np.abs(got - exact) <= rows * np.finfo(np.float64).eps * np.abs(X).max(axis=0))
    G = P.with_gaps(X)
    present = ~np.isnan(G)
    got = P.chunked_sum(G, where=present)
    exact = np.array([math.fsum(G[present[:, c], c]) for c in range(G.shape[1])])
    assert np.all(np.abs(got - exact) <= rows * np.finfo(np.float64).eps * np.nanmax(np.abs(G), axis=0))
    assert np.array_equal(P.chunked_sum(X, chunks=1), np.add.accumulate(X, axis=0)[-1])     # one chunk: the rows in order


@pytest.mark.parametrize("rows,used", [(33, 17), (65, 22)])
def test_trailing_chunks_are_empty_where_they_should_be(rows, used):
    ranges = P.chunk_ranges(rows)
    assert len(ranges) == P.COL_CHUNKS == 32
    assert [r1 > r0 for r0, r1 in ranges] == [True] * used + [False] * (32 - used)
    assert ranges[0][0] == 0 and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and ranges[-1][1] == rows


@pytest.mark.parametrize("rows", range(1, 70))
def test_the_chunks_tile_the_rows(rows):
    ranges = P.chunk_ranges(rows)
    assert len(ranges) == min(32, rows)
    assert [r for r0, r1 in ranges for r in range(r0, r1)] == list(range(rows))
