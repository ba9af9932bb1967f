"""The chunked column pass of xmca_amd/csrc/column_pass.h restated in numpy, and the shapes on its edges.

One thread per column; the rows cut into chunks = min(32, rows) chunks of ceil(rows / chunks) consecutive rows (trailing chunks
may be empty); a float64 partial per (chunk, column), rows ascending; the partials added chunk 0 first.  `chunked_sum` makes the
same additions in the same order (float -> double is exact and nothing reassociates), so it gives the device's bits."""
import numpy as np

COL_CHUNKS = 32
ROWS = (2, 3, 31, 32, 33, 63, 65)       # one row per chunk, a short last chunk, empty trailing chunks (33: 17 used, 65: 22 used)
COLS = (1, 255, 257)                    # below and above the 256 columns of a workgroup
DTYPES = (np.float64, np.float32)


def col_chunks(rows):
    return min(COL_CHUNKS, rows)


def chunk_ranges(rows, chunks=None):
    """[r0, r1) of every chunk; r0 == r1 for an empty one"""
    chunks = col_chunks(rows) if chunks is None else chunks
    per = -(-rows // chunks)
    return [(min(rows, k * per), min(rows, k * per + per)) for k in range(chunks)]


def chunked_sum(X64, chunks=None, where=None):
    """Column sums of the float64 rows x cols array X64 in the order of the device.  where: a boolean array of the same shape, only
    its entries are added (the present entries of a field with gaps)."""
    X64 = np.asarray(X64)
    assert X64.dtype == np.float64 and X64.ndim == 2
    total = np.zeros(X64.shape[1])
    for r0, r1 in chunk_ranges(X64.shape[0], chunks):
        part = np.zeros(X64.shape[1])
        for r in range(r0, r1):
            np.add(part, X64[r], out=part, where=True if where is None else where[r])
        total = total + part
    return total


def field(rows, cols, dtype, seed, offset=None, spread=None):
    """A rows x cols field of `dtype`: normal values around an offset in [-5, 5) with a spread in [0.5, 4), or as given"""
    rng = np.random.default_rng([seed, rows, cols])
    offset = rng.uniform(-5, 5) if offset is None else offset
    spread = rng.uniform(0.5, 4.0) if spread is None else spread
    return (offset + spread * rng.standard_normal((rows, cols))).astype(dtype)


def with_gaps(X):
    """X with NaNs by column, c mod 5: 0 the first row, 1 the last row, 2 the whole of chunk 1, 3 everything but one entry, 4 none.
    Every column keeps a present entry (a field of one row keeps all of them)."""
    X = X.copy()
    rows, cols = X.shape
    if rows == 1:
        return X
    r0, r1 = chunk_ranges(rows)[1]
    for c in range(cols):
        kind = c % 5
        if kind == 0:
            X[0, c] = np.nan
        elif kind == 1:
            X[rows - 1, c] = np.nan
        elif kind == 2:
            X[r0:r1, c] = np.nan
        elif kind == 3:
            keep = X[rows // 2, c]
            X[:, c] = np.nan
            X[rows // 2, c] = keep
    return X
