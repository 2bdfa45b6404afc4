"""The link rule of dst_links restated in numpy, for the tests: which entries of a full result (the context's own
run_square / run_rect values, canonical order) are links at T, and the connected components of an edge list."""
import numpy as np

INT_MEASURES = ("n", "n_high")


def linked(measure, vals, threshold):
    """The documented rule on DST_OUT_DISTANCE payloads: int64 v <= floor(T), clamped to the int64 range, nothing below
    -2^63; f64 IEEE v <= T (NaN never, -0.0 as +0.0, +inf links every non-NaN value)."""
    vals = np.asarray(vals)
    if measure in INT_MEASURES:
        f = np.floor(threshold)
        if f < -2.0 ** 63:
            return np.zeros(len(vals), bool)
        return vals <= (np.iinfo(np.int64).max if f >= 2.0 ** 63 else np.int64(f))
    with np.errstate(invalid="ignore"):
        return vals <= threshold


def pairs(n_rows, n_cols, square):
    """(row, col) of every pair in canonical order: square i < j row-major, rectangle i outer / j inner."""
    if square:
        i, j = np.triu_indices(n_rows, 1)
    else:
        i, j = np.divmod(np.arange(n_rows * n_cols, dtype=np.int64), max(n_cols, 1))
    return i.astype(np.uint32), j.astype(np.uint32)


def expected(measure, vals, n_rows, n_cols, square, T):
    """(row, col, vals) of the links in canonical order.  vals: the full result, condensed (square) or n_rows x n_cols."""
    vals = np.asarray(vals).reshape(-1)
    i, j = pairs(n_rows, n_cols, square)
    assert len(vals) == len(i)
    keep = linked(measure, vals, T)
    return i[keep], j[keep], vals[keep]


def components(n, a, b):
    """Labels of the connected components of the edges (a, b): the smallest record of each (hook the larger root under
    the smallest proposed one, then pointer jumping, until every edge lies inside one tree)."""
    parent = np.arange(n, dtype=np.int64)
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    while True:
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
        ra, rb = parent[a], parent[b]
        cross = ra != rb
        if not cross.any():
            return parent.astype(np.uint32)
        lo, hi = np.minimum(ra[cross], rb[cross]), np.maximum(ra[cross], rb[cross])
        np.minimum.at(parent, hi, lo)
        a, b = a[cross], b[cross]
