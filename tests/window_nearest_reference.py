"""The definition of dst_nearest_windows restated with numpy: from the (n_windows, n_rows, n_cols) DST_OUT_DISTANCE payloads
of every window, the k smallest (key, column record) of every (row, window).  The payloads come from the oracle on the cut
columns (n / n_high / raw) or from any full window result laid out by full_square / full_rect.  No GPU, no distance_amd."""
import numpy as np

import oracle
from window_reference import pair_index

INT_MEASURES = ("n", "n_high")


def keys(vals: np.ndarray) -> np.ndarray:
    """The documented sort key of DST_OUT_DISTANCE payloads (as tests/test_gpu_nearest.py::keys): int64 v ^ 2^63; f64 the
    order-preserving flip, NaN after +inf, -0.0 as +0.0."""
    vals = np.ascontiguousarray(vals)
    if vals.dtype == np.int64:
        return vals.view(np.uint64) ^ np.uint64(1 << 63)
    assert vals.dtype == np.float64
    b = vals.view(np.uint64)
    k = np.where((b >> np.uint64(63)) == 1, ~b, b | np.uint64(1 << 63))
    k[vals == 0] = np.uint64(1 << 63)
    k[np.isnan(vals)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return k


def nearest(payloads: np.ndarray, k: int, square: bool = False, row_begin: int = 0) -> np.ndarray:
    """index[n_rows, n_windows, k_used] from payloads[n_windows, n_rows, n_cols] (row r is record row_begin + r; square: its
    own column is no candidate).  k_used = min(k, candidates per row)."""
    nw, n_rows, n_cols = payloads.shape
    ku = min(k, n_cols - 1 if square else n_cols)
    ku = max(ku, 0)
    out = np.zeros((n_rows, nw, ku), np.uint32)
    if ku == 0:
        return out
    # a stable sort by key leaves equal keys in column order: ascending (key, column)
    order = np.argsort(keys(payloads), axis=2, kind="stable")
    if square:
        own = (row_begin + np.arange(n_rows))[None, :, None]
        order = order[order != own].reshape(nw, n_rows, n_cols - 1)
    return np.ascontiguousarray(order[:, :, :ku].transpose(1, 0, 2)).astype(np.uint32)


def full_square(cond: np.ndarray, n: int) -> np.ndarray:
    """(n_windows, n, n[, width]) from the condensed canonical-order results (n_windows, n (n - 1) / 2[, width]) of the whole
    square: entry (i, j) is the canonical pair's (min(i, j), max(i, j)); the diagonal is zero."""
    i, j = pair_index(True, n, n)
    out = np.zeros((cond.shape[0], n, n) + cond.shape[2:], cond.dtype)
    out[:, i, j] = cond
    out[:, j, i] = cond
    return out


def full_rect(res: np.ndarray, n_rows: int, n_cols: int) -> np.ndarray:
    return res.reshape((res.shape[0], n_rows, n_cols) + res.shape[2:])


def take(full: np.ndarray, index: np.ndarray, row_begin: int = 0) -> np.ndarray:
    """the entries of full[n_windows, rows of the set, n_cols, ...] that index[n_rows, n_windows, k] names, in its layout"""
    n_rows, nw, k = index.shape
    r = (row_begin + np.arange(n_rows))[:, None, None]
    w = np.arange(nw)[None, :, None]
    return full[w, r, index.astype(np.int64)]


def oracle_payloads(measure: str, a, b, windows, square: bool = False) -> np.ndarray:
    """(n_windows, n_a, n_b) payloads of n / n_high / raw from the oracle on contiguous copies of the column slices (square: a
    against itself, symmetric).  An empty window: 0, raw NaN."""
    assert measure in ("n", "n_high", "raw")
    a = np.asarray(a, np.uint8)
    b = a if square else np.asarray(b, np.uint8)
    dtype = np.int64 if measure in INT_MEASURES else np.float64
    out = np.zeros((len(windows), a.shape[0], b.shape[0]), dtype)
    for w, (lo, hi) in enumerate(np.asarray(windows).tolist()):
        if hi <= lo:
            if measure == "raw":
                out[w] = np.nan
            continue
        ca = np.ascontiguousarray(a[:, lo:hi])
        cb = ca if square else np.ascontiguousarray(b[:, lo:hi])
        out[w] = oracle.all_pairs_rect(measure, ca, cb).astype(dtype)
    return out
