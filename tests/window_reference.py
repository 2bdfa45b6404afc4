"""The definition of dst_run_windows / dst_window_base_counts / dst_sliding_windows restated with numpy and the oracle: a
window's result is the oracle's on contiguous copies of the column slices.  No GPU, no distance_amd."""
import numpy as np

import oracle

WIDTH = {"n": 1, "n_high": 1, "raw": 2, "jc69": 2, "k80": 3, "tn93": 4}
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")


def sliding(length, width, step):
    """begin_k = k step, end_k = min(begin_k + width, length), up to the first k whose end is `length` (with a step above
    the width: or the last that begins below `length`); none for length 0"""
    assert width >= 1 and step >= 1
    out = []
    k = 0
    while k * step < length:
        b = k * step
        e = min(b + width, length)
        out.append((b, e))
        if e == length:
            break
        k += 1
    return np.array(out, np.uint64).reshape(len(out), 2)


def pair_index(square, n_rows, n_cols, rb=0, re=None):
    """(row, col) of every pair of rows [rb, re) in the canonical order of dst_run_square / dst_run_rect"""
    re = n_rows if re is None else re
    rows = np.arange(rb, max(re, rb))
    if square:
        i = np.concatenate([np.full(n_cols - 1 - r, r) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
        j = np.concatenate([np.arange(r + 1, n_cols) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    else:
        i, j = [x.ravel() for x in np.meshgrid(rows, np.arange(n_cols), indexing="ij")]
    return i, j


def expected_tallies(measure, a, b, windows, square=False, rb=0, re=None):
    """(n_windows, P, width) uint32: oracle.tallies_rect on contiguous copies of the column slices, the pairs of rows
    [rb, re) in canonical order (square: a against itself, b ignored)"""
    a = np.asarray(a, np.uint8)
    b = a if square else np.asarray(b, np.uint8)
    re = a.shape[0] if re is None else re
    i, j = pair_index(square, a.shape[0], b.shape[0], rb, re)
    width = WIDTH[measure]
    out = np.zeros((len(windows), i.size, width), np.uint32)
    for w, (lo, hi) in enumerate(np.asarray(windows).tolist()):
        if hi <= lo or not i.size:
            continue
        ca = np.ascontiguousarray(a[:, lo:hi])
        cb = ca if square else np.ascontiguousarray(b[:, lo:hi])
        if not square:
            out[w] = oracle.tallies_rect(measure, ca[rb:re], cb)[:, :, :width].reshape(-1, width)
            continue
        # the square: blocks of rows against the records behind the block's first (the oracle never sees the lower half)
        for r0 in range(rb, re, 32):
            r1 = min(r0 + 32, re)
            if r0 + 1 >= cb.shape[0]:
                break
            block = oracle.tallies_rect(measure, ca[r0:r1], cb[r0 + 1:])
            keep = (i >= r0) & (i < r1)
            out[w, keep] = block[i[keep] - r0, j[keep] - (r0 + 1), :width]
    return out


def expected_counts(codes, windows):
    """(n_windows, n, 4) uint32 {A,T,G,C} by code inside every window"""
    codes = np.asarray(codes, np.uint8)
    out = np.zeros((len(windows), codes.shape[0], 4), np.uint32)
    for w, (lo, hi) in enumerate(np.asarray(windows).tolist()):
        if hi > lo:
            out[w] = oracle.count_bases_matrix(np.ascontiguousarray(codes[:, lo:hi])).astype(np.uint32)
    return out
