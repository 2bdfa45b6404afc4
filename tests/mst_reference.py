"""The definition of dst_mst restated on the host: Kruskal's algorithm over a condensed canonical-order value array.

An edge for every pair (i < j) whose value is not NaN, edges ordered by (nn_key(v), i, j) — a strict total order, so the
minimum spanning forest is unique — and the forest's edges returned in that order."""
import numpy as np

NAN_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
TOP = np.uint64(1 << 63)


def nn_key(vals):
    """The sort key of DST_OUT_DISTANCE payloads (dst_device.hpp: nn_key): int64 -> offset binary; f64 -> the
    order-preserving bit flip, every NaN ~0, -0.0 the key of +0.0."""
    vals = np.ascontiguousarray(vals)
    if vals.dtype == np.int64:
        return vals.view(np.uint64) ^ TOP
    assert vals.dtype == np.float64
    b = vals.view(np.uint64)
    k = np.where((b >> np.uint64(63)) == 1, ~b, b | TOP)
    k[vals == 0] = TOP
    k[np.isnan(vals)] = NAN_KEY
    return k


def kruskal(n, vals):
    """(edges int64[e, 2], values[e]) of the minimum spanning forest of the n records whose condensed square (canonical
    order: i < j row-major) is vals."""
    vals = np.ascontiguousarray(vals)
    i, j = np.triu_indices(n, 1)
    assert len(vals) == len(i)
    key = nn_key(vals)
    keep = np.ones(len(vals), bool) if vals.dtype == np.int64 else ~np.isnan(vals)   # NaN edges are dropped
    i, j, key, v = i[keep], j[keep], key[keep], vals[keep]
    order = np.lexsort((j, i, key))
    i, j, v = i[order], j[order], v[order]
    taken, _ = kruskal_edges(n, i, j)
    return np.stack([i[taken], j[taken]], axis=1).astype(np.int64).reshape(-1, 2), v[taken]


def kruskal_edges(n, i, j, state=None):
    """Kruskal's loop over the edges (i[e], j[e]) in the order given (the caller's (key, i, j) order): (the positions of the
    edges taken, ascending; the union-find state).  `state` from an earlier call continues that forest with edges that
    come later in the order; the loop ends once the forest has n - 1 edges."""
    parent, have = (list(range(n)), 0) if state is None else state

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    taken = []
    for e, (x, y) in enumerate(zip(np.asarray(i).tolist(), np.asarray(j).tolist())):
        if have + len(taken) == n - 1:
            break
        a, b = find(x), find(y)
        if a != b:
            parent[max(a, b)] = min(a, b)
            taken.append(e)
    return np.array(taken, np.int64), (parent, have + len(taken))


def condensed(matrix):
    """The strict upper triangle of a square matrix in canonical order."""
    matrix = np.asarray(matrix)
    return np.ascontiguousarray(matrix[np.triu_indices(len(matrix), 1)])


def components(n, a, b):
    """Labels of the connected components of the edges (a, b): the smallest record of each."""
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


def linked(vals, threshold):
    """dst_clusters' link rule on payloads: int64 v <= floor(T); f64 IEEE v <= T (NaN never)."""
    vals = np.asarray(vals)
    if vals.dtype == np.int64:
        f = np.floor(threshold)
        if f < -2.0 ** 63:
            return np.zeros(len(vals), bool)
        return vals <= (np.iinfo(np.int64).max if f >= 2.0 ** 63 else np.int64(f))
    with np.errstate(invalid="ignore"):
        return vals <= threshold
