"""The sequential definition of dst_representatives in numpy, no GPU: from a condensed canonical-order value vector (what
run_square returns) and the documented link rule.

Records i < j are linked when the pair's DST_OUT_DISTANCE payload satisfies dst_clusters' rule against T.  Walking the
records in input order, record j is a representative iff no representative i < j is linked to it; rep[j] = j then,
otherwise the smallest representative linked to j.  values[j] / tallies[j] are those of the pair (rep[j], j), all-zero
bits for a representative."""
import numpy as np

INT_MEASURES = ("n", "n_high")


def linked(measure, vals, threshold):
    """The documented link rule on DST_OUT_DISTANCE payloads: int64 v <= floor(T) (clamped to the int64 range, nothing
    below -2^63); f64 IEEE v <= T (NaN never, -0.0 as +0.0, +inf every value that is not NaN)."""
    vals = np.asarray(vals)
    if measure in INT_MEASURES:
        f = np.floor(threshold)
        if f < -2.0 ** 63:
            return np.zeros(len(vals), bool)
        return vals <= (np.iinfo(np.int64).max if f >= 2.0 ** 63 else np.int64(f))
    with np.errstate(invalid="ignore"):
        return vals <= threshold


def row_start(n, i):
    """canonical offset of pair (i, i + 1)"""
    return i * (2 * n - i - 1) // 2


def greedy(n, link):
    """rep int64[n] from the condensed link vector (canonical order: row i holds the pairs (i, i + 1 .. n - 1))."""
    link = np.asarray(link, bool)
    assert len(link) == n * (n - 1) // 2
    rep = np.full(n, -1, np.int64)
    for i in range(n):
        if rep[i] >= 0:
            continue   # a member: an earlier representative is linked to it
        rep[i] = i
        s = row_start(n, i)
        later = np.nonzero(link[s:s + n - i - 1])[0] + i + 1
        later = later[rep[later] < 0]   # (a record already taken keeps its smaller representative)
        rep[later] = i
    return rep


def greedy_from_neighbours(n, neighbours):
    """The same pass from adjacency: neighbours(i) -> the records linked to i (any order, both directions known).  For
    sparse graphs that are never written as a condensed vector."""
    rep = np.full(n, -1, np.int64)
    for i in range(n):
        if rep[i] >= 0:
            continue
        rep[i] = i
        nb = np.asarray(neighbours(i), np.int64)
        nb = nb[nb > i]
        nb = nb[rep[nb] < 0]
        rep[nb] = i
    return rep


def reference(measure, vals, n, threshold, tallies=None):
    """(rep uint32[n], values[n] of vals' dtype, tallies uint32[n, W] or None) from the condensed square result (and the
    condensed tallies [pairs, W])."""
    vals = np.asarray(vals)
    rep = greedy(n, linked(measure, vals, threshold))
    j = np.arange(n, dtype=np.int64)
    member = rep != j
    at = row_start(n, rep[member]) + (j[member] - rep[member] - 1)
    values = np.zeros(n, vals.dtype)
    values[member] = vals[at]
    tal = None
    if tallies is not None:
        tallies = np.asarray(tallies)
        tal = np.zeros((n, tallies.shape[1]), np.uint32)
        tal[member] = tallies[at]
    return rep.astype(np.uint32), values, tal


def condensed(n, edges, weight=1, rest=9):
    """A condensed int64 value vector: `weight` on the listed pairs (i, j), `rest` elsewhere."""
    vals = np.full(n * (n - 1) // 2, rest, np.int64)
    for i, j in edges:
        i, j = min(i, j), max(i, j)
        vals[row_start(n, i) + j - i - 1] = weight
    return vals


def check_consequences(n, link, rep, labels=None):
    """The consequences the header states, on a condensed link vector: asserts every one.  labels: the single-linkage
    labels (the smallest record of each cluster) when the cluster statements are to be checked too."""
    link = np.asarray(link, bool)
    rep = np.asarray(rep, np.int64)
    i, j = np.triu_indices(n, 1)
    is_rep = rep == np.arange(n)
    assert n == 0 or is_rep[0]                                  # record 0 is always a representative
    assert not (link & is_rep[i] & is_rep[j]).any()             # no two representatives are linked
    members = np.nonzero(~is_rep)[0]
    assert (rep[members] < members).all() and is_rep[rep[members]].all()
    adj = np.zeros((n, n), bool)
    adj[i, j] = link
    adj |= adj.T
    for m in members:
        linked_reps = np.nonzero(adj[m] & is_rep)[0]
        assert len(linked_reps) and rep[m] == linked_reps.min()   # linked to rep[m], and to no smaller representative
    if labels is not None:
        labels = np.asarray(labels, np.int64)
        assert (labels[rep] == labels).all()                    # a member lies in its representative's cluster
        assert is_rep[np.unique(labels)].all()                  # the smallest record of every cluster is a representative
        assert is_rep.sum() >= len(np.unique(labels))
