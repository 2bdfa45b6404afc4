"""A numpy restatement of the dendrogram contract of include/distance_hip.h (dst_dendrogram / dst_dendrogram_matrix), bit
for bit and deliberately naive: every round takes the global argmin of nn_key over the active upper triangle (the first
occurrence in row-major order is the smallest (a, b)), and the Lance-Williams update is separate elementwise operations
on whole rows.  No row-minimum cache and no library call.  The keys the argmin runs over are stored (K) and patched where
a round changes a distance, because recomputing all n^2 of them every round takes 80 s at n = 1500; every round up to
n = 300, and every 50th round above, K is also recomputed from the distances and the active flags alone and must be
equal, so the stored keys cannot drift from the definition unnoticed."""
import numpy as np

from nj_reference import ROOT_PARENT, nn_key, square  # noqa: F401  (square: re-exported for the tests)

LINKAGES = ("average", "weighted", "complete")
_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def dendrogram(d, linkage="average", trace=None):
    """The tree of an n x n matrix (strict upper triangle read): (parent uint32[2n-1], length, height float64[2n-1]).
    trace: a list that receives (a, b, d_ab) of every round."""
    assert linkage in LINKAGES
    d = np.asarray(d, np.float64)
    n = d.shape[0]
    assert n >= 2
    iu = np.triu_indices(n, 1)
    S = np.zeros((n, n))
    S[iu] = d[iu]
    S.T[iu] = d[iu]
    N = 2 * n - 1
    parent = np.zeros(N, np.uint32)
    length = np.zeros(N)
    height = np.zeros(N)
    node = np.arange(n, dtype=np.int64)     # node id by slot
    size = np.ones(n, dtype=np.int64)
    active = np.ones(n, bool)
    upper = np.triu(np.ones((n, n), bool), 1)

    def keys():
        """nn_key of the active strict upper triangle, every other entry "none" (a finite value's key never is)"""
        return np.where(upper & active[:, None] & active[None, :], nn_key(S), _NONE)

    K = keys()
    for t in range(n - 1):
        if n <= 300 or t % 50 == 0:
            assert np.array_equal(K, keys())
        flat = int(np.argmin(K))              # the first occurrence of the smallest key: the smallest (a, b)
        a, b = divmod(flat, n)
        assert a < b and active[a] and active[b] and K[a, b] != _NONE
        dab = S[a, b]
        if trace is not None:
            trace.append((a, b, dab))
        u = n + t
        hu = dab * 0.5
        for slot in (a, b):
            parent[node[slot]] = u
            length[node[slot]] = hu - height[node[slot]]
        height[u] = hu
        sa, sb = int(size[a]), int(size[b])
        dak, dbk = S[a].copy(), S[b].copy()
        if linkage == "average":
            left = float(sa) * dak
            right = float(sb) * dbk
            total = left + right
            duk = total / float(sa + sb)
        elif linkage == "weighted":
            total = dak + dbk
            duk = total * 0.5
        else:
            duk = np.where(dak < dbk, dbk, dak)
        others = active.copy()
        others[a] = others[b] = False
        S[a, others] = duk[others]
        S[others, a] = duk[others]
        ku = nn_key(duk)
        after = others & (np.arange(n) > a)
        K[a, after] = ku[after]               # (a, k) for k > a, (k, a) for k < a: the upper triangle's entries
        before = others & (np.arange(n) < a)
        K[before, a] = ku[before]
        K[b, :] = _NONE
        K[:, b] = _NONE
        node[a] = u
        size[a] = sa + sb
        active[b] = False
    parent[N - 1] = ROOT_PARENT
    length[N - 1] = 0.0
    return parent, length, height


# ---- trees ----------------------------------------------------------------------------------------------------------
def check_tree(parent, length, height, n):
    """A dst_dendrogram tree: 2n-1 nodes, root 2n-2, leaves without children, 2 children per internal node, parents of
    larger id than their children, finite lengths, leaf heights +0.0."""
    parent = np.asarray(parent)
    N = 2 * n - 1
    assert len(parent) == N and len(length) == N and len(height) == N
    assert parent[N - 1] == ROOT_PARENT and length[N - 1] == 0.0
    kids = np.bincount(parent[:N - 1].astype(np.int64), minlength=N)
    assert (kids[:n] == 0).all() and (kids[n:] == 2).all()
    assert (parent[:N - 1] > np.arange(N - 1)).all()
    assert np.isfinite(length).all() and np.isfinite(height).all()
    assert (height[:n].view(np.uint64) == 0).all()


def children(parent, n):
    """(left, right) child of every internal node n .. 2n-2, in ascending id."""
    N = 2 * n - 1
    kids = [[] for _ in range(N)]
    for x in range(N - 1):
        kids[int(parent[x])].append(x)
    return kids


def leaf_sets(parent, n):
    """The leaves below every node, as index arrays (parents have larger ids than their children)."""
    N = 2 * n - 1
    kids = children(parent, n)
    below = [np.array([x]) if x < n else None for x in range(N)]
    for u in range(n, N):
        below[u] = np.concatenate([below[c] for c in kids[u]])
    return below, kids
