"""A numpy restatement of the neighbour-joining contract of include/distance_hip.h (dst_nj / dst_nj_matrix), bit for bit:
the active list, one round, the compaction schedule and the order of every sum.  Row sums are sequential (one column
added at a time, from +0.0), never np.sum, which sums pairwise.  Also a small Newick parser and split-set
(Robinson-Foulds) helpers for the tree tests."""
import numpy as np

ROOT_PARENT = 0xFFFFFFFF
_SIGN = np.uint64(0x8000000000000000)
_MAG = np.uint64(0x7FFFFFFFFFFFFFFF)
_INF = np.uint64(0x7FF0000000000000)
_ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def nn_key(x):
    """dst_device.hpp's nn_key<false> on f64 values: an unsigned order in which -0 == +0 and NaN is last."""
    bits = np.ascontiguousarray(x, np.float64).view(np.uint64)
    mag = bits & _MAG
    key = np.where(bits >> np.uint64(63) == 1, ~bits, bits | _SIGN)
    key = np.where(mag == 0, _SIGN, key)
    return np.where(mag > _INF, _ALL, key)


def _row_sums(S):
    """r_x = sum of S[k, x] over k in order, from +0.0 (S symmetric with a +0.0 diagonal)."""
    r = np.zeros(S.shape[0])
    for k in range(S.shape[0]):
        r = r + S[k]
    return r


def nj(d):
    """The tree of an n x n matrix (strict upper triangle read): (parent uint32[2n-2], length float64[2n-2])."""
    d = np.asarray(d, np.float64)
    n = d.shape[0]
    assert n >= 3
    iu = np.triu_indices(n, 1)
    S = np.zeros((n, n))
    S[iu] = d[iu]
    S.T[iu] = d[iu]
    parent = np.zeros(2 * n - 2, np.uint32)
    length = np.zeros(2 * n - 2)
    ids = np.arange(n, dtype=np.int64)          # node id by slot
    active = np.ones(n, bool)
    P = n
    r = _row_sums(S)
    upper = np.triu(np.ones((P, P), bool), 1)
    for s in range(n - 3):
        m = n - s
        if m <= (3 * P) // 4:                   # compaction: the active slots in order, r from scratch
            keep = np.flatnonzero(active)
            S = np.ascontiguousarray(S[np.ix_(keep, keep)])
            ids = ids[keep]
            active = np.ones(m, bool)
            P = m
            r = _row_sums(S)
            upper = np.triu(np.ones((P, P), bool), 1)
        Q = (float(m - 2) * S - r[:, None]) - r[None, :]
        valid = upper & active[:, None] & active[None, :]
        # the smallest nn_key, the first in row-major order (= the smallest (a, b)); for a finite minimum that is the
        # first entry equal to it (== treats -0 and +0 alike, as nn_key does)
        v = np.where(valid, Q, np.inf).min()
        if np.isfinite(v):
            flat = int(np.argmax(valid & (Q == v)))
        else:
            keys = nn_key(Q)[valid]
            flat = int(np.flatnonzero(valid.ravel())[int(np.argmin(keys))])
        a, b = divmod(flat, P)
        dab = S[a, b]
        ra, rb = r[a], r[b]
        da = dab * 0.5 + (ra - rb) / float(2 * (m - 2))
        db = dab - da
        u = n + s
        parent[ids[a]], length[ids[a]] = u, da
        parent[ids[b]], length[ids[b]] = u, db
        others = active.copy()
        others[a] = others[b] = False
        dak, dbk = S[a].copy(), S[b].copy()
        duk = ((dak + dbk) - dab) * 0.5
        r = np.where(others, ((r - dak) - dbk) + duk, r)
        S[a, others] = duk[others]
        S[others, a] = duk[others]
        S[a, a] = 0.0
        r[a] = ((ra + rb) - float(m) * dab) * 0.5
        ids[a] = u
        active[b] = False
    x, y, z = np.flatnonzero(active)[:3]
    dxy, dxz, dyz = S[x, y], S[x, z], S[y, z]
    root = 2 * n - 3
    for slot, ln in ((x, ((dxy + dxz) - dyz) * 0.5), (y, ((dxy + dyz) - dxz) * 0.5), (z, ((dxz + dyz) - dxy) * 0.5)):
        parent[ids[slot]], length[ids[slot]] = root, ln
    parent[root], length[root] = ROOT_PARENT, 0.0
    return parent, length


def square(n, payloads):
    """The n x n f64 matrix of a condensed upper triangle (canonical pair order), as dst_nj reads it."""
    D = np.zeros((n, n))
    iu = np.triu_indices(n, 1)
    v = np.asarray(payloads).astype(np.float64)
    D[iu] = v
    D.T[iu] = v
    return D


# ---- trees ----------------------------------------------------------------------------------------------------------
def check_tree(parent, length, n):
    """A dst_nj tree: 2n-2 nodes, root 2n-3, leaves without children, 2 children per internal node, 3 at the root,
    every node reaches the root, lengths finite."""
    parent = np.asarray(parent)
    assert len(parent) == 2 * n - 2 and len(length) == 2 * n - 2
    root = 2 * n - 3
    assert parent[root] == ROOT_PARENT and length[root] == 0.0
    kids = np.bincount(np.delete(parent, root).astype(np.int64), minlength=2 * n - 2)
    assert (kids[:n] == 0).all() and (kids[n:root] == 2).all() and kids[root] == 3
    assert (np.delete(parent, root) > np.arange(2 * n - 2)[np.arange(2 * n - 2) != root]).all()   # joins in id order
    assert np.isfinite(length).all()


def splits(parent, length, n):
    """{split: length} of an unrooted tree whose parents have larger ids than their children (dst_nj output, trees from
    random_tree).  A split is the bitmask (python int) of the side that does not hold leaf 0; the two edges of a root of
    degree 2 give one split, their lengths summed."""
    N = len(parent)
    full = (1 << n) - 1
    mask = [1 << x if x < n else 0 for x in range(N)]
    for x in range(N):
        p = int(parent[x])
        if p != ROOT_PARENT:
            mask[p] |= mask[x]
    out = {}
    for x in range(N):
        if int(parent[x]) == ROOT_PARENT:
            continue
        sp = mask[x] if not mask[x] & 1 else full ^ mask[x]
        if sp == 0 or sp == full:
            continue
        out[sp] = out.get(sp, 0.0) + float(length[x])
    return out


def robinson_foulds(a, b):
    """Symmetric difference of two split sets (dicts or sets)."""
    return len(set(a) ^ set(b))


# ---- Newick -----------------------------------------------------------------------------------------------------------
def parse_newick(text):
    """A minimal Newick reader for dst_newick's output: (names, parent, length) with leaves numbered in order of
    appearance, internal nodes after them in order of closing; quoted names with '' unescaped."""
    if isinstance(text, bytes):
        text = text.decode()
    text = text.strip()
    assert text.endswith(";")
    pos = 0
    names, leaves, internals = [], [], []   # leaves: (name, len, parent_tmp); internals: (len, parent_tmp)

    def name():
        nonlocal pos
        if text[pos] == "'":
            out, pos = [], pos + 1
            while True:
                if text[pos] == "'":
                    if pos + 1 < len(text) and text[pos + 1] == "'":
                        out.append("'")
                        pos += 2
                        continue
                    pos += 1
                    return "".join(out)
                out.append(text[pos])
                pos += 1
        start = pos
        while text[pos] not in ",():;":
            pos += 1
        return text[start:pos]

    def blen():
        nonlocal pos
        if text[pos] != ":":
            return None
        pos += 1
        start = pos
        while text[pos] not in ",();":
            pos += 1
        return float(text[start:pos])

    nodes = []   # (kind, index): parent links filled in as subtrees close

    def subtree():
        nonlocal pos
        if text[pos] == "(":
            pos += 1
            kids = [subtree()]
            while text[pos] == ",":
                pos += 1
                kids.append(subtree())
            assert text[pos] == ")"
            pos += 1
            node = ("i", len(internals))
            internals.append([None, None])
            for k in kids:
                k[1] = node
            ln = blen()
            internals[node[1]][0] = ln
            entry = [node, None]
            for k in kids:
                nodes.append(k)
            return entry
        nm = name()
        node = ("l", len(leaves))
        leaves.append([nm, blen()])
        return [node, None]

    top = subtree()
    nodes.append(top)
    assert text[pos] == ";"
    nl = len(leaves)
    idx = lambda nd: nd[1] if nd[0] == "l" else nl + nd[1]
    N = nl + len(internals)
    parent = np.full(N, ROOT_PARENT, np.int64)
    length = np.zeros(N)
    for nd, par in nodes:
        if par is not None:
            parent[idx(nd)] = idx(par)
        length[idx(nd)] = (leaves[nd[1]][1] if nd[0] == "l" else internals[nd[1]][0]) or 0.0
    return [x[0] for x in leaves], parent, length


# ---- additive trees ---------------------------------------------------------------------------------------------------
def random_tree(n, shape, rng, lo=1, hi=1000):
    """A rooted binary tree on n leaves with integer edge lengths in [lo, hi]: (parent, length) with parents of larger id
    than their children, leaves 0..n-1 (shuffled leaf labels), root 2n-2.  shape: "random", "caterpillar" or
    "balanced"."""
    N = 2 * n - 1
    parent = np.full(N, ROOT_PARENT, np.int64)
    pool = list(rng.permutation(n))
    nxt = n
    if shape == "caterpillar":
        cur = pool[0]
        for leaf in pool[1:]:
            parent[cur] = parent[leaf] = nxt
            cur = nxt
            nxt += 1
    elif shape == "balanced":
        while len(pool) > 1:
            new = []
            for k in range(0, len(pool) - 1, 2):
                parent[pool[k]] = parent[pool[k + 1]] = nxt
                new.append(nxt)
                nxt += 1
            if len(pool) % 2:
                new.append(pool[-1])
            pool = new
    else:
        while len(pool) > 1:
            i, j = sorted(rng.choice(len(pool), 2, replace=False))
            a, b = pool[i], pool[j]
            parent[a] = parent[b] = nxt
            pool.pop(j)
            pool[i] = nxt
            nxt += 1
    assert nxt == N
    length = rng.integers(lo, hi + 1, N).astype(np.float64)
    length[N - 1] = 0.0
    return parent, length


def path_matrix(parent, length, n):
    """Leaf-to-leaf path lengths of a tree whose parents have larger ids (O(n^2) numpy work, O(n) python steps)."""
    N = len(parent)
    D = np.zeros((n, n))
    members = {x: np.array([x]) for x in range(n)}
    to_node = {x: np.zeros(1) for x in range(n)}   # distance of each member leaf to node x
    kids = {}
    for x in range(N):
        p = int(parent[x])
        if p != ROOT_PARENT:
            kids.setdefault(p, []).append(x)
    for x in range(n, N):
        ks = kids[x]
        parts = [(members.pop(k), to_node.pop(k) + length[k]) for k in ks]
        for i in range(len(parts)):
            for j in range(i + 1, len(parts)):
                (ma, da), (mb, db) = parts[i], parts[j]
                block = da[:, None] + db[None, :]
                D[np.ix_(ma, mb)] = block
                D[np.ix_(mb, ma)] = block.T
        members[x] = np.concatenate([p[0] for p in parts])
        to_node[x] = np.concatenate([p[1] for p in parts])
    return D
