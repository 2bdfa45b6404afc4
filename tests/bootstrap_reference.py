"""A restatement of the bootstrap contract of include/distance_hip.h (dst_bootstrap_columns, dst_nj_bootstrap,
dst_newick_support): the SplitMix64 column map in Python integers and in numpy, the replicate alignment, the support of a
main tree's splits counted from leaf bitmasks (not Day's intervals, which the library uses), and a reader for Newick text
with support labels."""
import re

import numpy as np

ROOT_PARENT = 0xFFFFFFFF
M64 = (1 << 64) - 1


def column(seed, k, length):
    """The source column of SplitMix64 output number k, in Python integers (mod 2^64 written out)."""
    z = (seed + (k + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z = z ^ (z >> 31)
    return (z * length) >> 64


def columns(seed, replicate, length):
    """The len source columns of one replicate, vectorised: uint64 arithmetic wraps mod 2^64; the high half of the
    128-bit z * len from 32-bit halves of z (len < 2^32)."""
    assert 0 <= length < (1 << 32)
    with np.errstate(over="ignore"):
        k = np.uint64(replicate) * np.uint64(length) + np.arange(length, dtype=np.uint64)
        z = np.uint64(seed) + (k + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        lo32, hi32, L = z & np.uint64(0xFFFFFFFF), z >> np.uint64(32), np.uint64(length)
        return ((hi32 * L + ((lo32 * L) >> np.uint64(32))) >> np.uint64(32)).astype(np.uint32)


def replicate(codes, seed, r):
    """Replicate r of an n x len alignment: column c is source column columns(seed, r, len)[c]."""
    codes = np.asarray(codes)
    return np.ascontiguousarray(codes[:, columns(seed, r, codes.shape[1])])


# ---- splits -------------------------------------------------------------------------------------------------------
def _below(parent, n):
    """Leaf bitmask below every node of a tree whose parents have larger ids than their children (dst_nj form)."""
    mask = [1 << x if x < n else 0 for x in range(len(parent))]
    for x in range(len(parent)):
        p = int(parent[x])
        if p != ROOT_PARENT:
            mask[p] |= mask[x]
    return mask


def node_splits(parent, n):
    """{internal non-root node x: the side of its split without leaf 0, as a bitmask}."""
    full = (1 << n) - 1
    mask = _below(parent, n)
    return {x: (mask[x] if not mask[x] & 1 else full ^ mask[x])
            for x in range(n, len(parent)) if int(parent[x]) != ROOT_PARENT}


def support(parent, rep_parents, n):
    """support[x] as dst_nj_bootstrap defines it: the replicate trees that hold x's split; UINT32_MAX at leaves and the
    root."""
    main = node_splits(parent, n)
    out = np.full(len(parent), ROOT_PARENT, np.uint32)
    reps = [set(node_splits(p, n).values()) for p in rep_parents]
    for x, sp in main.items():
        out[x] = sum(sp in s for s in reps)
    return out


# ---- Newick with support labels --------------------------------------------------------------------------------------
def strip_labels(text):
    """The Newick text without support labels: a label is the digits between ')' and ':'."""
    return re.sub(rb"\)\d+:", b"):", text) if isinstance(text, bytes) else re.sub(r"\)\d+:", "):", text)


def parse_labelled(text):
    """(names, parent, length, label) of labelled Newick text: leaves numbered in order of appearance, internal nodes
    after them in order of closing (the root last); label[x] is the integer after x's ')' or None."""
    if isinstance(text, bytes):
        text = text.decode()
    text = text.strip()
    assert text.endswith(";")
    pos = 0
    leaves, internals, links = [], [], []   # links: (child, parent) as ("l" | "i", index)

    def name():
        nonlocal pos
        if text[pos] == "'":
            out, pos = [], pos + 1
            while True:
                if text[pos] == "'":
                    if text[pos + 1] == "'":
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

    def tail():
        nonlocal pos
        start = pos
        while text[pos].isdigit():
            pos += 1
        label = int(text[start:pos]) if pos > start else None
        ln = None
        if text[pos] == ":":
            pos += 1
            start = pos
            while text[pos] not in ",();":
                pos += 1
            ln = float(text[start:pos])
        return label, ln

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
            internals.append(tail())
            links.extend((k, node) for k in kids)
            return node
        node = ("l", len(leaves))
        nm = name()
        leaves.append((nm, tail()[1]))
        return node

    subtree()
    assert text[pos] == ";"
    nl = len(leaves)
    idx = lambda nd: nd[1] if nd[0] == "l" else nl + nd[1]   # noqa: E731
    N = nl + len(internals)
    parent = np.full(N, ROOT_PARENT, np.int64)
    length = np.zeros(N)
    label = [None] * N
    for child, par in links:
        parent[idx(child)] = idx(par)
    for k, (_, ln) in enumerate(leaves):
        length[k] = ln or 0.0
    for k, (lab, ln) in enumerate(internals):
        length[nl + k] = ln or 0.0
        label[nl + k] = lab
    return [x[0] for x in leaves], parent, length, label
