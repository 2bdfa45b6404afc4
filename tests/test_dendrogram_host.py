"""CPU: the dendrogram restatement (dendrogram_reference.py) against facts that do not go through it — a 5-leaf UPGMA
tree worked by hand, the max / mean of the input over the leaf pairs across every node's two children — and
dst_newick_rooted: exact text, quoting, capacity, malformed parent arrays; the ABI version and the new symbols."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
import dendrogram_reference as R

ROOT = 0xFFFFFFFF
ERR_ARG, ERR_CAPACITY = 1, 6


# ---- the restatement ----------------------------------------------------------------------------------------------
def hand_matrix():
    d = np.zeros((5, 5))
    for (i, j), v in {(0, 1): 2, (0, 2): 4, (1, 2): 8, (3, 4): 3, (0, 3): 10, (0, 4): 12, (1, 3): 14, (1, 4): 16,
                      (2, 3): 9, (2, 4): 11}.items():
        d[i, j] = v
    return d


def test_upgma_by_hand():
    """d01 = 2, d02 = 4, d12 = 8, d34 = 3, d03 = 10, d04 = 12, d13 = 14, d14 = 16, d23 = 9, d24 = 11.
    round 0: the minimum is d01 = 2: node 5 = (0, 1), h = 1, both lengths 1.  Slot 0 holds {0, 1}, s = 2:
             d(5, 2) = (4 + 8) / 2 = 6, d(5, 3) = (10 + 14) / 2 = 12, d(5, 4) = (12 + 16) / 2 = 14.
    round 1: of 6, 12, 14, d23 = 9, d24 = 11, d34 = 3 the minimum is d34: node 6 = (3, 4), h = 1.5, lengths 1.5.
             Slot 3 holds {3, 4}: d(5, 6) = (12 + 14) / 2 = 13, d(2, 6) = (9 + 11) / 2 = 10.
    round 2: of d(5, 2) = 6, d(5, 6) = 13, d(2, 6) = 10 the minimum is 6: node 7 = (5, 2), h = 3, length[5] = 3 - 1 = 2,
             length[2] = 3.  Slot 0 holds {0, 1, 2}, s = 3: d(7, 6) = (2 * 13 + 1 * 10) / 3 = 12, which is the plain mean of
             10, 12, 14, 16, 9, 11.
    round 3: node 8 = (7, 6), h = 6, length[7] = 6 - 3 = 3, length[6] = 6 - 1.5 = 4.5.  8 is the root.
    Weighted linkage differs in round 2 only: d(7, 6) = (13 + 10) / 2 = 11.5, h_8 = 5.75.  Complete linkage: d(5, 2) = 8,
    d(5, 3) = 14, d(5, 4) = 16, d(6, 5) = 16, d(6, 2) = 11; round 2 joins (5, 2) at 8, h = 4; d(7, 6) = 16, h_8 = 8."""
    d = hand_matrix()
    parent, length, height = R.dendrogram(d, "average")
    assert list(parent) == [5, 5, 7, 6, 6, 7, 8, 8, ROOT]
    assert list(length) == [1, 1, 3, 1.5, 1.5, 2, 4.5, 3, 0]
    assert list(height) == [0, 0, 0, 0, 0, 1, 1.5, 3, 6]
    parent, length, height = R.dendrogram(d, "weighted")
    assert list(parent) == [5, 5, 7, 6, 6, 7, 8, 8, ROOT]
    assert list(height) == [0, 0, 0, 0, 0, 1, 1.5, 3, 5.75] and list(length[5:]) == [2, 4.25, 2.75, 0]
    parent, length, height = R.dendrogram(d, "complete")
    assert list(parent) == [5, 5, 7, 6, 6, 7, 8, 8, ROOT]
    assert list(height) == [0, 0, 0, 0, 0, 1, 1.5, 4, 8] and list(length) == [1, 1, 4, 1.5, 1.5, 3, 6.5, 4, 0]
    R.check_tree(parent, length, height, 5)


def cross_values(d, parent, n):
    """per internal node, D over the leaf pairs across its two children"""
    sym = np.triu(d, 1)
    sym = sym + sym.T
    below, kids = R.leaf_sets(parent, n)
    return [sym[np.ix_(below[kids[u][0]], below[kids[u][1]])] for u in range(n, 2 * n - 1)]


@pytest.mark.parametrize("n", [2, 3, 7, 33, 60])
def test_linkage_properties(n):
    rng = np.random.default_rng(100 + n)
    d = rng.random((n, n)) * 5
    trace = []
    parent, length, height = R.dendrogram(d, "complete", trace)
    R.check_tree(parent, length, height, n)
    for (a, b, dab), cross in zip(trace, cross_values(d, parent, n)):
        assert np.float64(dab).view(np.uint64) == cross.max().view(np.uint64)     # pure selection: bitwise
    assert (np.diff(height[n:]) >= 0).all()
    trace = []
    parent, length, height = R.dendrogram(d, "average", trace)
    R.check_tree(parent, length, height, n)
    for (a, b, dab), cross in zip(trace, cross_values(d, parent, n)):
        assert abs(dab - cross.mean()) <= 1e-12 * cross.mean()
    assert np.array_equal(height[n:], np.array([t[2] for t in trace]) * 0.5)


def test_tie_rule_and_negative_zero():
    d = np.full((6, 6), 1.0)
    trace = []
    R.dendrogram(d, "complete", trace)
    assert [t[:2] for t in trace] == [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5)]
    d = np.full((4, 4), 0.0)
    d[2, 3] = -0.0           # equal to +0.0 under nn_key: (0, 1) stays first
    trace = []
    R.dendrogram(d, "average", trace)
    assert trace[0][:2] == (0, 1)


# ---- dst_newick_rooted ----------------------------------------------------------------------------------------------
def raw(parent, length, names, cap=None):
    """(status, text, *len) of one dst_newick_rooted call"""
    parent = np.ascontiguousarray(parent, np.uint32)
    length = np.ascontiguousarray(length, np.float64)
    assert len(parent) == 2 * len(names) - 1 and len(length) == len(parent)
    names = [x.encode() for x in names]
    chars = b"".join(names)
    off = np.zeros(len(names) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in names])
    cap = 1 << 16 if cap is None else cap
    buf = C.create_string_buffer(max(cap, 1))
    ln = C.c_size_t(0)
    rc = da.load().dst_newick_rooted(len(names), parent.ctypes.data, length.ctypes.data, chars, off.ctypes.data,
                                     buf if cap else None, cap, C.byref(ln))
    return rc, buf.raw[:ln.value] if rc == 0 else b"", ln.value


# leaves 0..3; node 4 = (0, 1), node 5 = (2, 3), root 6 = (4, 5)
P4 = [4, 4, 5, 5, 6, 6, ROOT]
L4 = [1.0, 2.0, 0.5, -0.25, 1.0 / 3.0, 7.0, 0.0]


def test_text():
    assert da.newick_rooted([2, 2, ROOT], [0.5, 0.25, 0.0], ["a", "b"]) == b"(a:0.500000000000,b:0.250000000000);\n"
    assert da.newick_rooted(P4, L4, ["a", "b", "c", "d"]) == \
        b"((a:1.000000000000,b:2.000000000000):0.333333333333,(c:0.500000000000,d:-0.250000000000):7.000000000000);\n"
    # children in ascending node id: leaf 2 before node 5 at the root 6; node 5 = (leaf 3, node 4)
    assert da.newick_rooted([4, 4, 6, 5, 5, 6, ROOT], [1, 2, 3, 4, 5, 6, 0], ["a", "b", "c", "d"]) == \
        b"(c:3.000000000000,(d:4.000000000000,(a:1.000000000000,b:2.000000000000):5.000000000000):6.000000000000);\n"


@pytest.mark.parametrize("name,text", [
    ("plain_name", b"plain_name"), ("", b"''"), ("has space", b"'has space'"), ("it's", b"'it''s'"), ("a(b", b"'a(b'"),
    ("a)b", b"'a)b'"), ("a[b]", b"'a[b]'"), ("a:b", b"'a:b'"), ("a;b", b"'a;b'"), ("a,b", b"'a,b'"),
    ("x|y.z-1/2", b"x|y.z-1/2"),
])
def test_quoting(name, text):
    t = da.newick_rooted(P4, L4, [name, "b", "c", "d"])
    assert t.startswith(b"((" + text + b":1.000000000000,b:")


def test_capacity():
    rc, text, need = raw(P4, L4, ["a", "b", "c", "d"])
    assert rc == 0 and need == len(text)
    for cap in (0, 1, need - 1):
        rc, _, got = raw(P4, L4, ["a", "b", "c", "d"], cap=cap)
        assert rc == ERR_CAPACITY and got == need
    assert raw(P4, L4, ["a", "b", "c", "d"], cap=need)[1] == text


@pytest.mark.parametrize("parent", [
    [4, 4, 5, 5, 6, 6, 6],               # no root
    [4, 4, 5, 5, 6, ROOT, ROOT],         # two roots
    [4, 4, 5, 5, 7, 6, ROOT],            # out of range
    [4, 4, 4, 5, 6, 6, ROOT],            # 3 children below node 4, 1 below node 5
    [4, 5, 5, 5, 6, 6, ROOT],            # 1 child below node 4
    [4, 4, 5, 5, 4, 6, ROOT],            # node 4 its own parent
    [4, 4, 5, 0, 6, 6, ROOT],            # a leaf with a child
    [4, 4, 5, 6, 6, 6, ROOT],            # a root with 3 children (the shape dst_newick wants)
    [4, 4, 5, 5, 6, ROOT, 5],            # the root 5 with 3 children, node 6 with 1
])
def test_malformed(parent):
    assert raw(parent, [1.0] * 7, ["a", "b", "c", "d"])[0] == ERR_ARG


@pytest.mark.parametrize("tail", [ROOT, 0, 5, 6, 7])
def test_nj_shaped_array_in_the_library(tail):
    """dst_nj's tree of 4 leaves (2n - 2 = 6 nodes, a 3-child root at node 5) handed to dst_newick_rooted itself: it reads
    2n - 1 = 7 entries, so whatever follows the six is the seventh, and none makes a binary-rooted tree"""
    assert raw([4, 4, 5, 5, 5, ROOT, tail], [1.0] * 7, ["a", "b", "c", "d"])[0] == ERR_ARG


def test_wrong_length_and_nj_shape():
    with pytest.raises((da.DistanceError, ValueError)):
        da.newick_rooted([4, 4, 5, 5, 5, ROOT], [1.0] * 6, ["a", "b", "c", "d"])   # dst_nj's 2n - 2 nodes
    with pytest.raises((da.DistanceError, ValueError)):
        da.newick_rooted([ROOT], [0.0], ["a"])


def test_cycle():
    # 6 leaves, internal 6..10, root 10: 7 and 8 are each other's parent; every child count is right
    parent = [6, 6, 7, 8, 9, 9, 10, 8, 7, 10, ROOT]
    kids = np.bincount([p for p in parent if p != ROOT], minlength=11)
    assert list(kids[6:]) == [2, 2, 2, 2, 2]
    assert raw(parent, [1.0] * 11, list("abcdef"))[0] == ERR_ARG
    good = [6, 6, 7, 7, 8, 8, 9, 9, 10, 10, ROOT]
    assert raw(good, [1.0] * 11, list("abcdef"))[0] == 0


def test_small_n_and_null():
    assert raw([ROOT], [0.0], ["a"])[0] == ERR_ARG
    rc = da.load().dst_newick_rooted(4, None, None, None, None, None, 0, C.byref(C.c_size_t()))
    assert rc == ERR_ARG


def test_reference_tree_as_text():
    d = hand_matrix()
    parent, length, _ = R.dendrogram(d, "average")
    assert da.newick_rooted(parent, length, list("abcde")) == \
        (b"((d:1.500000000000,e:1.500000000000):4.500000000000,"
         b"(c:3.000000000000,(a:1.000000000000,b:1.000000000000):2.000000000000):3.000000000000);\n")


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_abi():
    lib = da.load()
    assert lib.dst_abi_version() == 3
    for name in ("dst_dendrogram", "dst_dendrogram_matrix", "dst_newick_rooted"):
        assert hasattr(lib, name) and name in da.declared_symbols()
