"""CPU: dst_newick, the Newick text of a dst_nj tree — quoting, length text, child order, capacity and malformed parent
arrays — and the restatement's tree helpers on it (no GPU)."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
import nj_reference as R

ROOT = 0xFFFFFFFF
ERR_ARG, ERR_CAPACITY = 1, 6


def raw(parent, length, names, cap=None):
    """(status, text, *len) of one dst_newick call"""
    parent = np.ascontiguousarray(parent, np.uint32)
    length = np.ascontiguousarray(length, np.float64)
    names = [x.encode() for x in names]
    chars = b"".join(names)
    off = np.zeros(len(names) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in names])
    cap = 1 << 16 if cap is None else cap
    buf = C.create_string_buffer(max(cap, 1))
    ln = C.c_size_t(0)
    rc = da.load().dst_newick(len(names), parent.ctypes.data, length.ctypes.data, chars, off.ctypes.data,
                              buf if cap else None, cap, C.byref(ln))
    return rc, buf.raw[:ln.value] if rc == 0 else b"", ln.value


# leaves 0..3; node 4 = (0, 1), root 5 = (2, 3, 4)
P4 = [4, 4, 5, 5, 5, ROOT]
L4 = [1.0, 2.0, 0.5, -0.25, 1.0 / 3.0, 0.0]


def test_text_and_child_order():
    assert da.newick(P4, L4, ["a", "b", "c", "d"]) == \
        b"(c:0.500000000000,d:-0.250000000000,(a:1.000000000000,b:2.000000000000):0.333333333333);\n"
    # children in ascending node id, whatever the order of the leaves' names
    assert da.newick([5, 4, 4, 5, 5, ROOT], L4, ["z", "y", "x", "w"]).startswith(b"(z:1.0")


def test_length_text():
    t = da.newick(P4, [1e-13, -0.0, 123456.5, 2.0 / 3.0, 7.0, 0.0], ["a", "b", "c", "d"])
    assert t == b"(c:123456.500000000000,d:0.666666666667,(a:0.000000000000,b:-0.000000000000):7.000000000000);\n"
    for v in (0.1, 1.0 / 7.0, -2.5, 1e6 / 3.0):
        assert da.format_distance("raw", v).encode() in da.newick(P4, [v] * 5 + [0.0], ["a", "b", "c", "d"])


@pytest.mark.parametrize("name,text", [
    ("plain_name", b"plain_name"), ("", b"''"), ("has space", b"'has space'"), ("tab\there", b"'tab\there'"),
    ("it's", b"'it''s'"), ("a(b", b"'a(b'"), ("a)b", b"'a)b'"), ("a[b]", b"'a[b]'"), ("a:b", b"'a:b'"),
    ("a;b", b"'a;b'"), ("a,b", b"'a,b'"), ("''", b"''''''"), ("x|y.z-1/2", b"x|y.z-1/2"),
])
def test_quoting(name, text):
    t = da.newick(P4, L4, [name, "b", "c", "d"])
    assert t.startswith(b"(c:0.500000000000,d:-0.250000000000,(" + text + b":1.000000000000,")
    names, _, _ = R.parse_newick(t)
    assert names[2] == name


def test_capacity():
    rc, text, need = raw(P4, L4, ["a", "b", "c", "d"])
    assert rc == 0 and need == len(text)
    for cap in (0, 1, need - 1):
        rc, _, got = raw(P4, L4, ["a", "b", "c", "d"], cap=cap)
        assert rc == ERR_CAPACITY and got == need
    assert raw(P4, L4, ["a", "b", "c", "d"], cap=need)[1] == text


@pytest.mark.parametrize("parent", [
    [4, 4, 5, 5, 5, 5],               # no root
    [4, 4, 5, 5, ROOT, ROOT],         # two roots
    [4, 4, 5, 5, 6, ROOT],            # out of range
    [4, 4, 5, 4, 5, ROOT],            # 3 children below node 4, 2 at the root
    [4, 5, 5, 5, 5, ROOT],            # 1 child below node 4
    [4, 4, 5, 5, 4, ROOT],            # node 4 its own parent
    [4, 4, 5, 0, 5, ROOT],            # a leaf with a child
    [4, 4, 5, 5, 5, ROOT][:5],        # too short for n = 4 (read as n = 3 leaves: wrong shape)
])
def test_malformed(parent):
    names = ["a", "b", "c", "d"] if len(parent) == 6 else ["a", "b", "c"]
    length = [1.0] * len(parent)
    if len(parent) == 6:
        assert raw(parent, length, names)[0] == ERR_ARG
    else:
        with pytest.raises((da.DistanceError, ValueError)):
            da.newick(parent, length, names)


def test_cycle():
    # 6 leaves, internal 6..8, root 9: 7 and 8 are each other's parent; every child count is right
    parent = [6, 6, 7, 8, 9, 9, 9, 8, 7, ROOT]
    kids = np.bincount([p for p in parent if p != ROOT], minlength=10)
    assert list(kids[6:]) == [2, 2, 2, 3]
    assert raw(parent, [1.0] * 10, list("abcdef"))[0] == ERR_ARG
    good = [6, 6, 7, 7, 8, 8, 9, 9, 9, ROOT]
    assert raw(good, [1.0] * 10, list("abcdef"))[0] == 0


def test_small_n_and_null():
    assert raw([ROOT, 0, 0, 0], [0.0] * 4, ["a", "b"])[0] == ERR_ARG
    rc = da.load().dst_newick(4, None, None, None, None, None, 0, C.byref(C.c_size_t()))
    assert rc == ERR_ARG


def test_round_trip_through_parser():
    rng = np.random.default_rng(4)
    parent, length = R.random_tree(40, "random", rng)
    p, ln = R.nj(R.path_matrix(parent, length, 40))
    names = [f"leaf{i}" for i in range(40)]
    got_names, gp, gl = R.parse_newick(da.newick(p, ln, names))
    assert sorted(got_names) == sorted(names)
    assert len(gp) == 78 and (gp == R.ROOT_PARENT).sum() == 1
    assert sorted(np.round(gl, 12)) == sorted(np.round(ln, 12))
