"""No GPU: dst_group_summary is declared and exported, its constants are the header's, and the tests' reference
(group_summary_reference) gives hand-computed cells and obeys the consequences the header states."""
import ctypes as C
import re

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from group_summary_reference import GROUPS_MAX, NONE, bits, check_consequences, group_summary
from summary_reference import summary

INF = float("inf")


def test_declared_exported_and_constants():
    assert "dst_group_summary" in _lib.declared_symbols() and "dst_group_summary" in _lib._SIGS
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dst_group_summary")
    lib.dst_abi_version.restype = C.c_int
    assert lib.dst_abi_version() == 3
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+DST_ABI_VERSION\s+3\b", text)
    assert re.search(r"#define\s+DST_GROUPS_MAX\s+1024u", text) and GROUPS_MAX == _lib.GROUPS_MAX == 1024
    assert re.search(r"#define\s+DST_GROUP_NONE\s+0xFFFFFFFFu", text) and NONE == _lib.GROUP_NONE == 0xFFFFFFFF
    assert C.sizeof(_lib.GroupCell) == 56 and [f[0] for f in _lib.GroupCell._fields_] == [
        "pairs", "nan_pairs", "summable_pairs", "links", "sum", "min_bits", "max_bits"]
    assert hasattr(da.Engine, "group_summary")


def test_hand_computed_square():
    """5 records, groups 0 0 1 1 -, n_high values of the pairs (i, j) in canonical order:
    01:1 02:4 03:5 04:9 | 12:3 13:6 14:9 | 23:2 24:9 | 34:9.  Threshold 3."""
    vals = np.array([1, 4, 5, 9, 3, 6, 9, 2, 9, 9], np.int64)
    g = np.array([0, 0, 1, 1, -1])
    r = group_summary("n_high", vals, 5, 5, True, 3.0, g, 2)
    assert r["pairs"].tolist() == [[1, 4], [4, 1]]
    assert r["nan_pairs"].tolist() == [[0, 0], [0, 0]] and r["summable_pairs"].tolist() == [[1, 4], [4, 1]]
    assert r["links"].tolist() == [[1, 1], [1, 1]]                      # 01 | 12 | 23
    assert r["sum"].tolist() == [[1.0, 18.0], [18.0, 2.0]]              # 4 + 5 + 3 + 6
    assert r["min"].tolist() == [[1, 3], [3, 2]] and r["max"].tolist() == [[1, 6], [6, 2]]
    assert r["min"].dtype == np.int64
    # per record, partners by group (record 4 has no group but has a row; nobody counts it as a partner)
    assert r["rec_summable"].tolist() == [[1, 2], [1, 2], [2, 1], [2, 1], [2, 2]]
    assert r["rec_within"].tolist() == [[1, 0], [1, 1], [1, 1], [0, 1], [0, 0]]
    assert r["rec_sum"].tolist() == [[1.0, 9.0], [1.0, 9.0], [7.0, 2.0], [11.0, 2.0], [18.0, 18.0]]
    check_consequences(r, g, True)


def test_hand_computed_rectangle_and_empty_cells():
    """2 x 3 raw values, row groups (1, 0) of 2, column groups (0, -, 2) of 3: one NaN, one -0.0."""
    vals = np.array([[0.5, 0.25, np.nan], [-0.0, 0.125, 0.75]])
    r = group_summary("raw", vals, 2, 3, False, 0.5, [1, 0], 2, [0, NONE, 2], 3)
    assert r["pairs"].tolist() == [[1, 0, 1], [1, 0, 1]]
    assert r["nan_pairs"].tolist() == [[0, 0, 0], [0, 0, 1]]
    assert r["summable_pairs"].tolist() == [[1, 0, 1], [1, 0, 0]]
    assert r["links"].tolist() == [[1, 0, 0], [1, 0, 0]]
    assert r["sum"].tolist() == [[0.0, 0.0, 0.75], [0.5, 0.0, 0.0]]
    b75, b50, none = int(np.float64(0.75).view(np.uint64)), int(np.float64(0.5).view(np.uint64)), 0x7FF8000000000000
    assert bits(r["min"]).tolist() == [[0, none, b75], [b50, none, none]]
    assert np.array_equal(bits(r["min"]), bits(r["max"]))   # (one pair per cell at most; -0.0 comes back as +0.0)
    assert r["rec_summable"].tolist() == [[1, 0, 0], [1, 0, 1]] and r["rec_sum"].tolist() == [[0.5, 0.0, 0.0], [0.0, 0.0, 0.75]]
    check_consequences(r, [1, 0], False)


@pytest.mark.parametrize("measure", ["n", "raw", "tn93"])
@pytest.mark.parametrize("square", [True, False])
def test_consequences_on_random_values(measure, square):
    rng = np.random.default_rng(7)
    nr, nc = (41, 41) if square else (23, 31)
    count = nr * (nr - 1) // 2 if square else nr * nc
    if measure == "n":
        vals = rng.integers(0, 50, count).astype(np.int64)
    else:
        vals = rng.random(count) * 0.3
        for k, v in zip(rng.choice(count, 12, replace=False), [np.nan, np.inf, -np.inf, -0.0] * 3):
            vals[k] = v
    Gr, Gc = 4, (4 if square else 6)
    rg, cg = rng.integers(0, Gr, nr), rng.integers(0, Gc, nc)
    t = 20.0 if measure == "n" else 0.15
    full = group_summary(measure, vals, nr, nc, square, t, rg, Gr, cg, Gc)
    check_consequences(full, rg, square)
    # everyone assigned: dst_summary's totals and per-record results
    want = summary(measure, vals, nr, nc, square, t)
    cells = np.triu(np.ones((Gr, Gc), bool)) if square else np.ones((Gr, Gc), bool)
    for k, total in (("pairs", "pairs"), ("nan_pairs", "nan_pairs"), ("summable_pairs", "summable_pairs"), ("links", "links")):
        assert int(full[k][cells].sum()) == want[total], k
    assert np.array_equal(full["rec_within"].sum(axis=1), want["within"])
    assert np.array_equal(full["rec_summable"].sum(axis=1), want["summable"])
    if measure == "n":   # integer sums add exactly in double
        assert np.array_equal(full["rec_sum"].sum(axis=1), want["sum"]) and full["sum"][cells].sum() == want["total_sum"]
    # some records unassigned: their pairs leave the cells, their own rows stay
    rg2 = rg.copy()
    rg2[::5] = -1
    cg2 = rg2 if square else cg
    part = group_summary(measure, vals, nr, nc, square, t, rg2, Gr, cg2, Gc)
    check_consequences(part, rg2, square)
    assert (part["pairs"] <= full["pairs"]).all() and part["pairs"].sum() < full["pairs"].sum()
    if not square:
        assert np.array_equal(part["rec_summable"], full["rec_summable"])   # the columns' labels did not change
    # min / max: the extreme payloads of the cell by the sort key, -0.0 as +0.0, NaN left out
    if measure != "n":
        assert np.isneginf(full["min"]).any() and np.isposinf(full["max"]).any()
