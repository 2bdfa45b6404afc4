"""dst_group_summary's definition (include/distance_hip.h) restated in numpy and Python integers, on top of
summary_reference and links_reference: applied to a full result (the context's own run_square / run_rect values, canonical
order) and the labels it gives what the library must return, to the bit."""
import numpy as np

from links_reference import INT_MEASURES, linked, pairs
from summary_reference import convert, fixed_point

GROUPS_MAX = 1024
NONE = 0xFFFFFFFF
QUIET_NAN = 0x7FF8000000000000
TOP = np.uint64(1 << 63)
CELL_KEYS = ("pairs", "nan_pairs", "summable_pairs", "links", "sum", "min", "max")
REC_KEYS = ("rec_within", "rec_summable", "rec_sum")


def labels_of(groups):
    """labels as int64, -1 for a record without a group (given as -1 or 2^32 - 1)"""
    g = np.asarray(groups).astype(np.int64)
    return np.where(g == NONE, -1, g)


def sort_key(measure, vals):
    """dst_nearest's sort key of every payload (uint64); NaN: all ones"""
    vals = np.ascontiguousarray(vals).reshape(-1)
    if measure in INT_MEASURES:
        return vals.astype(np.int64).view(np.uint64) ^ TOP
    b = vals.astype(np.float64).view(np.uint64)
    mag = b & ~TOP
    key = np.where(b >> np.uint64(63) != 0, ~b, b | TOP)
    key = np.where(mag == 0, TOP, key)
    return np.where(mag > np.uint64(0x7FF0000000000000), np.uint64(0xFFFFFFFFFFFFFFFF), key)


def payload_of_key(measure, key):
    key = np.asarray(key, np.uint64)
    if measure in INT_MEASURES:
        return key ^ TOP
    return np.where(key & TOP != 0, key & ~TOP, ~key)


def _converted(measure, sums):
    """exact integer sums (int64 or Python ints) to double once each"""
    flat = sums.reshape(-1)
    if flat.dtype == object:
        out = np.array([convert(measure, int(s)) for s in flat], np.float64)
    else:
        out = flat.astype(np.float64)   # (round to nearest even, as float(int))
        if measure not in INT_MEASURES:
            out = np.ldexp(out, -37)
    return out.reshape(sums.shape)


def group_summary(measure, vals, n_rows, n_cols, square, threshold, row_group, n_row_groups, col_group=None, n_col_groups=None):
    """The dict Engine.group_summary returns with per_record=True."""
    vals = np.asarray(vals).reshape(-1)
    i, j = pairs(n_rows, n_cols, square)
    i, j = i.astype(np.int64), j.astype(np.int64)
    assert len(vals) == len(i)
    rg = labels_of(row_group)
    Gr = int(n_row_groups)
    cg, Gc = (rg, Gr) if square else (labels_of(col_group), int(n_col_groups))
    assert len(rg) == n_rows and len(cg) == n_cols
    assert rg.max(initial=-1) < Gr and cg.max(initial=-1) < Gc
    link = linked(measure, vals, threshold)
    ok, q = fixed_point(measure, vals)
    nan = np.zeros(len(vals), bool) if measure in INT_MEASURES else np.isnan(vals)
    key = sort_key(measure, vals)
    gi, gj = rg[i], cg[j]
    wide = int(np.abs(q).max(initial=0)) * max(len(q), 1) >= 2 ** 62   # an int64 sum could overflow: Python ints
    qs = q.astype(object) if wide else q

    def table(shape):
        return (np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.zeros(shape, object if wide else np.int64))

    def add(tab, at, keep):
        """the pairs `keep`, each to entry at[0][k], at[1][k]"""
        w, s, t = tab
        a, b = at[0][keep], at[1][keep]
        np.add.at(w, (a, b), link[keep].astype(np.int64))
        np.add.at(s, (a, b), ok[keep].astype(np.int64))
        np.add.at(t, (a, b), np.where(ok[keep], qs[keep], 0))

    rec = table((n_rows, Gc))
    add(rec, (i, gj), gj >= 0)
    if square:
        add(rec, (j, gi), gi >= 0)
    cell = table((Gr, Gc))
    both = (gi >= 0) & (gj >= 0)
    add(cell, (gi, gj), both)
    n_nan = np.zeros((Gr, Gc), np.int64)
    np.add.at(n_nan, (gi[both & nan], gj[both & nan]), 1)
    kmin = np.full((Gr, Gc), 0xFFFFFFFFFFFFFFFF, np.uint64)
    kmax = np.zeros((Gr, Gc), np.uint64)
    real = both & ~nan
    np.minimum.at(kmin, (gi[real], gj[real]), key[real])
    np.maximum.at(kmax, (gi[real], gj[real]), key[real])
    n_real = np.zeros((Gr, Gc), np.int64)
    np.add.at(n_real, (gi[real], gj[real]), 1)
    row_size = np.bincount(rg[rg >= 0], minlength=Gr).astype(np.int64)
    col_size = np.bincount(cg[cg >= 0], minlength=Gc).astype(np.int64)
    n_pairs = np.outer(row_size, col_size)
    if square:
        # a pair (i, j) was entered at (group of i, group of j): the cell of the other order holds the rest of it
        off = ~np.eye(Gr, dtype=bool)
        cell = tuple(np.where(off, x + x.T, x) for x in cell)
        n_nan = np.where(off, n_nan + n_nan.T, n_nan)
        n_real = np.where(off, n_real + n_real.T, n_real)
        kmin = np.where(off, np.minimum(kmin, kmin.T), kmin)
        kmax = np.where(off, np.maximum(kmax, kmax.T), kmax)
        n_pairs[np.diag_indices(Gr)] = row_size * (row_size - 1) // 2
    value = np.int64 if measure in INT_MEASURES else np.float64
    empty = np.uint64(0 if measure in INT_MEASURES else QUIET_NAN)
    lo = np.where(n_real > 0, payload_of_key(measure, kmin), empty).astype(np.uint64)
    hi = np.where(n_real > 0, payload_of_key(measure, kmax), empty).astype(np.uint64)
    return {"pairs": n_pairs.astype(np.uint64), "nan_pairs": n_nan.astype(np.uint64),
            "summable_pairs": cell[1].astype(np.uint64), "links": cell[0].astype(np.uint64), "sum": _converted(measure, cell[2]),
            "min": lo.view(value), "max": hi.view(value),
            "rec_within": rec[0].astype(np.uint32), "rec_summable": rec[1].astype(np.uint32), "rec_sum": _converted(measure, rec[2])}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a


def assert_group_summary(got, want, what=""):
    """integers equal, doubles bitwise; `got` may lack the per-record tables"""
    for k in CELL_KEYS + tuple(k for k in REC_KEYS if k in got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)


def check_consequences(res, row_group, square):
    """what the header states follows from the definition, on a result with the per-record tables (the sums compared as
    the counts are: `sum` itself is rounded, so only the integer tables are summed)"""
    rg = labels_of(row_group)
    Gr, Gc = res["pairs"].shape
    for name, cell in (("rec_within", "links"), ("rec_summable", "summable_pairs")):
        for a in range(Gr):
            tot = res[name][rg == a].astype(np.int64).sum(axis=0)
            for b in range(Gc):
                if square and a == b:
                    assert tot[b] % 2 == 0 and tot[b] // 2 == int(res[cell][a, b]), (name, a, b)
                else:
                    assert tot[b] == int(res[cell][a, b]), (name, a, b)
    assert (res["nan_pairs"] + res["summable_pairs"] <= res["pairs"]).all()
    assert (res["links"] <= res["pairs"]).all()
    if square:
        for k in CELL_KEYS:
            assert np.array_equal(bits(res[k]), bits(res[k].T)), k
